"""Cost of actuator / sensor delays (csrc/history.hpp: k_history_ctrl in front of the step, k_history_sensor behind the sensor launch): time per
step of the benchmark humanoid with delay = 0.02, nsample = 3 on all of its actuators plus three delayed sensors, against the same model (the same
three sensors) without the delay attributes.  One process, variants interleaved, HIP events.
python tools/history_cost.py [nworld] [out file]
Both variants get the benchmark's control noise; in the delayed model it is a launch of its own in front of k_history_ctrl (in the other it rides with
the position launch), which is part of what the feature costs."""
import os, sys
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import mujoco_warp_amd as mjw

nworld = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
HUMANOID = os.path.join(ROOT, "benchmarks", "humanoid", "humanoid.xml")
DELAY = dict(delay="0.02", nsample="3")


def humanoid(delayed):
  root = ET.parse(HUMANOID).getroot()
  acts = list(root.find("actuator"))
  joints = [e.get("joint") for e in acts if e.get("joint")]
  if delayed:
    for e in acts:
      e.attrib.update(DELAY)
  sens = root.find("sensor")
  if sens is None:
    sens = ET.SubElement(root, "sensor")
  extra = DELAY if delayed else {}
  ET.SubElement(sens, "jointpos", joint=joints[0], **extra)
  ET.SubElement(sens, "jointvel", joint=joints[1], **extra)
  ET.SubElement(sens, "subtreecom", body="torso", **extra)
  return mjw.mjcf.from_xml_string(ET.tostring(root, encoding="unicode"), os.path.dirname(HUMANOID))


state = {}
for name, mjm in (("humanoid_3_sensors", humanoid(False)), ("humanoid_delayed", humanoid(True))):
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=nworld, nconmax=24, njmax=64)
  mjw.reset_data_keyframe(m, d, 0)
  mjw.timed_steps(m, d, 150, step0=0)
  state[name] = (m, d, [])
for rep in range(4):
  for name, (m, d, runs) in state.items():
    ms, _ = mjw.timed_steps(m, d, 200, step0=150 + 200 * rep)
    runs.append(round(1e3 * ms / 200, 2))
print(f"# {nworld} worlds, 4 x 200 steps by HIP events after 150 warm-up steps, variants interleaved in one process; per-launch classes: timed_steps(per_kernel=True), 50 steps", file=out)
med = {}
for name, (m, d, runs) in state.items():
  _, pk = mjw.timed_steps(m, d, 50, step0=950, per_kernel=True)
  med[name] = float(np.median(runs))
  assert np.isfinite(d.qpos.numpy()).all()
  print(f"{name:20s} nhistory {m.nhistory:4d} (actuators {m.nu_history}, sensors {m.nsensor_history_posvel} + {m.nsensor_history_acc})  step median {med[name]:8.2f} us  (runs {runs})  "
        f"per-launch classes (us) { {n: round(1e3 * t / 50, 1) for n, t in zip(mjw.KERNEL_NAMES, pk) if t > 0} }", file=out)
print(f"humanoid_delayed     added per step over humanoid_3_sensors: {med['humanoid_delayed'] - med['humanoid_3_sensors']:+.2f} us", file=out)
