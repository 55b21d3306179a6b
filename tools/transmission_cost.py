"""Cost of the general transmission path (k_transmission + the velocity stage's general instantiation; a model with such an actuator also takes
k_mid's roles as launches of their own): time per step with and without the actuator, one process, variants interleaved, HIP events.
python tools/transmission_cost.py [nworld] [out file]   -- a quadrotor (one free body; four rotor sites, a joint and a jointinparent wrench) against
the same body without actuators, and the benchmark humanoid with one site motor at a hand against the humanoid as it is.  The humanoids get the
benchmark's control noise; the quadrotors run with ctrl = 0 (both drop onto the floor and rest there, so the two steps differ by the actuation
path alone -- the benchmark's correlated noise on a gear of several N m spins an undamped 4 g m^2 body up until explicit Euler diverges)."""
import os, sys
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import mujoco_warp_amd as mjw

nworld = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
HUMANOID = os.path.join(ROOT, "benchmarks", "humanoid", "humanoid.xml")
DRONE = """<mujoco><option timestep="0.002"/><worldbody><geom type="plane" size="5 5 .1"/><body name="drone" pos="0 0 1"><joint name="root" type="free"/>
  <geom type="box" size=".1 .1 .02" mass="1.2"/><site name="r0" pos=".1 .1 0"/><site name="r1" pos="-.1 .1 0"/><site name="r2" pos="-.1 -.1 0"/>
  <site name="r3" pos=".1 -.1 0"/></body></worldbody>ACT</mujoco>"""
ROTORS = """<actuator><motor site="r0" gear="0 0 1 0 0 .1" ctrlrange="0 10"/><motor site="r1" gear="0 0 1 0 0 -.1" ctrlrange="0 10"/>
  <motor site="r2" gear="0 0 1 0 0 .1" ctrlrange="0 10"/><motor site="r3" gear="0 0 1 0 0 -.1" ctrlrange="0 10"/>
  <motor joint="root" gear="1 2 3 4 5 6"/><general jointinparent="root" gear="1 2 3 4 5 6"/></actuator>"""


def humanoid_site():
  root = ET.parse(HUMANOID).getroot()
  hand = next(e for e in root.iter("body") if e.get("name") == "hand_right")
  ET.SubElement(hand, "site", name="trn_site", pos=".03 -.02 .05", quat=".8 .2 -.4 .4")
  ET.SubElement(root.find("actuator"), "motor", name="trn_motor", site="trn_site", gear=".3 -1 2 .5 0 -.7")
  return mjw.mjcf.from_xml_string(ET.tostring(root, encoding="unicode"), os.path.dirname(HUMANOID))


variants = {"drone_no_actuator": (mjw.mjcf.from_xml_string(DRONE.replace("ACT", "")), 4, 16), "drone": (mjw.mjcf.from_xml_string(DRONE.replace("ACT", ROTORS)), 4, 16),
            "humanoid": (mjw.mjcf.load_xml(HUMANOID), 24, 64), "humanoid_site_motor": (humanoid_site(), 24, 64)}
state = {}
for name, (mjm, nconmax, njmax) in variants.items():
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=nworld, nconmax=nconmax, njmax=njmax)
  if mjm.nkey:
    mjw.reset_data_keyframe(m, d, 0)
  std = -1.0 if name.startswith("drone") else 0.01  # (a negative noise_std: no control noise)
  mjw.timed_steps(m, d, 150, step0=0, noise_std=std)
  state[name] = (m, d, [], std)
for rep in range(4):
  for name, (m, d, runs, std) in state.items():
    ms, _ = mjw.timed_steps(m, d, 200, step0=150 + 200 * rep, noise_std=std)
    runs.append(round(1e3 * ms / 200, 2))
print(f"# {nworld} worlds, 4 x 200 steps by HIP events after 150 warm-up steps, variants interleaved in one process; per-launch classes: timed_steps(per_kernel=True), 50 steps", file=out)
med = {}
for name, (m, d, runs, std) in state.items():
  _, pk = mjw.timed_steps(m, d, 50, step0=950, per_kernel=True, noise_std=std)
  med[name] = float(np.median(runs))
  assert np.isfinite(d.qpos.numpy()).all()
  print(f"{name:22s} trn_general {m.trn_general}  step median {med[name]:8.2f} us  (runs {runs})  per-launch classes (us) "
        f"{ {n: round(1e3 * t / 50, 1) for n, t in zip(mjw.KERNEL_NAMES, pk) if t > 0} }", file=out)
for a, b in (("drone", "drone_no_actuator"), ("humanoid_site_motor", "humanoid")):
  print(f"{a:22s} added per step over {b}: {med[a] - med[b]:+.2f} us", file=out)
