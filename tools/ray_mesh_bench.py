"""rays() on the two mesh-heavy benchmark models: aloha_pot (8192 worlds x 256 rays) and clutter_synth (2048 x 256), one fan of rays from a
point above the scene, broadcast to every world, the arms / objects posed differently per world, the scenes as loaded (aloha_pot's visual-only
shells, geom group 2, carry no triangles and are hidden by the call's geomgroup).  Device events around mjh_rays only, warm-up
first, the two cases alternated; prints one JSON line (and writes it to argv[1] if given):

  python tools/ray_mesh_bench.py profiles/ray_mesh.json
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import mujoco_warp_amd as mjw
from mujoco_warp_amd.device import DeviceArray

NRAY, REPS, WARM = 256, 10, 3


def case(name, xml, nworld, origin, key):
  mjm = mjw.mjcf.load_xml(xml)
  m = mjw.put_model(mjm)
  # the scene as loaded; visual-only mesh geoms carry no triangles, and rays() asks the caller to hide their groups (aloha_pot: group 2)
  hidden = m._ray_unsupported_groups
  mask = [0.0 if g in hidden else 1.0 for g in range(6)] if hidden else None
  d = mjw.make_data(mjm, nworld=nworld, nconmax=8, njmax=8)
  rng = np.random.default_rng(0)
  q = np.tile(np.asarray(mjm.key_qpos[key] if mjm.nkey else mjm.qpos0, dtype=np.float32), (nworld, 1))
  hinge = [int(mjm.jnt_qposadr[j]) for j in range(mjm.njnt) if int(mjm.jnt_type[j]) in (2, 3)]
  q[:, hinge] += rng.uniform(-0.1, 0.1, size=(nworld, len(hinge))).astype(np.float32)
  d.qpos.assign(q)
  mjw.kinematics(m, d)
  a, b = rng.uniform(0, 2 * np.pi, NRAY), rng.uniform(0.05, 1.0, NRAY)
  pnt = np.tile(np.asarray(origin, dtype=np.float32), (1, NRAY, 1))
  vec = np.stack([np.sin(b) * np.cos(a), np.sin(b) * np.sin(a), -np.cos(b)], axis=1)[None].astype(np.float32)
  bufs = (DeviceArray.from_numpy(pnt), DeviceArray.from_numpy(vec), DeviceArray.full((NRAY,), -1, np.int32), DeviceArray.zeros((nworld, NRAY)),
          DeviceArray.zeros((nworld, NRAY), np.int32), DeviceArray.zeros((nworld, NRAY, 3)))
  # (the library's own choice, csrc/mjhip.hip mjh_rays: a height field, or more than 64 triangles per mesh on average -> the lane-group kernel)
  kernel = "k_rays_group (16 lanes)" if m.nhfield > 0 or m.nmeshface > 64 * m.nmesh else "k_rays_serial_full" if m.nmeshface else "k_rays"
  return dict(name=name, m=m, d=d, bufs=bufs, mask=mask, kernel=kernel, nmesh=int(m.nmesh), nworld=nworld, nmeshface=int(m.nmeshface), ngeom=int(mjm.ngeom), us=[])


def cast(c):
  P, V, ex, dist, gid, nrm = c["bufs"]
  mjw.rays(c["m"], c["d"], P, V, c["mask"], True, ex, dist, gid, nrm)


cases = [case("aloha_pot", os.path.join(ROOT, "benchmarks", "aloha_pot", "scene.xml"), 8192, [0.0, 0.0, 1.6], 0),
         case("clutter_synth", os.path.join(ROOT, "benchmarks", "clutter_synth", "scene_clutter_synth.xml"), 2048, [0.0, 0.0, 1.6], 0)]
for rep in range(WARM + REPS):
  for c in cases:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    cast(c)
    e1.record()
    torch.cuda.synchronize()
    if rep >= WARM:
      c["us"].append(e0.elapsed_time(e1) * 1e3)
out = dict(device=torch.cuda.get_device_name(0), nray=NRAY, reps=REPS, cases=[])
for c in cases:
  us = float(np.median(c["us"]))
  hit = float((c["bufs"][4].numpy() >= 0).mean())
  out["cases"].append(dict(name=c["name"], kernel=c["kernel"], nmesh=c["nmesh"], hidden_groups=c["m"]._ray_unsupported_groups, nworld=c["nworld"], ngeom=c["ngeom"], nmeshface=c["nmeshface"], us_per_launch_median=round(us, 1), us_min=round(min(c["us"]), 1),
                           us_max=round(max(c["us"]), 1), rays_per_s=round(c["nworld"] * NRAY / us * 1e6), hit_fraction=round(hit, 3)))
line = json.dumps(out)
print(line)
if len(sys.argv) > 1:
  open(sys.argv[1], "w").write(json.dumps(out, indent=1) + "\n")
