"""render() against rays() on the same pixel rays: humanoid (8192 worlds, the egocentric camera at 64 x 64, its own body excluded) and aloha_pot
(1024 worlds, the overhead camera at 64 x 64, geom group 2 -- the visual shells without triangles -- hidden).  rays() is given camera_rays'
output, i.e. the rays render() casts, the same group mask and bodyexclude: the way to this image before render() existed.  Device events
around INNER calls of each, warm-up first, the two alternated within every repetition; also counts the pixels on which the two images
differ.  Prints one JSON line (and writes it to argv[1] if given):

  python tools/bench_render.py profiles/render.json
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import mujoco_warp_amd as mjw
from mujoco_warp_amd.device import DeviceArray

RES, REPS, WARM, INNER = (64, 64), 10, 3, 5


def case(name, xml, nworld, camera, groups, exclude, key):
  mjm = mjw.mjcf.load_xml(xml)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=nworld, nconmax=8, njmax=8)
  rng = np.random.default_rng(0)
  q = np.tile(np.asarray(mjm.key_qpos[key] if mjm.nkey else mjm.qpos0, dtype=np.float32), (nworld, 1))
  hinge = [int(mjm.jnt_qposadr[j]) for j in range(mjm.njnt) if int(mjm.jnt_type[j]) in (2, 3)]
  q[:, hinge] += rng.uniform(-0.1, 0.1, size=(nworld, len(hinge))).astype(np.float32)
  d.qpos.assign(q)
  mjw.kinematics(m, d)
  rc = mjw.create_render_context(mjm, nworld, cam_res=RES, render_depth=True, render_seg=True, render_normal=True, enabled_geom_groups=groups,
                                 cam_active=[camera], exclude_camera_body=exclude)
  n = rc.npixel
  pnt, vec = DeviceArray.zeros((nworld, n, 3)), DeviceArray.zeros((nworld, n, 3))
  mjw.camera_rays(m, d, rc, pnt, vec)
  bufs = (pnt, vec, DeviceArray.full((n,), int(rc.cam_exclude[0]), np.int32), DeviceArray.zeros((nworld, n)), DeviceArray.zeros((nworld, n), np.int32), DeviceArray.zeros((nworld, n, 3)))
  kernel = "k_rays_group (16 lanes)" if m.nhfield > 0 or m.nmeshface > 64 * m.nmesh else "k_rays_serial_full" if m.nmeshface else "k_rays"
  return dict(name=name, m=m, d=d, rc=rc, bufs=bufs, kernel=kernel, nworld=nworld, camera=camera, ngeom=int(mjm.ngeom), nmeshface=int(m.nmeshface), groups=list(groups),
              us=dict(render=[], rays=[]))


def run(c, which):
  if which == "render":
    mjw.render(c["m"], c["d"], c["rc"])
  else:
    P, V, ex, dist, gid, nrm = c["bufs"]
    mjw.rays(c["m"], c["d"], P, V, c["rc"].geomgroup, True, ex, dist, gid, nrm)


if not torch.cuda.is_available():
  sys.exit("tools/bench_render.py needs a GPU")
cases = [case("humanoid", os.path.join(ROOT, "benchmarks", "humanoid", "humanoid.xml"), 8192, "egocentric", (0, 1, 2), True, 0),
         case("aloha_pot", os.path.join(ROOT, "benchmarks", "aloha_pot", "scene.xml"), 1024, "overhead_cam", (0, 1, 3, 4, 5), False, 0)]
for rep in range(WARM + REPS):
  for c in cases:
    for which in (("render", "rays") if rep % 2 == 0 else ("rays", "render")):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(INNER):
        run(c, which)
      e1.record()
      torch.cuda.synchronize()
      if rep >= WARM:
        c["us"][which].append(e0.elapsed_time(e1) * 1e3 / INNER)
out = dict(device=torch.cuda.get_device_name(0), resolution=list(RES), reps=REPS, calls_per_rep=INNER, cases=[])
for c in cases:
  seg, gid = c["rc"].seg_data.numpy()[..., 0], c["bufs"][4].numpy()
  r, y = float(np.median(c["us"]["render"])), float(np.median(c["us"]["rays"]))
  out["cases"].append(dict(name=c["name"], camera=c["camera"], nworld=c["nworld"], ngeom=c["ngeom"], nmeshface=c["nmeshface"], enabled_geom_groups=c["groups"], rays_kernel=c["kernel"],
                           render_us_median=round(r, 1), render_us_min=round(min(c["us"]["render"]), 1), render_us_max=round(max(c["us"]["render"]), 1),
                           rays_us_median=round(y, 1), rays_us_min=round(min(c["us"]["rays"]), 1), rays_us_max=round(max(c["us"]["rays"]), 1),
                           rays_over_render=round(y / r, 3), pixels_per_s_render=round(c["nworld"] * c["rc"].npixel / r * 1e6), hit_fraction=round(float((gid >= 0).mean()), 3),
                           geoms_seen=int(len(np.unique(gid))), pixels_differing=int((seg != gid).sum()), pixels=int(gid.size)))
line = json.dumps(out)
print(line)
if len(sys.argv) > 1:
  open(sys.argv[1], "w").write(json.dumps(out, indent=1) + "\n")
