"""Outputs of rays() on the primitive-only scene of tests/test_ray.py (3 worlds, 500 rays, its four filter settings), saved as one .npz.

Run on a GPU from a checkout whose primitive ray kernel is the one to pin:

  python tools/dump_ray_primitive.py tests/golden/ray_primitive_parent.npz

tests/test_ray_mesh.py::test_gpu_primitive_models_bitwise_unchanged compares the current build with that file bit for bit."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

FILTERS = (dict(), dict(geomgroup=[1, 0, 0, 1, 1, 1]), dict(flg_static=False), dict(bodyexclude=1))


def outputs():
  """{"dist_k", "geomid_k", "normal_k"} for filter setting k, from the current build."""
  import mujoco_warp_amd as mjw
  from mujoco_warp_amd.device import DeviceArray
  from tests.test_ray import SCENE, _random_rays

  mjm = mjw.mjcf.from_xml_string(SCENE)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=3)
  q = d.qpos.numpy()
  q[1, :3] += [0.4, 0.2, 0.3]
  q[2, :3] += [1.0, 1.5, 1.0]
  d.qpos.assign(q)
  mjw.forward(m, d)
  pnt, vec = _random_rays(500, 2)
  P, V = DeviceArray.from_numpy(pnt[None].astype(np.float32)), DeviceArray.from_numpy(vec[None].astype(np.float32))
  out = {}
  for k, kw in enumerate(FILTERS):
    dist, gid, nrm = DeviceArray.zeros((3, 500)), DeviceArray.zeros((3, 500), np.int32), DeviceArray.zeros((3, 500, 3))
    ex = DeviceArray.full((500,), kw.get("bodyexclude", -1), np.int32)
    mjw.rays(m, d, P, V, kw.get("geomgroup"), kw.get("flg_static", True), ex, dist, gid, nrm)
    out[f"dist_{k}"], out[f"geomid_{k}"], out[f"normal_{k}"] = dist.numpy().copy(), gid.numpy().copy(), nrm.numpy().copy()
  return out


if __name__ == "__main__":
  o = outputs()
  np.savez_compressed(sys.argv[1], **o)
  print("wrote", sys.argv[1], {k: v.shape for k, v in o.items()})
