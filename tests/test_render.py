"""Depth / segmentation cameras: mjcf <camera> -> MjModel.camera, create_render_context, render, camera_rays, get_depth, get_segmentation
(mujoco_warp_amd/render.py, csrc/render.hpp).

The tile kernel is checked against rays() -- the same device functions on the same float32 rays (camera_rays' output): geom ids, planar depth
(dist * -ray_cam.z, 1e-6 relative) and normals (1e-6) must agree on every pixel; images of more than 128 pixels may differ in geom id on at
most 0.5 % of their pixels, each of which must have a 4-neighbour whose rays() geom id equals the rendered one (a silhouette flip) -- against
the numpy brute force of tests/ray_bruteforce.py (1e-4, where the nearest and the second-nearest geom are more than 1e-4 apart), and against
closed forms."""

import copy
import types as pytypes

import numpy as np
import pytest

import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi
from mujoco_warp_amd.device import DeviceArray
from tests import ray_bruteforce as bf


def _vstr(v):
  return " ".join(f"{x:.9g}" for x in np.asarray(v).reshape(-1))


_PHI = (1.0 + 5.0**0.5) / 2.0
ICO_V = 0.4 * np.array([[0, s1, s2 * _PHI] for s1 in (-1, 1) for s2 in (-1, 1)] + [[s1, s2 * _PHI, 0] for s1 in (-1, 1) for s2 in (-1, 1)]
                       + [[s2 * _PHI, 0, s1] for s1 in (-1, 1) for s2 in (-1, 1)]) / np.sqrt(1.0 + _PHI**2)  # 12 vertices, radius 0.4
_HF = "0.1 0.4 0.3 0.2  0.5 0.9 0.6 0.3  0.2 0.7 1.0 0.4  0.0 0.3 0.5 0.2"

MIXED = f"""
<mujoco>
  <asset>
    <mesh name="ico" vertex="{_vstr(ICO_V)}"/>
    <hfield name="bumps" nrow="4" ncol="4" size="0.6 0.5 0.4 0.1" elevation="{_HF}"/>
  </asset>
  <worldbody>
    <camera name="A" pos="0.2 -0.1 5" euler="8 -5 20" resolution="9 7"/>
    <geom name="plane" type="plane" size="5 5 .1"/>
    <geom name="sphere" type="sphere" pos="0 0 0.6" size="0.5"/>
    <geom name="capsule" type="capsule" pos="1.2 1.0 0.8" quat="0 0.3826834 0 0.9238795" size="0.2 0.4"/>
    <geom name="ellipsoid" type="ellipsoid" pos="-1.2 1.0 0.6" euler="10 20 30" size="0.5 0.3 0.2"/>
    <geom name="cylinder" type="cylinder" pos="1.3 -1.0 0.5" euler="30 0 0" size="0.3 0.4"/>
    <geom name="box" type="box" pos="-1.2 -1.1 0.5" euler="0 15 40" size="0.4 0.25 0.3"/>
    <geom name="ico" type="mesh" mesh="ico" pos="0 1.5 0.9" euler="10 20 30"/>
    <geom name="bumps" type="hfield" hfield="bumps" pos="0.3 -1.6 0.1" euler="0 0 15"/>
    <geom name="ghost" type="sphere" pos="0 0 2" size="0.6" rgba="1 1 1 0"/>
    <geom name="masked" type="box" pos="0.8 0 1.5" size="0.4 0.4 0.1" group="3"/>
    <body name="crate" pos="-0.4 0.3 1.6" euler="20 30 40"><freejoint/><geom name="crate" type="box" size="0.25 0.2 0.15"/></body>
    <body name="rover" pos="-3.2 0 1.0"><freejoint/><geom name="head" type="sphere" size="0.15"/>
      <camera name="B" pos="0.02 0 0.03" euler="90 -80 0" fovy="70" resolution="16 8"/></body>
  </worldbody>
</mujoco>
"""
MANY = ("<mujoco><worldbody><camera name='top' pos='0 0 3' resolution='8 8' fovy='54.7'/>"
        + "".join(f"<geom name='s{k}' type='sphere' size='0.14' pos='{0.3 * (k % 10) - 1.35:.3f} {0.3 * (k // 10) - 0.9:.3f} 0.1'/>" for k in range(69))
        + "<body name='last' pos='1.35 0.9 0.1'><freejoint/><geom name='s69' type='sphere' size='0.14'/></body></worldbody></mujoco>")
PLANE = ("<mujoco><worldbody><camera name='down' pos='0 0 2' resolution='9 7'/><geom name='floor' type='plane' size='0 0 .1'/>{extra}"
         "<body pos='5 5 5'><freejoint/><geom size='.05'/></body></worldbody></mujoco>")
GROUPS = (0, 1, 2)
GEOMGROUP = [1, 1, 1, 0, 0, 0]


def _mixed_q(mjm):
  q = np.tile(mjm.qpos0, (3, 1))
  q[1, :3] += [0.3, -0.2, 0.2]
  q[1, 7:10] += [0.1, 0.3, 0.2]
  q[2, :7] = [-0.7, 0.1, 1.3, *(np.array([0.8, -0.3, 0.4, 0.2]) / np.linalg.norm([0.8, -0.3, 0.4, 0.2]))]
  q[2, 7:14] = [-3.0, -0.4, 1.3, *(np.array([0.99, 0.05, -0.08, 0.06]) / np.linalg.norm([0.99, 0.05, -0.08, 0.06]))]
  return q


def _many_q(mjm):
  q = np.tile(mjm.qpos0, (2, 1))
  q[1, :3] += [0.0, 0.4, 0.3]
  return q


def _quat_mat(q):
  w, x, y, z = q
  return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# ---------------------------------------------------------------------------------------------------------------- host
def test_loader_compiles_cameras_beside_the_model():
  mjm = mjw.mjcf.from_xml_string(MIXED)
  cam = mjm.camera
  assert cam.n == 2 and cam.names == ["A", "B"] and list(cam.bodyid) == [0, mjm.body_names.index("rover")] and cam.mode == ["fixed", "fixed"]
  assert np.allclose(cam.pos, [[0.2, -0.1, 5], [0.02, 0, 0.03]]) and np.allclose(cam.fovy, [45, 70]) and cam.resolution.tolist() == [[9, 7], [16, 8]]
  assert np.allclose(np.linalg.norm(cam.quat, axis=1), 1.0)
  # euler="90 -80 0": the camera looks (its -z) along world (sin 80, cos 80, 0)-ish: x (90) then y (-80), intrinsic
  look = _quat_mat(cam.quat[1]) @ [0, 0, -1.0]
  c, s = np.cos(np.radians(80)), np.sin(np.radians(80))
  assert np.allclose(look, [s, c, 0], atol=1e-12) and np.allclose(_quat_mat(cam.quat[1]) @ [0, 1.0, 0], [0, 0, 1], atol=1e-12)
  assert mjm.ncam == 0 and mjw.put_model(mjm).ncam == 0  # the step's model is as it was
  # defaults and childclass
  m2 = mjw.mjcf.from_xml_string('<mujoco><default><camera fovy="30"/><default class="wide"><camera fovy="100" resolution="4 3"/></default></default><worldbody>'
                                '<camera name="a"/><body childclass="wide"><freejoint/><geom size=".1"/><camera name="b" pos="1 2 3" zaxis="0 1 0"/>'
                                '<camera name="c" class="main" xyaxes="0 1 0 0 0 1" mode="track"/></body></worldbody></mujoco>')
  assert m2.camera.names == ["a", "b", "c"] and np.allclose(m2.camera.fovy, [30, 100, 30]) and m2.camera.resolution.tolist() == [[1, 1], [4, 3], [1, 1]]
  assert np.allclose(_quat_mat(m2.camera.quat[1]) @ [0, 0, 1.0], [0, 1, 0], atol=1e-12) and np.allclose(_quat_mat(m2.camera.quat[2])[:, 0], [0, 1, 0], atol=1e-12)
  assert m2.camera.unbuilt == [[], [], [("mode", "track")]] and m2.ncam == 0


def test_pixel_rays_follow_the_closed_form():
  mjm = mjw.mjcf.from_xml_string(MIXED)
  rc = mjw.create_render_context(mjm, nworld=1)
  assert rc.ray.shape == (9 * 7 + 16 * 8, 3) and rc.ray.dtype == np.float32 and rc.npixel == 191
  assert np.abs(np.linalg.norm(rc.ray.astype(np.float64), axis=1) - 1.0).max() < 2e-7
  for k, (w, h, fovy) in enumerate(((9, 7, 45.0), (16, 8, 70.0))):
    r = rc.ray[rc.depth_adr[k] : rc.depth_adr[k] + w * h].reshape(h, w, 3).astype(np.float64)
    t = np.tan(np.radians(fovy) / 2)
    for py in range(h):
      for px in range(w):
        want = np.array([t * (w / h) * (2 * (px + 0.5) / w - 1), t * (1 - 2 * (py + 0.5) / h), -1.0])
        assert np.abs(r[py, px] - want / np.linalg.norm(want)).max() < 2e-7, (k, px, py)
    assert (r[..., 2] < 0).all() and r[0, 0, 1] > 0 and r[0, 0, 0] < 0  # looks along -z; row 0 is the top, column 0 the left
    for a, b, sx, sy in (((0, 0), (0, w - 1), -1, 1), ((0, 0), (h - 1, 0), 1, -1), ((0, 0), (h - 1, w - 1), -1, -1)):  # the corners mirror each other
      assert np.abs(r[a] - r[b] * [sx, sy, 1]).max() < 2e-7
    assert abs(r[0, 0, 1] / -r[0, 0, 2] - t * (1 - 1 / h)) < 1e-6  # tan of the top row's vertical angle


def test_context_layout_and_camera_selection():
  mjm = mjw.mjcf.from_xml_string(MIXED)
  rc = mjw.create_render_context(mjm, nworld=3, render_seg=True, render_normal=True)
  assert rc.ncam == 2 and list(rc.cam_id) == [0, 1] and list(rc.depth_adr) == [0, 63] and list(rc.seg_adr) == [0, 63] and rc.cam_res.tolist() == [[9, 7], [16, 8]]
  assert rc.depth_data.shape == (3, 191) and rc.seg_data.shape == (3, 191, 2) and rc.normal_data.shape == (3, 191, 3)
  assert rc.cam_xpos.shape == (3, 2, 3) and rc.cam_xmat.shape == (3, 2, 9) and np.allclose(rc.cam_fovy, [45, 70])
  assert list(rc.cam_bodyid) == [0, mjm.body_names.index("rover")] and np.allclose(rc.cam_pos, mjm.camera.pos) and np.allclose(rc.cam_quat, mjm.camera.quat)
  assert len(rc.tile) == 2 * 1 + 2 * 1 and rc.tile.tolist() == [[0, 0, 0], [0, 8, 0], [1, 0, 0], [1, 8, 0]]
  assert mjw.create_render_context(mjm, nworld=1).normal_data is None
  for sel in (["B"], [1], [False, True]):
    one = mjw.create_render_context(mjm, nworld=2, cam_active=sel)
    assert one.ncam == 1 and list(one.cam_id) == [1] and list(one.depth_adr) == [0] and one.npixel == 128 and one.cam_res.tolist() == [[16, 8]]
  both = mjw.create_render_context(mjm, nworld=1, cam_res=[(4, 3), (10, 20)], cam_active=["B", "A"])
  assert list(both.cam_id) == [1, 0] and list(both.depth_adr) == [0, 12] and both.npixel == 212 and len(both.tile) == 1 + 2 * 3
  assert mjw.create_render_context(mjm, nworld=1, cam_res=(64, 48)).cam_res.tolist() == [[64, 48], [64, 48]]
  ex = mjw.create_render_context(mjm, nworld=1, exclude_camera_body=True)
  assert list(ex.cam_exclude) == [0, mjm.body_names.index("rover")] and list(rc.cam_exclude) == [-1, -1]
  with pytest.raises(ValueError):
    mjw.create_render_context(mjm, nworld=1, cam_active=["nobody"])
  with pytest.raises(ValueError):
    mjw.create_render_context(mjm, nworld=1, cam_res=[(4, 3)])


def test_refusals():
  mjm = mjw.mjcf.from_xml_string(MIXED)
  for kw in (dict(render_rgb=True), dict(use_textures=True), dict(use_shadows=True), dict(flex_render_smooth=True), dict(splat_files=["a.ply"])):
    with pytest.raises(NotImplementedError):
      mjw.create_render_context(mjm, nworld=1, **kw)
  body = '<body><freejoint/><geom size=".1"/></body><body name="t" pos="1 0 0"><freejoint/><geom size=".1"/></body>'
  for attr in ('mode="track"', 'mode="trackcom"', 'mode="targetbody" target="t"', 'mode="targetbodycom" target="t"', 'orthographic="true"', 'sensorsize="1 1"',
               'focal="1 1"', 'focalpixel="10 10"', 'principal="0 0"', 'principalpixel="1 1"'):
    m2 = mjw.mjcf.from_xml_string(f'<mujoco><worldbody><camera name="ok"/><camera name="odd" {attr}/>{body}</worldbody></mujoco>')
    mjw.put_model(m2)  # the model loads as before ...
    assert mjw.create_render_context(m2, nworld=1, cam_active=["ok"]).ncam == 1  # ... and renders through its other cameras
    with pytest.raises(NotImplementedError, match="odd.*" + attr.split("=")[0]):
      mjw.create_render_context(m2, nworld=1)
  # visible mesh geoms without triangles in an enabled group: the error rays() raises
  bare = copy.deepcopy(mjm)
  bare.mesh_face, bare.mesh_faceadr, bare.nmeshface = np.zeros((0, 3), dtype=np.int32), np.zeros(1, dtype=np.int32), 0
  with pytest.raises(NotImplementedError, match="no triangles"):
    mjw.create_render_context(bare, nworld=1)
  bare.geom_group[list(bare.geom_names).index("ico")] = 2
  assert mjw.create_render_context(bare, nworld=1, enabled_geom_groups=(0, 1)).groupmask == 3
  # rays(rc=...) still raises, and points to render()
  z = lambda *sh: DeviceArray.zeros(sh, np.float32)
  with pytest.raises(NotImplementedError, match="render"):
    mjw.rays(None, None, z(1, 1, 3), z(1, 1, 3), None, True, None, z(1, 1), None, None, rc=mjw.create_render_context(mjm, nworld=1))
  rc = mjw.create_render_context(mjm, nworld=2, render_seg=True)
  for shape in ((2, 9, 7), (2, 7, 8), (1, 7, 9)):
    with pytest.raises(ValueError):
      mjw.get_depth(rc, 0, 1.0, z(*shape))
  with pytest.raises(ValueError):
    mjw.get_depth(rc, 2, 1.0, z(2, 7, 9))
  with pytest.raises(ValueError):
    mjw.get_segmentation(rc, 1, DeviceArray.zeros((2, 8, 16), np.int32))


def test_abi_exports_the_render_entry_points():
  L = _abi.lib()
  assert hasattr(L, "mjh_render") and hasattr(L, "mjh_camera_rays") and {"mjh_render", "mjh_camera_rays"} <= set(_abi.FUNCTIONS)
  assert L.mjh_abi_version() == 45 == _abi.DEFINES["MJH_ABI_VERSION"]
  assert [n for n, _, _ in _abi.RENDER_FIELDS][:5] == ["nworld", "ncam", "npixel", "ntile", "groupmask"]


# ---------------------------------------------------------------------------------------------------------------- GPU
def _setup(xml, q, **kw):
  mjm = mjw.mjcf.from_xml_string(xml)
  q = q(mjm) if callable(q) else q
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=len(q))
  d.qpos.assign(np.asarray(q, dtype=np.float32))
  mjw.kinematics(m, d)
  kw.setdefault("enabled_geom_groups", GROUPS)
  rc = mjw.create_render_context(mjm, nworld=len(q), render_depth=True, render_seg=True, render_normal=True, **kw)
  return mjm, m, d, rc


def _render(m, d, rc):
  mjw.render(m, d, rc)
  return rc.depth_data.numpy().copy(), rc.seg_data.numpy().copy(), rc.normal_data.numpy().copy()


def _rays_image(m, d, rc):
  """The parent's way to the same image: the pixel rays through rays(), same group mask, static geoms hit, same bodyexclude."""
  n = rc.npixel
  pnt, vec = DeviceArray.zeros((d.nworld, n, 3)), DeviceArray.zeros((d.nworld, n, 3))
  mjw.camera_rays(m, d, rc, pnt, vec)
  ex = np.concatenate([np.full(w * h, rc.cam_exclude[k], dtype=np.int32) for k, (w, h) in enumerate(rc.cam_res)])
  dist, gid, nrm = DeviceArray.zeros((d.nworld, n)), DeviceArray.zeros((d.nworld, n), np.int32), DeviceArray.zeros((d.nworld, n, 3))
  mjw.rays(m, d, pnt, vec, GEOMGROUP, True, DeviceArray.from_numpy(ex), dist, gid, nrm)
  return pnt.numpy().copy(), vec.numpy().copy(), dist.numpy().copy(), gid.numpy().copy(), nrm.numpy().copy()


def _compare_with_rays(label, m, d, rc):
  depth, seg, nrm = _render(m, d, rc)
  _, vec, rd, rg, rn = _rays_image(m, d, rc)
  assert np.abs(np.linalg.norm(vec, axis=2) - 1).max() < 1e-5
  want_depth = np.where(rg >= 0, rd * -rc.ray[None, :, 2], 0.0)
  seen = set()
  for w in range(d.nworld):
    for k, (wd, ht) in enumerate(rc.cam_res):
      sl = slice(rc.depth_adr[k], rc.depth_adr[k] + wd * ht)
      got, want = seg[w, sl, 0].reshape(ht, wd), rg[w, sl].reshape(ht, wd)
      differ = got != want
      cap = 0 if wd * ht <= 128 else int(0.005 * wd * ht)
      print(f"{label} world {w} camera {k} ({wd}x{ht}): pixels {wd * ht}, hits {(want >= 0).sum()}, geoms {sorted(set(want.ravel()))}, geom id differs on {differ.sum()} (cap {cap})")
      assert differ.sum() <= cap, (label, w, k, int(differ.sum()), cap)
      for y, x in zip(*np.nonzero(differ)):  # a silhouette flip: a neighbour of the pixel shows the rendered geom in rays()' image
        nb = [want[yy, xx] for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= yy < ht and 0 <= xx < wd]
        assert got[y, x] in nb, (label, w, k, x, y, got[y, x], want[y, x], nb)
      same = ~differ.ravel()
      assert (seg[w, sl, 1][same] == np.where(want.ravel()[same] >= 0, int(mjw.ObjType.GEOM), -1)).all()
      a, b = depth[w, sl][same], want_depth[w, sl][same]
      assert (np.abs(a - b) <= 1e-6 * np.abs(b)).all(), (label, w, k, np.abs(a - b).max())
      assert (a[want.ravel()[same] < 0] == 0).all()
      assert np.abs(nrm[w, sl][same] - rn[w, sl][same]).max() <= 1e-6, (label, w, k)
      seen |= set(int(g) for g in got.ravel())
  return seen, seg


@pytest.mark.gpu
@pytest.mark.parametrize("exclude", [False, True])
def test_gpu_render_equals_rays_mixed(exclude):
  mjm, m, d, rc = _setup(MIXED, _mixed_q, exclude_camera_body=[False, exclude])
  seen, seg = _compare_with_rays(f"mixed exclude={exclude}", m, d, rc)
  names = list(mjm.geom_names)
  assert not seen & {names.index("ghost"), names.index("masked")}  # alpha 0; group 3
  b = seg[:, 63:, 0]
  if exclude:
    assert {names.index(n) for n in ("plane", "sphere", "capsule", "ellipsoid", "cylinder", "box", "ico", "bumps", "crate")} <= seen, sorted(seen)
    assert not (b == names.index("head")).any() and len(set(b.ravel())) >= 4
    assert (seg[0] != seg[1]).any() and (seg[0] != seg[2]).any()  # the worlds differ
  else:
    assert (b == names.index("head")).all()  # camera B sits inside its body's sphere


@pytest.mark.gpu
def test_gpu_render_equals_rays_many():
  mjm, m, d, rc = _setup(MANY, _many_q)
  assert mjm.ngeom == 70  # two chunks of the cull loop
  seen, seg = _compare_with_rays("many", m, d, rc)
  assert len(seen - {-1}) >= 20 and max(seen) >= 64 and (seg[0] != seg[1]).any(), sorted(seen)


@pytest.mark.gpu
def test_gpu_render_equals_rays_mixed_64x48():
  mjm, m, d, rc = _setup(MIXED, _mixed_q, cam_res=(64, 48), exclude_camera_body=[False, True])
  seen, _ = _compare_with_rays("mixed 64x48", m, d, rc)
  assert len(seen) >= 10


@pytest.mark.gpu
def test_gpu_render_vs_bruteforce():
  """World 0 of `mixed`, camera A, against float64 numpy: meshes and height fields by tests/ray_bruteforce.py at the poses read back from the
  device, primitives by the oracle's primitive walk with every other geom made invisible (one distance per geom)."""
  from oracle import ref

  mjm, m, d, rc = _setup(MIXED, _mixed_q, cam_active=["A"])
  depth, seg, _ = _render(m, d, rc)
  pnt, vec, _, _, _ = _rays_image(m, d, rc)
  p, v = pnt[0].astype(np.float64), vec[0].astype(np.float64)
  pose = pytypes.SimpleNamespace(geom_xpos=d.geom_xpos.numpy()[0].astype(np.float64), geom_xmat=d.geom_xmat.numpy()[0].astype(np.float64))
  dist = np.full((rc.npixel, mjm.ngeom), np.inf)
  for g, tri, _ in bf.Caster(mjm, pose).geoms:
    if not bf.eliminated(mjm, g, GEOMGROUP):
      dist[:, g] = bf.moller_trumbore(p, v, tri)[0].min(axis=1)
  for g in range(mjm.ngeom):
    if int(mjm.geom_type[g]) in (bf.MESH, bf.HFIELD):
      continue
    solo = copy.deepcopy(mjm)
    solo.geom_rgba[np.arange(mjm.ngeom) != g, 3] = 0.0
    s = ref.RefSim(solo, nconmax=16, njmax=64)
    s.qpos[:] = _mixed_q(mjm)[0]
    s.forward()
    for r in range(rc.npixel):
      x, gid, _ = s.ray(p[r], v[r], geomgroup=GEOMGROUP)
      if gid == g:
        dist[r, g] = x
  order = np.sort(dist, axis=1)
  clear = ~(order[:, 1] - order[:, 0] <= 1e-4)  # (inf - inf is nan: a pixel that hits nothing is clear)
  want_g = np.where(np.isfinite(order[:, 0]), dist.argmin(axis=1), -1)
  print(f"brute force: pixels {rc.npixel}, clear {clear.sum()}, hits {(want_g >= 0).sum()}, geoms {sorted(set(want_g))}")
  assert clear.sum() >= 0.9 * rc.npixel and len(set(want_g)) >= 6
  assert (seg[0, :, 0][clear] == want_g[clear]).all(), (seg[0, :, 0], want_g)
  hit = clear & (want_g >= 0)
  got_dist = depth[0] / -rc.ray[:, 2]
  assert np.abs(got_dist[hit] - order[hit, 0]).max() < 1e-4
  assert (depth[0][clear & (want_g < 0)] == 0).all()


@pytest.mark.gpu
def test_gpu_closed_forms():
  mjm, m, d, rc = _setup(PLANE.format(extra=""), lambda mjm: np.tile(mjm.qpos0, (1, 1)))
  depth, seg, nrm = _render(m, d, rc)
  assert (np.abs(depth[0] - 2.0) <= 2e-6).all() and (seg[0] == [0, int(mjw.ObjType.GEOM)]).all() and np.abs(nrm[0] - [0, 0, 1]).max() < 1e-6
  mjm, m, d, rc = _setup(PLANE.format(extra="<geom name='ball' pos='0 0 0' size='0.25'/>"), lambda mjm: np.tile(mjm.qpos0, (1, 1)))
  depth, seg, _ = _render(m, d, rc)
  centre = 3 * 9 + 4
  assert abs(depth[0, centre] - 1.75) <= 1.75e-6 and tuple(seg[0, centre]) == (1, int(mjw.ObjType.GEOM))
  floor = seg[0, :, 0] == 0  # (the ball, 0.25 against a pixel pitch of 0.24 at the floor, also covers part of the centre pixel's neighbours)
  assert (np.abs(depth[0, floor] - 2.0) <= 2e-6).all() and floor.sum() >= 63 - 9 and set(seg[0, ~floor, 0]) == {1}
  assert ((depth[0, ~floor] >= 1.75) & (depth[0, ~floor] < 2.0)).all()
  # a finite floor: the corner pixels look past it
  mjm, m, d, rc = _setup(PLANE.format(extra="").replace("size='0 0 .1'", "size='0.5 0.5 .1'"), lambda mjm: np.tile(mjm.qpos0, (1, 1)))
  depth, seg, nrm = _render(m, d, rc)
  assert depth[0, 0] == 0 and tuple(seg[0, 0]) == (-1, -1) and (nrm[0, 0] == 0).all() and depth[0, centre] > 0 and (seg[0, :, 0] == -1).sum() >= 4


@pytest.mark.gpu
def test_gpu_camera_frames():
  mjm, m, d, rc = _setup(MIXED, _mixed_q)
  _render(m, d, rc)
  xpos, xmat = d.xpos.numpy().astype(np.float64), d.xmat.numpy().astype(np.float64).reshape(3, -1, 3, 3)
  cp, cm = rc.cam_xpos.numpy(), rc.cam_xmat.numpy().reshape(3, 2, 3, 3)
  for w in range(3):
    for k in range(2):
      b = int(rc.cam_bodyid[k])
      assert np.abs(cp[w, k] - (xpos[w, b] + xmat[w, b] @ mjm.camera.pos[k])).max() < 1e-6 * max(1.0, np.abs(xpos[w, b]).max())
      assert np.abs(cm[w, k] - xmat[w, b] @ _quat_mat(mjm.camera.quat[k])).max() < 1e-6
  assert np.abs(cp[0, 1] - cp[1, 1]).max() > 0.1 and np.abs(cm[0, 1] - cm[2, 1]).max() > 0.01 and (cp[0, 0] == cp[2, 0]).all()


@pytest.mark.gpu
def test_gpu_get_depth_and_segmentation():
  mjm, m, d, rc = _setup(MIXED, _mixed_q, exclude_camera_body=[False, True])
  depth, seg, _ = _render(m, d, rc)
  for k, (w, h) in enumerate(((9, 7), (16, 8))):
    out, sout = DeviceArray.zeros((3, h, w)), DeviceArray.zeros((3, h, w, 2), np.int32)
    sl = slice(rc.depth_adr[k], rc.depth_adr[k] + w * h)
    for scale in (1.0, 4.0, 10.0):
      mjw.get_depth(rc, k, scale, out)
      assert np.abs(out.numpy() - np.clip(depth[:, sl] / np.float32(scale), 0, 1).reshape(3, h, w)).max() <= 1e-7
    assert out.numpy().max() < 1 and out.numpy().std() > 0.01  # (scale 10: nothing clamped, a real image)
    mjw.get_segmentation(rc, k, sout)
    assert (sout.numpy() == seg[:, sl].reshape(3, h, w, 2)).all()


@pytest.mark.gpu
def test_gpu_render_is_deterministic_and_leaves_data_alone():
  mjm, m, d, rc = _setup(MIXED, _mixed_q, exclude_camera_body=True)
  a = _render(m, d, rc)
  b = _render(m, d, rc)
  assert all((x == y).all() for x, y in zip(a, b))
  fields = ("qpos", "qvel", "qacc", "xpos", "xmat", "geom_xpos", "geom_xmat", "qacc_warmstart")

  def run(with_render):
    d2 = mjw.make_data(mjm, nworld=3)
    d2.qpos.assign(_mixed_q(mjm).astype(np.float32))
    for _ in range(3):
      mjw.step(m, d2)
      if with_render:
        mjw.render(m, d2, rc)
    return [getattr(d2, f).numpy().copy() for f in fields]

  for f, x, y in zip(fields, run(False), run(True)):
    assert (x == y).all(), f
