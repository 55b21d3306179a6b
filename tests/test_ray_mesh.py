"""Rays against mesh and height-field geoms (reference ray.py _ray_triangle / ray_mesh / ray_hfield; csrc/ray.hpp k_rays_group, ray_world_full).

Ground truth is tests/ray_bruteforce.py: float64 Moeller-Trumbore over every triangle, posed with the oracle's geom_xpos / geom_xmat; the
oracle's own RefSim.ray walks primitives only and is used for those alone.  Tolerances are those of tests/test_ray.py:
|d dist| < 2e-5 max(1, dist), |d normal| < 2e-3, a miss is dist == -1, geomid == -1, normal exactly 0.

Grazing rays: a ray may hit in float32 and miss in float64 at a silhouette; a ray whose geomid differs from the ground truth is a flip and is
skipped, at most 1 % of a case's rays.  The ray sets (fixed seeds) are chosen so that the brute force in float32 against itself in float64
stays within half of that: test_ray_sets_are_well_conditioned asserts it on the CPU for every case and prints the counts (measured when the
sets were fixed: cube 0 / 1800, mixed 0 / 1200 under each filter, hfield 0 / 1220 with 7 of 1118 normals left out, aloha_pot 0 / 1024 with 1 of 736 left out).  Normals are compared where the
float64 hit is at least 1e-4 (barycentric) from a triangle edge -- on a shared edge two triangles tie on distance; so do the coincident
opposite faces that aloha_pot's thin parts store, which count the same way -- and the share of hits left
out that way is capped at 5 % per case, asserted in the same CPU test."""

import os

import numpy as np
import pytest

import mujoco_warp_amd as mjw
from mujoco_warp_amd.device import DeviceArray
from oracle import ref
from tests import conftest
from tests import ray_bruteforce as bf

# aloha_pot's 26 visual-only mesh geoms (group 2: no collision, no mass) are never read by the loader and carry no triangles; rays() serves the
# model when the call hides that group -- rays against the collision geometry (groups 0, 1, 3), the brute force under the same mask
ALOHA_KW = dict(geomgroup=[1, 1, 0, 1, 1, 1])
FILTERS = (dict(), dict(geomgroup=[1, 0, 0, 1, 1, 1]), dict(flg_static=False), dict(bodyexclude=1))  # (tests/test_ray.py:146)
HX, HY, HZ = 0.5, 0.25, 0.3


def _vstr(v):
  return " ".join(f"{x:.9g}" for x in np.asarray(v).reshape(-1))


CUBE_V = np.array([[sx * HX, sy * HY, sz * HZ] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
CUBE = """
<mujoco>
  <asset><mesh name="cube" vertex="{v}"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="4 4 .1" pos="0 0 -2"/>
    <body name="b" pos="0.1 -0.2 1" euler="20 30 40"><freejoint/>{geom}</body>
  </worldbody>
</mujoco>
"""
CUBE_MESH = CUBE.format(v=_vstr(CUBE_V), geom='<geom type="mesh" mesh="cube"/>')
CUBE_BOX = CUBE.format(v=_vstr(CUBE_V), geom=f'<geom type="box" size="{HX} {HY} {HZ}"/>')

# an L-shaped prism (non-convex, explicit faces): the L in the x-y plane, arms of width 0.3 and length 0.9, extruded over z in [0, 0.4]
_L2 = [(0, 0), (0.9, 0), (0.9, 0.3), (0.3, 0.3), (0.3, 0.9), (0, 0.9)]
L_V = np.array([[x, y, z] for z in (0.0, 0.4) for x, y in _L2])
_L_CAP = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]  # (a fan from the L's outer corner stays inside the L)
L_F = np.array([[c, b, a] for a, b, c in _L_CAP] + [[a + 6, b + 6, c + 6] for a, b, c in _L_CAP]
               + [t for i in range(6) for t in ([i, (i + 1) % 6, (i + 1) % 6 + 6], [i, (i + 1) % 6 + 6, i + 6])])
OCTA_V = np.array([[0.35, 0, 0], [-0.35, 0, 0], [0, 0.3, 0], [0, -0.3, 0], [0, 0, 0.45], [0, 0, -0.25]])


def _terrain(nrow, ncol, fn):
  rows = []
  for r in range(nrow):  # MJCF lists the far (+y) row first (tests/test_hfield.py:32)
    y = 1.0 - 2.0 * r / (nrow - 1)
    rows.append(" ".join(f"{fn(-1.0 + 2.0 * c / (ncol - 1), y):.6f}" for c in range(ncol)))
  return "  ".join(rows)


_HILLS = lambda x, y: 0.5 + 0.3 * np.sin(3.0 * x + 0.5) * np.cos(2.0 * y) + 0.2 * x * y
MIXED = f"""
<mujoco>
  <asset>
    <material name="glass" rgba="1 1 1 0"/>
    <mesh name="octa" vertex="{_vstr(OCTA_V)}"/>
    <mesh name="ell" vertex="{_vstr(L_V)}" face="{_vstr(L_F)}"/>
    <hfield name="hills" nrow="9" ncol="11" size="0.8 0.6 0.5 0.1" elevation="{_terrain(9, 11, _HILLS)}"/>
  </asset>
  <worldbody>
    <geom name="plane" size="4 4 4" type="plane" rgba="0.1 0.1 0.1 1"/>
    <geom name="sphere" pos="0 0 1" size="0.5" type="sphere"/>
    <geom name="capsule" pos="0 1 1" quat="0 0.3826834 0 0.9238795" size="0.25 0.5" type="capsule"/>
    <geom name="box" pos="1 0 1" euler="0 0 90" size="0.5 0.25 0.3" type="box"/>
    <geom name="octa" type="mesh" mesh="octa" pos="2 0 1" euler="10 20 30" group="2"/>
    <geom name="ell" type="mesh" mesh="ell" pos="-2 -1.2 0.8" euler="0 0 25"/>
    <geom name="hills" type="hfield" hfield="hills" pos="-1.4 0.9 0.3" euler="0 0 15" group="1"/>
    <geom name="ghost_mesh" type="mesh" mesh="octa" pos="0 0 2.5" rgba="1 1 1 0"/>
    <geom name="ghost_hills" type="hfield" hfield="hills" pos="0 0 3.2" material="glass"/>
    <geom name="masked_mesh" type="mesh" mesh="ell" pos="1.2 -1.6 0.6" group="1"/>
    <body name="mover" pos="-1 -1.5 1.6"><freejoint/><geom name="ball" size="0.2"/><geom name="rider" type="mesh" mesh="octa" pos="0.5 0 0"/></body>
  </worldbody>
</mujoco>
"""

HF_ONLY = f"""
<mujoco>
  <asset><hfield name="hills" nrow="7" ncol="9" size="1 0.8 0.6 0.2" elevation="{_terrain(7, 9, _HILLS)}"/></asset>
  <worldbody><geom name="hills" type="hfield" hfield="hills" pos="0.1 -0.1 0.2" euler="5 -4 20"/></worldbody>
</mujoco>
"""

RANGE = f"""
<mujoco>
  <option timestep="0.004"/>
  <asset>
    <mesh name="ell" vertex="{_vstr(L_V)}" face="{_vstr(L_F)}"/>
    <hfield name="hills" nrow="9" ncol="11" size="0.8 0.6 0.3 0.1" elevation="{_terrain(9, 11, _HILLS)}"/>
  </asset>
  <worldbody>
    <geom name="hills" type="hfield" hfield="hills"/>
    <geom name="ell" type="mesh" mesh="ell" pos="0.1 -0.2 0.45" euler="0 0 30"/>
    <body name="drone" pos="0.25 0 1.6" euler="8 -6 0"><freejoint/><geom size="0.05"/>
      <site name="down" pos="0 0 -.06" euler="180 0 0"/><site name="side" euler="0 100 0"/></body>
  </worldbody>
  <sensor><rangefinder site="down"/><rangefinder site="side"/></sensor>
</mujoco>
"""


def _sims(mjm, qs):
  out = []
  for q in qs:
    s = ref.RefSim(mjm, nconmax=16, njmax=64)
    s.qpos[:] = q
    s.forward()
    out.append(s)
  return out


def _aimed_rays(n, seed, lo, hi, tlo, thi):
  rng = np.random.default_rng(seed)
  pnt = rng.uniform(lo, hi, size=(n, 3))
  return pnt, rng.uniform(tlo, thi, size=(n, 3)) - pnt


def _shell_rays(n, seed, centre, radius, spread):
  """Origins on a sphere around `centre` (outside every bounding box of the case), aimed at points within `spread` of it."""
  rng = np.random.default_rng(seed)
  u = rng.normal(size=(n, 3))
  pnt = np.asarray(centre) + radius * u / np.linalg.norm(u, axis=1, keepdims=True)
  return pnt, np.asarray(centre) + rng.uniform(-1, 1, size=(n, 3)) * spread - pnt


# ---- the cases: (model, qpos per world, rays) ----
def _case_cube():
  mjm = mjw.mjcf.from_xml_string(CUBE_MESH)
  q = np.tile(mjm.qpos0, (3, 1))
  q[1, :3] += [0.3, 0.1, -0.2]
  q[2, :7] = [-0.2, 0.3, 1.3, *(np.array([0.8, -0.3, 0.4, 0.2]) / np.linalg.norm([0.8, -0.3, 0.4, 0.2]))]
  return mjm, q, _shell_rays(600, 11, [0.1, 0, 1.1], 2.5, [0.9, 0.9, 0.9])


def _case_mixed():
  mjm = mjw.mjcf.from_xml_string(MIXED)
  q = np.tile(mjm.qpos0, (2, 1))
  q[1, :3] += [0.6, 0.4, 0.3]
  pnt, vec = _aimed_rays(600, 5, [-3.5, -3.5, 2.2], [3.5, 3.5, 4.0], [-2.6, -2.2, 0.0], [2.6, 1.8, 1.4])
  return mjm, q, (pnt, vec)


def _hfield_rays():
  """Above, from the four sides (walls), from below (base box), through the boundary cells (c = ncol - 2, r = nrow - 2) and along a grid line,
  in the height field's frame (then moved to the world by the caller)."""
  rng = np.random.default_rng(21)
  P, V = [], []
  for _ in range(400):  # from above
    p = rng.uniform([-1.6, -1.4, 1.2], [1.6, 1.4, 2.0])
    P.append(p), V.append(rng.uniform([-1.1, -0.9, 0.0], [1.1, 0.9, 0.3]) - p)
  for _ in range(400):  # from the sides, roughly level: walls (and over them, the grid)
    a = rng.uniform(0, 2 * np.pi)
    p = np.array([2.2 * np.cos(a), 2.0 * np.sin(a), rng.uniform(0.02, 0.7)])
    P.append(p), V.append(rng.uniform([-0.9, -0.7, 0.0], [0.9, 0.7, 0.5]) - p)
  for _ in range(200):  # from below: the base box
    p = rng.uniform([-1.5, -1.2, -1.5], [1.5, 1.2, -0.5])
    P.append(p), V.append(rng.uniform([-0.9, -0.7, -0.1], [0.9, 0.7, 0.3]) - p)
  dx, dy = 2.0 / 8, 1.6 / 6
  for _ in range(200):  # straight down into the last cell column / row
    edge_col = rng.uniform() < 0.5
    x = rng.uniform(1.0 - dx, 1.0 - 1e-3) if edge_col else rng.uniform(-1, 1)
    y = rng.uniform(-0.8, 0.8) if edge_col else rng.uniform(0.8 - dy, 0.8 - 1e-3)
    P.append(np.array([x, y, 1.5])), V.append(np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), -1.0]))
  for k in range(20):  # along the grid line x = -1 + 3 dx, descending
    P.append(np.array([-1.0 + 3 * dx, -1.5 + 0.01 * k, 1.0 + 0.01 * k])), V.append(np.array([0.0, 1.0, -0.35]))
  return np.array(P), np.array(V)


def _case_hfield():
  mjm = mjw.mjcf.from_xml_string(HF_ONLY)
  s = _sims(mjm, [mjm.qpos0])[0]
  R, p = s.geom_xmat[0].reshape(3, 3), s.geom_xpos[0]
  P, V = _hfield_rays()
  return mjm, np.tile(mjm.qpos0, (1, 1)), (P @ R.T + p, V @ R.T)


def _aloha():
  from tests import test_aloha_pot as T

  mjm = mjw.mjcf.load_xml(T.XML)  # (the scene as loaded: nothing is edited)
  k = mjm.key_names.index("lift_pot0")
  q = np.tile(np.asarray(mjm.key_qpos[k], dtype=np.float64), (4, 1))
  rng = np.random.default_rng(3)
  for w in range(1, 4):
    q[w, :16] += rng.uniform(-0.15, 0.15, size=16)  # (the arms' joints)
  rng = np.random.default_rng(4)
  a, b = rng.uniform(0, 2 * np.pi, 256), rng.uniform(0.05, 1.0, 256)  # a fan from a point above the table, downwards
  pnt = np.tile([0.0, 0.0, 1.6], (256, 1))
  vec = np.stack([np.sin(b) * np.cos(a), np.sin(b) * np.sin(a), -np.cos(b)], axis=1)
  return mjm, q, (pnt, vec)


def _precision_counts(mjm, q, rays, filters=(dict(),)):
  """(flips, left-out normals, hits, rays) of the brute force in float32 against itself in float64, summed over worlds, per filter."""
  pnt, vec = rays
  out = []
  for kw in filters:
    flips = left = hits = 0
    for s in _sims(mjm, q):
      d64, g64, n64, e64 = bf.expected(bf.Caster(mjm, s), s, pnt, vec, **kw)
      p32, v32 = pnt.astype(np.float32), vec.astype(np.float32)
      d32, g32, _, _ = bf.expected(bf.Caster(mjm, s, np.float32), s, p32, v32, **kw)
      flips += int((g32 != g64).sum())
      hits += int((g64 >= 0).sum())
      left += int(((g64 >= 0) & (e64 < 1e-4)).sum())
    out.append((flips, left, hits, len(pnt) * len(q)))
  return out


# ---------------------------------------------------------------------------------------------------------------- host
def _faces_of(m, i):
  f1 = m.mesh_faceadr[i + 1] if i + 1 < m.nmesh else m.nmeshface
  return np.asarray(m.mesh_face)[m.mesh_faceadr[i] : f1], np.asarray(m.mesh_vert)[m.mesh_vertadr[i] : m.mesh_vertadr[i] + m.mesh_vertnum[i]]


def test_mesh_face_tables():
  # (a) inline vertices without faces: the hull's triangles, outwards, a closed surface
  rng = np.random.default_rng(0)
  pts = rng.normal(size=(40, 3)) * [0.4, 0.3, 0.2]
  m = mjw.mjcf.from_xml_string(f'<mujoco><asset><mesh name="a" vertex="{_vstr(pts)}"/><mesh name="c" vertex="{_vstr(CUBE_V)}"/></asset><worldbody>'
                               '<body><freejoint/><geom type="mesh" mesh="a"/></body><body pos="2 0 0"><freejoint/><geom type="mesh" mesh="c"/></body></worldbody></mujoco>')
  assert m.nmesh == 2 and m.mesh_face.dtype == np.int32 and m.mesh_face.shape == (m.nmeshface, 3) and m.mesh_faceadr.shape == (2,) and m.mesh_faceadr[0] == 0
  for i in range(2):
    f, v = _faces_of(m, i)
    assert f.min() >= 0 and f.max() < len(v)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("fk,fk->f", n, v[f].mean(axis=1) - v[np.unique(f)].mean(axis=0)) > 0).all()
    edges = {tuple(sorted((int(t[a]), int(t[b])))) for t in f for a, b in ((0, 1), (1, 2), (2, 0))}
    assert len(np.unique(f)) - len(edges) + len(f) == 2
  assert len(_faces_of(m, 1)[0]) == 12
  # (b) an OBJ and an STL of aloha_pot: the file's triangles (OBJ polygons as fans), indices inside the mesh's vertex block
  d = os.path.join(conftest.ROOT, "benchmarks", "aloha_pot")
  obj = sorted(f for f in os.listdir(d) if f.endswith(".obj"))[0]
  stl = sorted(f for f in os.listdir(d) if f.endswith(".stl"))[0]
  nobj = sum(len(line.split()) - 3 for line in open(os.path.join(d, obj)) if line.startswith("f "))
  nstl = int(np.frombuffer(open(os.path.join(d, stl), "rb").read()[80:84], dtype="<u4")[0])
  m = mjw.mjcf.from_xml_string(f'<mujoco><asset><mesh name="o" file="{obj}"/><mesh name="s" file="{stl}"/></asset><worldbody>'
                               '<body><freejoint/><geom type="mesh" mesh="o"/></body><body pos="2 0 0"><freejoint/><geom type="mesh" mesh="s"/></body></worldbody></mujoco>', d)
  assert [len(_faces_of(m, i)[0]) for i in range(2)] == [nobj, nstl] and m.nmeshface == nobj + nstl and list(m.mesh_faceadr) == [0, nobj]
  for i in range(2):
    f, v = _faces_of(m, i)
    assert f.min() >= 0 and f.max() < len(v)
  # (c) a mirroring scale turns the triangles over
  xml = '<mujoco><asset><mesh name="l" vertex="{v}" face="{f}" scale="{s}"/></asset><worldbody><body><freejoint/><geom type="mesh" mesh="l"/></body></worldbody></mujoco>'
  vol = []
  for sc in ("1 1 1", "1 -1 1"):
    m = mjw.mjcf.from_xml_string(xml.format(v=_vstr(L_V), f=_vstr(L_F), s=sc))
    f, v = _faces_of(m, 0)
    assert len(f) == len(L_F)
    vol.append(np.einsum("fk,fk->f", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
  assert vol[0] == pytest.approx(0.45 * 0.4, rel=1e-9) and vol[1] == pytest.approx(vol[0], rel=1e-9)  # outwards both times: the mirror flipped the order
  assert (np.asarray(mjw.mjcf.from_xml_string(xml.format(v=_vstr(L_V), f=_vstr(L_F), s="1 -1 1")).mesh_face)[:, [0, 2, 1]] == L_F).all()
  # put_model: the tables reach the device model; a visible mesh geom without triangles is still refused
  mjm = mjw.mjcf.from_xml_string(CUBE_MESH)
  dm = mjw.put_model(mjm)
  assert dm.nmeshface == 12 and tuple(dm.mesh_face.shape) == (12, 3) and tuple(dm.mesh_faceadr.shape) == (1,) and dm._ray_unsupported_geoms == 0
  mjm.mesh_face, mjm.mesh_faceadr, mjm.nmeshface = np.zeros((0, 3), dtype=np.int32), np.zeros(1, dtype=np.int32), 0
  bare = mjw.put_model(mjm)
  assert bare._ray_unsupported_geoms == 1 and bare._ray_unsupported_groups == [0]
  # several meshes (the declared schema gives Model.mesh_face no symbolic shape: checked here): shape, dtype and content of the device arrays
  mjm = mjw.mjcf.from_xml_string(MIXED)
  dm = mjw.put_model(mjm)
  assert mjm.nmesh == 2 and dm.nmesh == 2 and dm.nmeshface == mjm.nmeshface == 8 + len(L_F)
  assert tuple(dm.mesh_face.shape) == (dm.nmeshface, 3) and np.dtype(dm.mesh_face.dtype) == np.int32
  assert tuple(dm.mesh_faceadr.shape) == (dm.nmesh,) and np.dtype(dm.mesh_faceadr.dtype) == np.int32


def test_visual_only_meshes_are_refused_unless_masked():
  """aloha_pot as loaded: 26 visible mesh geoms (the visual shells, group 2) have no triangles.  rays() refuses the model -- before anything is
  launched -- unless the call's geomgroup hides group 2."""
  mjm, q, (pnt, vec) = _aloha()
  m = mjw.put_model(mjm)
  assert m.nmeshface == mjm.nmeshface > 60000 and m._ray_unsupported_geoms == 26 and m._ray_unsupported_groups == [2]
  d = mjw.make_data(mjm, nworld=1)
  z = lambda *sh, dt=np.float32: DeviceArray.zeros(sh, dt)
  for gg in (None, [-1] * 6, [1, 1, 1, 1, 1, 1], [0, 0, 1, 0, 0, 0]):
    with pytest.raises(NotImplementedError):
      mjw.rays(m, d, z(1, 4, 3), z(1, 4, 3), gg, True, None, z(1, 4), None, None)
  with pytest.raises(ValueError):  # the mask is accepted: the call goes on to its argument checks (dist of the wrong shape)
    mjw.rays(m, d, z(1, 4, 3), z(1, 4, 3), ALOHA_KW["geomgroup"], True, None, z(1, 5), None, None)


def test_bruteforce_against_closed_forms():
  # a cube mesh is a box
  mesh, box = mjw.mjcf.from_xml_string(CUBE_MESH), mjw.mjcf.from_xml_string(CUBE_BOX)
  sm, sb = _sims(mesh, [mesh.qpos0])[0], _sims(box, [box.qpos0])[0]
  pnt, vec = _case_cube()[2]
  dist, gid, nrm, _ = bf.Caster(mesh, sm).cast(pnt, vec)
  hits = 0
  for r in range(len(pnt)):
    bd, bg, bn = sb.ray(pnt[r], vec[r])
    if bg != 1:
      assert gid[r] == -1 and dist[r] == -1.0
      continue
    hits += 1
    assert gid[r] == 1 and abs(dist[r] - bd) < 1e-12 and np.abs(nrm[r] - bn).max() < 1e-9, (r, dist[r], bd, nrm[r], bn)
  assert hits > 100
  # a flat height field is a box from -base to the top
  flat = mjw.mjcf.from_xml_string('<mujoco><asset><hfield name="t" nrow="4" ncol="5" size="1 .8 .3 .2" elevation="1 1 1 1 1  1 1 1 1 1  1 1 1 1 1  1 1 1 1 1.000001"/></asset>'
                                  '<worldbody><geom type="hfield" hfield="t" pos=".1 .2 .3" euler="10 20 30"/></worldbody></mujoco>')
  flat.hfield_data[:] = 1.0  # (the loader normalises by the range: a constant elevation is written as 1 after loading)
  sf = _sims(flat, [flat.qpos0])[0]
  eq = mjw.mjcf.from_xml_string('<mujoco><worldbody><geom type="box" size="1 .8 .25" pos="0 0 .05"/></worldbody></mujoco>')
  se = _sims(eq, [eq.qpos0])[0]
  R, p = sf.geom_xmat[0].reshape(3, 3), sf.geom_xpos[0]
  P, V = _shell_rays(400, 13, [0, 0, 0.05], 3.0, [1.1, 0.9, 0.4])
  dist, gid, nrm, _ = bf.Caster(flat, sf).cast(P @ R.T + p, V @ R.T)
  hits = 0
  for r in range(len(P)):
    bd, bg, bn = se.ray(P[r], V[r])
    if bg < 0:
      assert gid[r] == -1
      continue
    hits += 1
    assert gid[r] == 0 and abs(dist[r] - bd) < 1e-12 and np.abs(nrm[r] - R @ bn).max() < 1e-9, (r, dist[r], bd)
  assert hits > 100


def test_ray_sets_are_well_conditioned():
  """The caps on flips (1 %) and on normals left out near edges (5 %) are conditions on the ray sets: the brute force alone, float32 against
  float64, must stay within half the flip cap and within the edge cap on every case."""
  for name, (mjm, q, rays), filters in (("cube", _case_cube(), (dict(),)), ("mixed", _case_mixed(), FILTERS), ("hfield", _case_hfield(), (dict(),)),
                                        ("aloha_pot", _aloha(), (ALOHA_KW,))):
    for kw, (flips, left, hits, n) in zip(filters, _precision_counts(mjm, q, rays, filters)):
      print(f"{name} {kw}: float32-vs-float64 flips {flips} / {n}, hits {hits}, normals left out {left}")
      assert flips <= 0.005 * n and left <= 0.05 * max(hits, 1) and hits > 10, (name, kw, flips, left, hits, n)


# ----------------------------------------------------------------------------------------------------------------- GPU
def _gpu_rays(mjm, q, pnt, vec, geomgroup=None, flg_static=True, bodyexclude=-1, broadcast=True, nworld=None):
  m = mjw.put_model(mjm)
  nworld = nworld or len(q)
  d = mjw.make_data(mjm, nworld=nworld)
  d.qpos.assign(np.asarray(q, dtype=np.float32) if len(q) == nworld else np.tile(np.asarray(q[:1], dtype=np.float32), (nworld, 1)))
  mjw.kinematics(m, d)
  n = len(pnt)
  shape = (1, n, 3) if broadcast else (nworld, n, 3)
  P = DeviceArray.from_numpy(np.ascontiguousarray(np.broadcast_to(pnt[None].astype(np.float32), shape)))
  V = DeviceArray.from_numpy(np.ascontiguousarray(np.broadcast_to(vec[None].astype(np.float32), shape)))
  dist, gid, nrm = DeviceArray.zeros((nworld, n)), DeviceArray.zeros((nworld, n), np.int32), DeviceArray.zeros((nworld, n, 3))
  mjw.rays(m, d, P, V, geomgroup, flg_static, DeviceArray.full((n,), bodyexclude, np.int32), dist, gid, nrm)
  return dist.numpy().copy(), gid.numpy().copy(), nrm.numpy().copy()


def _check(got, want, label, min_hits):
  """Tolerances of tests/test_ray.py:161; flips <= 1 % of the rays, normals left out near edges <= 5 % of the hits."""
  (dist, gid, nrm), (wd, wg, wn, we) = got, want
  n = len(wd)
  flips = hits = left = 0
  for r in range(n):
    if wg[r] != gid[r]:
      flips += 1
      continue
    if wg[r] < 0:
      assert dist[r] == -1.0 and (nrm[r] == 0).all(), (label, r, dist[r], nrm[r])
      continue
    hits += 1
    assert abs(dist[r] - wd[r]) < 2e-5 * max(1.0, abs(wd[r])), (label, r, dist[r], wd[r], gid[r])
    if we[r] < 1e-4:
      left += 1
      continue
    assert np.abs(nrm[r] - wn[r]).max() < 2e-3, (label, r, nrm[r], wn[r], gid[r])
  print(f"{label}: rays {n}, hits {hits}, flips {flips}, normals left out {left}")
  assert flips <= 0.01 * n and left <= 0.05 * max(hits, 1) and hits >= min_hits, (label, flips, left, hits, n)
  return hits


def _want(mjm, q, w, pnt, vec, **kw):
  s = _sims(mjm, [q[w]])[0]
  p32, v32 = pnt.astype(np.float32).astype(np.float64), vec.astype(np.float32).astype(np.float64)  # (the rays the GPU was given)
  return bf.expected(bf.Caster(mjm, s), s, p32, v32, **kw)


@pytest.mark.gpu
def test_gpu_cube_mesh_equals_box_primitive():
  mjm, q, (pnt, vec) = _case_cube()
  box = mjw.mjcf.from_xml_string(CUBE_BOX)
  a, b = _gpu_rays(mjm, q, pnt, vec), _gpu_rays(box, q, pnt, vec)
  hits = flips = 0
  for w in range(3):
    for r in range(len(pnt)):
      if a[1][w, r] != b[1][w, r]:
        flips += 1
        continue
      if b[1][w, r] < 0:
        assert a[0][w, r] == -1.0 and (a[2][w, r] == 0).all()
        continue
      hits += 1
      assert abs(a[0][w, r] - b[0][w, r]) < 2e-5 * max(1.0, abs(b[0][w, r])) and np.abs(a[2][w, r] - b[2][w, r]).max() < 2e-3, (w, r, a[0][w, r], b[0][w, r], a[2][w, r], b[2][w, r])
  print(f"cube mesh vs box: hits {hits}, flips {flips}")
  assert flips <= 0.01 * 3 * len(pnt) and hits > 300 and (a[1] == 1).sum() > 100
  for w in range(3):  # ... and the brute force agrees
    _check((a[0][w], a[1][w], a[2][w]), _want(mjm, q, w, pnt, vec), f"cube world {w}", 50)


@pytest.mark.gpu
def test_gpu_mixed_scene_vs_bruteforce():
  mjm, q, (pnt, vec) = _case_mixed()
  names = list(mjm.geom_names)
  seen = set()
  for kw in FILTERS:
    got = _gpu_rays(mjm, q, pnt, vec, **kw)
    for w in range(len(q)):
      _check((got[0][w], got[1][w], got[2][w]), _want(mjm, q, w, pnt, vec, **kw), f"mixed {kw} world {w}", 10)
      seen |= set(int(g) for g in got[1][w])
    hit = set(names[g] for g in np.unique(got[1]) if g >= 0)
    assert not hit & {"ghost_mesh", "ghost_hills"}, hit  # alpha 0 on the geom / on its material
    if "geomgroup" in kw:
      assert not hit & {"masked_mesh", "hills"}, hit  # group 1 is masked
    if kw.get("bodyexclude") == 1:
      assert not hit & {"ball", "rider"}, hit
    if kw.get("flg_static") is False:
      assert hit <= {"ball", "rider"}, hit
  assert {names.index(n) for n in ("plane", "sphere", "capsule", "box", "octa", "ell", "hills", "masked_mesh", "rider")} <= seen
  # through the concavity of the L (its hull would be hit): straight down at the notch, in the L's frame (0.6, 0.6); the L's top is at z = 0.4 there
  g = names.index("ell")
  # (world frame, from the geom's own placement pos="-2 -1.2 0.8" euler="0 0 25")
  c, sn = np.cos(np.radians(25)), np.sin(np.radians(25))
  notch = np.array([-2.0, -1.2, 0.8]) + np.array([c * 0.6 - sn * 0.6, sn * 0.6 + c * 0.6, 0.0])
  arm = np.array([-2.0, -1.2, 0.8]) + np.array([c * 0.6 - sn * 0.15, sn * 0.6 + c * 0.15, 0.0])
  P2 = np.array([notch + [0, 0, 2.0], arm + [0, 0, 2.0]])
  V2 = np.array([[0, 0, -1.0], [0, 0, -1.0]])
  d2, g2, n2 = _gpu_rays(mjm, q[:1], P2, V2)
  assert g2[0, 0] == names.index("plane") and abs(d2[0, 0] - 2.8) < 1e-4, (d2, g2)  # past the L, down to the floor
  assert g2[0, 1] == g and abs(d2[0, 1] - 1.6) < 1e-4 and np.abs(n2[0, 1] - [0, 0, 1]).max() < 2e-3, (d2, g2, n2)  # the arm's top face


@pytest.mark.gpu
def test_gpu_hfield_vs_bruteforce():
  mjm, q, (pnt, vec) = _case_hfield()
  got = _gpu_rays(mjm, q, pnt, vec)
  want = _want(mjm, q, 0, pnt, vec)
  _check((got[0][0], got[1][0], got[2][0]), want, "hfield", 800)
  # every part of the solid was hit: grid (tilted normals), the four walls, the base's underside
  s = _sims(mjm, [q[0]])[0]
  local = got[2][0][got[1][0] == 0] @ s.geom_xmat[0].reshape(3, 3)
  for axis in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1]):
    assert (np.abs(local - axis).max(axis=1) < 1e-3).sum() >= 5, axis
  assert ((local[:, 2] > 0.3) & (local[:, 2] < 0.999)).sum() > 300


@pytest.mark.gpu
def test_gpu_aloha_pot_vs_bruteforce():
  """aloha_pot as loaded, at the pose of tests/test_aloha_pot.py (key lift_pot0, the arms' joints moved per world): a fan of 256 rays from above the
  table against every visible mesh of groups 0, 1 and 3 -- the model's visual shells (group 2) have no triangles, see ALOHA_KW."""
  mjm, q, (pnt, vec) = _aloha()
  m = mjw.put_model(mjm)
  assert m._ray_unsupported_geoms == 26 and m._ray_unsupported_groups == [2]
  with pytest.raises(NotImplementedError):  # (nothing silent: without the mask the call is refused)
    _gpu_rays(mjm, q, pnt, vec)
  got = _gpu_rays(mjm, q, pnt, vec, **ALOHA_KW)
  meshes = 0
  for w in range(4):
    _check((got[0][w], got[1][w], got[2][w]), _want(mjm, q, w, pnt, vec, **ALOHA_KW), f"aloha_pot world {w}", 100)
    meshes += int((np.asarray(mjm.geom_type)[got[1][w][got[1][w] >= 0]] == bf.MESH).sum())
  assert meshes > 100 and (got[1][0] != got[1][1]).any()  # (not vacuous: mesh geoms were hit; the worlds differ)


@pytest.mark.gpu
def test_gpu_rangefinder_over_mesh_and_hfield():
  mjm = mjw.mjcf.from_xml_string(RANGE)
  m = mjw.put_model(mjm)  # (accepted: it raised NotImplementedError before)
  d = mjw.make_data(mjm, nworld=2)
  q = d.qpos.numpy()
  q[1, :3] += [-0.7, -0.3, 0.1]  # (world 0 hovers over the L, world 1 over open terrain)
  d.qpos.assign(q)
  body = int(mjm.site_bodyid[0])
  seen, skipped = set(), 0
  for step in range(30):
    mjw.forward(m, d)
    sd = d.sensordata.numpy().copy()
    xp, xm = d.site_xpos.numpy(), d.site_xmat.numpy().reshape(2, mjm.nsite, 3, 3)
    P = DeviceArray.from_numpy(np.ascontiguousarray(xp[:, :2].astype(np.float32)))
    V = DeviceArray.from_numpy(np.ascontiguousarray(xm[:, :2, :, 2].astype(np.float32)))
    dist, gid = DeviceArray.zeros((2, 2)), DeviceArray.zeros((2, 2), np.int32)
    mjw.rays(m, d, P, V, None, True, DeviceArray.full((2,), body, np.int32), dist, gid, None)
    rd = dist.numpy()
    assert (np.abs(sd - rd) <= np.spacing(np.maximum(np.abs(sd), np.abs(rd)).astype(np.float32))).all(), (step, sd, rd)  # same device functions: 1 ulp
    for w in range(2):
      s = ref.RefSim(mjm, nconmax=16, njmax=64)
      s.qpos[:] = d.qpos.numpy()[w]
      s.forward()
      wd, wg, _, _ = bf.expected(bf.Caster(mjm, s), s, xp[w, :2].astype(np.float64), xm[w, :2, :, 2].astype(np.float64), bodyexclude=body)
      for k in range(2):
        if wg[k] == gid.numpy()[w, k]:
          assert abs(sd[w, k] - wd[k]) < 1e-4, (step, w, k, sd[w, k], wd[k])
          seen.add(int(wg[k]))
        else:
          skipped += 1  # (a grazing ray: another geom in float32 than in float64)
    mjw.step(m, d)
  assert skipped <= 0.01 * 120, skipped  # (30 steps x 2 worlds x 2 sensors; the same cap as for rays())
  assert {0, 1} <= seen and d.qpos.numpy()[0, 2] < 1.6  # the height field and the mesh were both ranged; the drone fell


@pytest.mark.gpu
def test_gpu_determinism_and_shape_independence():
  mjm, q, (pnt, vec) = _case_mixed()
  a = _gpu_rays(mjm, q[:1], pnt, vec)
  b = _gpu_rays(mjm, q[:1], pnt, vec)
  for x, y in zip(a, b):
    assert x.tobytes() == y.tobytes()
  big = _gpu_rays(mjm, q[:1], pnt, vec, nworld=64)  # broadcast pnt (pnt.shape[0] == 1), 64 identical worlds
  own = _gpu_rays(mjm, q[:1], pnt, vec, nworld=64, broadcast=False)
  for x, y, z in zip(a, big, own):
    for w in range(64):
      assert x[0].tobytes() == y[w].tobytes() == z[w].tobytes(), w


@pytest.mark.gpu
def test_gpu_primitive_models_bitwise_unchanged():
  """Primitive-only models keep the one-thread-per-ray kernel: rays() on the scene of tests/test_ray.py is bit for bit what the commit before
  this feature computed.  tests/golden/ray_primitive_parent.npz was made on an MI355X from a checkout of that commit, built as it was, onto which
  tools/dump_ray_primitive.py (which that commit did not have; it uses only the public API and the scene of tests/test_ray.py) was copied, with

    python tools/dump_ray_primitive.py tests/golden/ray_primitive_parent.npz
  """
  import importlib.util

  spec = importlib.util.spec_from_file_location("dump_ray_primitive", os.path.join(conftest.ROOT, "tools", "dump_ray_primitive.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  want = np.load(os.path.join(conftest.GOLDEN_DIR, "ray_primitive_parent.npz"))
  got = mod.outputs()
  assert sorted(got) == sorted(want.files)
  for k in want.files:
    assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
