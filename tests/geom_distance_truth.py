"""Scenes, poses and expected values of the geom distance sensors (tests/test_geom_distance.py).

The expected signed distance of a geom pair comes from tests/geom_truth.py alone (closed forms and one-dimensional searches on the shapes,
NumPy float64); pair classes without a closed form (cylinder-box, ellipsoid-box, box-mesh) use the float64 GJK / EPA of the oracle.  The
float32 twin of that GJK / EPA (`ref._F32`) measures, on the same poses, the error a float32 implementation of the algorithm has against
the same expected value: the floor the kernel's bound is built from.

  python tests/geom_distance_truth.py        prints the floor table of test_geom_distance.py (CPU only)
"""

import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import geom_truth as gt  # noqa: E402

NWORLD = 32
GEOM_TYPE = {"plane": 0, "sphere": 2, "capsule": 3, "ellipsoid": 4, "cylinder": 5, "box": 6, "mesh": 7}
# the 8-vertex inline mesh: a skewed hexahedron (no two faces parallel to a coordinate plane pair, so it is not mistaken for a box)
MESH_VERT = np.array([[-.10, -.08, -.06], [.12, -.07, -.05], [.11, .09, -.07], [-.09, .10, -.06], [-.07, -.06, .08], [.08, -.05, .07], [.07, .06, .09], [-.06, .07, .08]])
SIZES = {"sphere": [0.11], "capsule": [0.06, 0.14], "ellipsoid": [0.09, 0.13, 0.07], "cylinder": [0.08, 0.12], "box": [0.10, 0.07, 0.12], "mesh": [], "plane": [1, 1, 0.1]}
# (class name, kind of side 1, kind of side 2, penetrating poses have a truth)
CLASSES = [
  ("sphere_sphere", "sphere", "sphere", True), ("sphere_capsule", "sphere", "capsule", True), ("capsule_capsule", "capsule", "capsule", True),
  ("sphere_box", "sphere", "box", True), ("capsule_box", "capsule", "box", True), ("box_box", "box", "box", True),
  ("sphere_cylinder", "sphere", "cylinder", True), ("capsule_cylinder", "capsule", "cylinder", True), ("cylinder_box", "cylinder", "box", False),
  ("ellipsoid_box", "ellipsoid", "box", False), ("box_mesh", "box", "mesh", False),
  ("plane_sphere", "plane", "sphere", True), ("plane_capsule", "plane", "capsule", True), ("plane_box", "plane", "box", True), ("plane_cylinder", "plane", "cylinder", True),
]
ORACLE_CLASSES = ("cylinder_box", "ellipsoid_box", "box_mesh")
PLANE_QUAT = np.array([0.9914449, 0.0922959, -0.0922959, 0.0], dtype=np.float32)  # a tilted floor
PLANE_POS = np.array([0.1, -0.2, 0.05], dtype=np.float32)


def quat_to_mat32(q):
  """Rotation of a quaternion, every operation in float32 (the pose a float32 engine derives from a float32 qpos, up to rounding)."""
  q = np.asarray(q, dtype=np.float32)
  q = q / np.sqrt(np.sum(q * q, dtype=np.float32))
  w, x, y, z = q
  two = np.float32(2)
  return np.array([[w * w + x * x - y * y - z * z, two * (x * y - w * z), two * (x * z + w * y)],
                   [two * (x * y + w * z), w * w - x * x + y * y - z * z, two * (y * z - w * x)],
                   [two * (x * z - w * y), two * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=np.float32)


def shape(kind, pos, mat, size=None, vert=None):
  return gt.Shape(kind, pos, mat, SIZES[kind] if size is None else size, vert if kind == "mesh" else None)


_FMT = lambda v: " ".join(f"{float(x):.9g}" for x in np.asarray(v).reshape(-1))


def geom_xml(name, kind, size=None, attrs=""):
  size = SIZES[kind] if size is None else size
  return f'<geom name="{name}" type="{kind}" {"mesh=" + chr(34) + "hexa" + chr(34) if kind == "mesh" else "size=" + chr(34) + _FMT(size) + chr(34)} {attrs}/>'


def scene_xml(name, sensors=None, cutoff=10.0, option=""):
  """The scene of class `name`: geom g1 (a plane: fixed in the world; else on free body b1) and g2 on free body b2; by default the three
  sensors in both orders: d12 n12 f12 d21 n21 f21."""
  _, k1, k2, _ = next(c for c in CLASSES if c[0] == name)
  if sensors is None:
    sensors = "".join(f'<{tag} name="{tag[0]}{a}{b}" geom1="g{a}" geom2="g{b}" cutoff="{cutoff}"/>' for a, b in ((1, 2), (2, 1)) for tag in ("distance", "normal", "fromto"))
  first = geom_xml("g1", k1, attrs=f'pos="{_FMT(PLANE_POS)}" quat="{_FMT(PLANE_QUAT)}"') if k1 == "plane" else f'<body name="b1"><freejoint/>{geom_xml("g1", k1)}</body>'
  asset = f'<asset><mesh name="hexa" vertex="{_FMT(MESH_VERT)}"/></asset>' if "mesh" in (k1, k2) else ""
  return f"""<mujoco>{option}{asset}<worldbody>{first}<body name="b2"><freejoint/>{geom_xml("g2", k2)}</body></worldbody><sensor>{sensors}</sensor></mujoco>"""


def model(name, **kw):
  import mujoco_warp_amd as mjw

  return mjw.mjcf.from_xml_string(scene_xml(name, **kw))


def mesh_vert(mjm, g):
  """Vertices of mesh geom g in its geom frame, as the model holds them (the loader re-centres a mesh asset); None for other geoms."""
  if int(mjm.geom_type[g]) != GEOM_TYPE["mesh"]:
    return None
  k = int(mjm.geom_dataid[g])
  return np.asarray(mjm.mesh_vert, dtype=np.float64).reshape(-1, 3)[int(mjm.mesh_vertadr[k]) : int(mjm.mesh_vertadr[k]) + int(mjm.mesh_vertnum[k])]


def _quat_mul32(a, b):
  a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
  return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                   a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=np.float32)


def geom_poses32(mjm, q):
  """(pos [ngeom, 3], mat [ngeom, 3, 3]) float32 of the model's geoms at qpos row q (free bodies in order, geoms of the world fixed): the
  float32 composition body pose x geom frame, standing in for a float32 engine's kinematics where no GPU is at hand."""
  pos, mat = [], []
  for g in range(mjm.ngeom):
    b = int(mjm.geom_bodyid[g])
    gp, gq = np.asarray(mjm.geom_pos[g], dtype=np.float32), np.asarray(mjm.geom_quat[g], dtype=np.float32)
    if b == 0:
      pos.append(gp)
      mat.append(quat_to_mat32(gq))
    else:
      a = int(mjm.jnt_qposadr[int(mjm.body_jntadr[b])])
      pb, qb = np.asarray(q[a : a + 3], dtype=np.float32), np.asarray(q[a + 3 : a + 7], dtype=np.float32)
      pos.append(pb + quat_to_mat32(qb) @ gp)
      mat.append(quat_to_mat32(_quat_mul32(qb / np.sqrt(np.sum(qb * qb, dtype=np.float32)), gq)))
  return np.array(pos, dtype=np.float32), np.array(mat, dtype=np.float32)


def _radius(kind):
  s = SIZES[kind]
  return {"sphere": lambda: s[0], "capsule": lambda: s[0] + s[1], "ellipsoid": lambda: max(s), "cylinder": lambda: np.hypot(s[0], s[1]), "box": lambda: np.linalg.norm(s),
          "mesh": lambda: np.linalg.norm(MESH_VERT, axis=1).max()}[kind]()


def _inradius(kind):
  s = SIZES[kind]
  return {"sphere": lambda: s[0], "capsule": lambda: s[0], "ellipsoid": lambda: min(s), "cylinder": lambda: min(s), "box": lambda: min(s), "mesh": lambda: 0.05}[kind]()


def expected(name, s1, s2):
  """Signed distance of the two shapes of class `name` from the geometry alone; None where the pose is outside what the closed forms cover
  (a capsule whose axis segment enters the other shape: the minimum over the segment is then no longer the penetration depth)."""
  k1, k2 = s1.kind, s2.kind
  if k1 == "plane":
    return gt.plane_distance(s1, s2)
  if k1 == "sphere":
    return float(gt.sdf(s2, s1.pos)) - s1.size[0]
  if k1 == "capsule":
    p, q = s1.pos - s1.axis * s1.size[1], s1.pos + s1.axis * s1.size[1]
    if k2 == "capsule":
      d = gt.segment_segment_distance(p, q, s2.pos - s2.axis * s2.size[1], s2.pos + s2.axis * s2.size[1])
      return d - s1.size[0] - s2.size[0] if d > 1e-3 else None
    d = gt.segment_shape_distance(p, q, s2)[0]
    return d - s1.size[0] if d > 1e-3 else None
  if k1 == "box" and k2 == "box":
    depth = gt.box_box_sat_depth(s1, s2)[0]
    return -depth if depth > 0 else gt.box_box_distance(s1, s2)
  return None


def poses(name, nworld=NWORLD):
  """qpos [nworld, 7 or 14] float32 of class `name`: random orientations, the second body in a random direction at a centre distance drawn
  between touching deeply and clearly apart.  A plane is side 1 and fixed in the world (its class has one free body)."""
  _, k1, k2, _ = next(c for c in CLASSES if c[0] == name)
  rng = np.random.default_rng(sum(map(ord, name)))
  out = []
  for w in range(nworld):
    q1, q2 = (rng.normal(size=4).astype(np.float32) for _ in range(2))
    q1, q2 = (q / np.linalg.norm(q).astype(np.float32) for q in (q1, q2))
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    if k1 == "plane":
      p1, q1 = PLANE_POS, PLANE_QUAT
      n = quat_to_mat32(q1).astype(np.float64)[:, 2]
      lateral = u - n * (u @ n)
      p2 = (p1 + 0.3 * lateral + n * rng.uniform(-0.3 * _inradius(k2), _radius(k2) + 0.25)).astype(np.float32)
    else:
      p1 = rng.uniform(-0.2, 0.2, size=3).astype(np.float32)
      lo, hi = max(_radius(k1), _radius(k2)) * 0.75, _radius(k1) + _radius(k2) + 0.2
      p2 = (p1 + u * rng.uniform(lo, hi)).astype(np.float32)
    out.append(np.concatenate([p2, q2] if k1 == "plane" else [p1, q1, p2, q2]).astype(np.float32))
  return np.array(out, dtype=np.float32)


def oracle(real, k1, p1, m1, k2, p2, m2, tolerance=1e-6, iterations=35, size1=None, size2=None, vert1=None, vert2=None):
  """(dist, x1, x2) of the oracle's GJK / EPA in one precision (`ref._F64` / `ref._F32`), geoms passed in collider order (lower type first)
  and the result handed back in the caller's order; margin 0, no cutoff."""
  from oracle import ref

  R = {"f64": ref._F64, "f32": ref._F32}[real]
  a = [GEOM_TYPE[k1], p1, m1, SIZES[k1] if size1 is None else size1, vert1 if k1 == "mesh" else None]
  b = [GEOM_TYPE[k2], p2, m2, SIZES[k2] if size2 is None else size2, vert2 if k2 == "mesh" else None]
  swap = a[0] > b[0]
  if swap:
    a, b = b, a
  arr = lambda x, n: R.arr(np.resize(np.asarray(x, dtype=np.float64).reshape(-1), n) if np.size(x) else np.zeros(n))
  size = lambda s: R.arr((list(np.asarray(s, dtype=np.float64).reshape(-1)) + [0, 0, 0])[:3])
  args = []
  keep = []
  for t, p, mt, s, v in (a, b):
    vv = R.arr(v) if v is not None else None
    keep += [arr(p, 3), arr(mt, 9), size(s), vv]
    args += [int(t), R.ptr(keep[-4]), R.ptr(keep[-3]), R.ptr(keep[-2]), R.ptr(vv) if vv is not None else None, 0 if vv is None else len(vv)]
  out, wit = R.arr(np.zeros(9)), R.arr(np.zeros(48))
  fn = R.lib().ref_ccd_mesh
  fn.restype = ctypes.c_int
  fn.argtypes = None
  fn(*args, R.c_real(0.0), R.c_real(tolerance), R.c_real(1e30), int(iterations), 0, R.ptr(out), R.ptr(wit))
  x1, x2 = out[1:4].astype(np.float64), out[4:7].astype(np.float64)
  return float(out[0]), (x2 if swap else x1), (x1 if swap else x2)


def plane_closed_form32(plane_pos, plane_mat, k2, p2, m2):
  """The plane pairs' closed form -- height of the lowest point of the shape over the plane -- evaluated in NumPy float32."""
  f = np.float32
  n = np.asarray(plane_mat, dtype=f)[:, 2]
  s, m2, p2 = np.asarray(SIZES[k2], dtype=f), np.asarray(m2, dtype=f), np.asarray(p2, dtype=f)
  l = -(m2.T @ n)  # the direction -n in the shape's frame
  sg = np.where(l >= 0, f(1), f(-1))
  if k2 == "sphere":
    loc = l * s[0]
  elif k2 == "capsule":
    loc = l * s[0] + np.array([0, 0, sg[2] * s[1]], dtype=f)
  elif k2 == "box":
    loc = sg * s[:3]
  else:  # cylinder
    rn = np.sqrt(l[0] * l[0] + l[1] * l[1])
    rad = np.array([l[0], l[1]], dtype=f) * (s[0] / rn) if rn > 0 else np.zeros(2, dtype=f)
    loc = np.array([rad[0], rad[1], sg[2] * s[1]], dtype=f)
  x = m2 @ loc + p2
  return float(n @ (x - np.asarray(plane_pos, dtype=f)))


def class_truth(name, mjm, xpos, xmat):
  """(expected signed distance or None, shape 1, shape 2) of class `name` with the model's geoms g1, g2 (ids 0, 1) at the given poses."""
  _, k1, k2, _ = next(c for c in CLASSES if c[0] == name)
  p1, m1, p2, m2 = (np.asarray(x, dtype=np.float64) for x in (xpos[0], np.reshape(xmat[0], (3, 3)), xpos[1], np.reshape(xmat[1], (3, 3))))
  v1, v2 = mesh_vert(mjm, 0), mesh_vert(mjm, 1)
  s1, s2 = shape(k1, p1, m1, vert=v1), shape(k2, p2, m2, vert=v2)
  if name in ORACLE_CLASSES:
    return oracle("f64", k1, p1, m1, k2, p2, m2, vert1=v1, vert2=v2)[0], s1, s2
  return expected(name, s1, s2), s1, s2


def floor(name):
  """Largest error of the float32 twin (plane pairs: of the float32 closed form) against the expected value over the poses of `name`."""
  _, k1, k2, _ = next(c for c in CLASSES if c[0] == name)
  mjm, worst, count = model(name), 0.0, [0, 0, 0]
  for q in poses(name):
    xpos, xmat = geom_poses32(mjm, q)
    want, _, _ = class_truth(name, mjm, xpos, xmat)
    count[2 if want is None else int(want < 0)] += 1
    if want is None:
      continue
    got = (plane_closed_form32(xpos[0], xmat[0], k2, xpos[1], xmat[1]) if k1 == "plane" else
           oracle("f32", k1, xpos[0], xmat[0], k2, xpos[1], xmat[1], tolerance=float(mjm.opt.ccd_tolerance), iterations=int(mjm.opt.ccd_iterations), vert1=mesh_vert(mjm, 0), vert2=mesh_vert(mjm, 1))[0])
    worst = max(worst, abs(got - want))
  return worst, count


if __name__ == "__main__":
  for c in CLASSES:
    worst, (nsep, npen, nnone) = floor(c[0])
    print(f'  "{c[0]}": {worst:.1e},  # {nsep} separated, {npen} penetrating, {nnone} outside the closed forms')
