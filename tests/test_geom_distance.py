"""Geom distance sensors (<distance> / <normal> / <fromto>, mjSENS_GEOMDIST / GEOMNORMAL / GEOMFROMTO = 39 / 40 / 41;
csrc/sensor_collision.hpp) and <insidesite> (38, csrc/sensor.hpp).

CPU: the loader's tables and refusals, put_model's tables, and the expected values of tests/geom_distance_truth.py pinned on hand-computed
poses.  GPU: every world's sensordata against the geometry (tests/geom_truth.py) at the engine's own geom poses.

Bound of a pair class: max(4 x FLOOR, 2e-7), the rule of tests/test_colliders.py: FLOOR is the largest error, against the same expected
value on the same sweep of poses, of the float32 twin of the oracle's GJK / EPA (plane pairs: of the closed form in NumPy float32),
measured on the CPU; nothing is derived from the kernel's output.

The kernel runs `ccd_gjk_phase` in its GUARD instantiation (csrc/convex.hpp `ccd_gjk`).  Without it two classes missed their bound on the
MI355X -- capsule_cylinder 4.5e-6 against 2.56e-6, ellipsoid_box 2.1e-4 against 1.24e-5, and cylinder_box came to 6.3e-4 -- always on SEPARATED
pairs with a curved shape that is no sphere or capsule, always with a distance SMALLER than the true one.  The cause, found on the CPU with
the engine's own `ccd_gjk_phase` compiled for the host and run on the engine's recorded geom poses: in float32 the sub-distance solve of a
three-vertex simplex whose support points lie close together on a curved rim, nearly collinear, loses its digits; its "closest point" lands
outside the Minkowski difference, below the lower bound the loop has already proven (the duality gap turns negative and the loop ends on
it), or two simplices alternate with a rising |x_k| until the iterations run out.  The float64 oracle is exact on the same poses and stops
long before the iteration cap; more iterations change nothing in float32.  The guard refuses a closest point below the proven lower bound
and returns the smallest sound |x_k| with its witness points.  The step's narrowphase keeps the unguarded instantiation (its device code is
unchanged): a contact survives such an error, a sensor reading is used as a number.

Measured on the MI355X with the guard (worst distance error per class over the 32 worlds, beside its bound): sphere_sphere 5.7e-8 / 2.1e-7,
sphere_capsule 9.6e-8 / 3.6e-7, capsule_capsule 5.3e-8 / 2e-7, sphere_box 1.2e-7 / 3.4e-7, capsule_box 1.5e-7 / 4.4e-7, box_box 8.2e-8 /
2.8e-7, sphere_cylinder 1.3e-7 / 2.3e-7, capsule_cylinder 6.5e-7 / 2.56e-6, cylinder_box 1.0e-6 / 8.8e-4, ellipsoid_box 2.6e-7 / 1.24e-5
(witness 6.4e-7), box_mesh 2.5e-8 / 2e-7, the four plane classes 2.1e-8 .. 3.9e-8 / 2e-7.  The floors of the curved classes are what the
UNGUARDED float32 twin gives (its own tail: cylinder_box 2.2e-4 in one world, ~1e-8 in most); they stay as the rule measures them.
"""

import functools

import numpy as np
import pytest

import conftest
import geom_distance_truth as T
import geom_truth as gt

import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi, io

NW = T.NWORLD
# python tests/geom_distance_truth.py   (CPU; the float32 twin `ref._F32.lib().ref_ccd_mesh` with the model's ccd_tolerance 1e-6 and 35 iterations)
FLOOR = {
  "sphere_sphere": 5.3e-08,  # 15 separated, 17 penetrating, 0 outside the closed forms
  "sphere_capsule": 8.9e-08,  # 29 separated, 3 penetrating, 0 outside the closed forms
  "capsule_capsule": 4.8e-08,  # 28 separated, 4 penetrating, 0 outside the closed forms
  "sphere_box": 8.5e-08,  # 25 separated, 7 penetrating, 0 outside the closed forms
  "capsule_box": 1.1e-07,  # 27 separated, 2 penetrating, 3 outside the closed forms
  "box_box": 7.1e-08,  # 20 separated, 12 penetrating, 0 outside the closed forms
  "sphere_cylinder": 5.8e-08,  # 23 separated, 9 penetrating, 0 outside the closed forms
  "capsule_cylinder": 6.4e-07,  # 30 separated, 2 penetrating, 0 outside the closed forms
  "cylinder_box": 2.2e-04,  # 22 separated, 10 penetrating, 0 outside the closed forms  (against the float64 oracle: EPA on a curved shape)
  "ellipsoid_box": 3.1e-06,  # 21 separated, 11 penetrating, 0 outside the closed forms  (against the float64 oracle)
  "box_mesh": 3.1e-08,  # 23 separated, 9 penetrating, 0 outside the closed forms  (against the float64 oracle)
  "plane_sphere": 4.2e-08,  # 18 separated, 14 penetrating, 0 outside the closed forms
  "plane_capsule": 3.3e-08,  # 24 separated, 8 penetrating, 0 outside the closed forms
  "plane_box": 3.9e-08,  # 18 separated, 14 penetrating, 0 outside the closed forms
  "plane_cylinder": 3.7e-08,  # 22 separated, 10 penetrating, 0 outside the closed forms
}
NAMES = [c[0] for c in T.CLASSES]


def bound(name):
  return max(4.0 * FLOOR[name], 2e-7)


def _bits(x):
  return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _rot(axis, angle):
  axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
  K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
  return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


# ---- loader ---------------------------------------------------------------------------------------------------------------------------
_WORLD = """
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1"/>
    <site name="zone" type="box" size=".1 .1 .1"/>
    <body name="a" pos="0 0 .5"><freejoint/><geom name="ga" type="sphere" size=".1"/></body>
    <body name="b" pos="1 0 .5"><freejoint/><geom name="gb" type="box" size=".1 .1 .1"/></body>
    <body name="c" pos="2 0 .5"><freejoint/><geom name="c0" type="sphere" size=".1"/><geom name="c1" type="capsule" size=".05 .1" pos=".3 0 0"/>
      <geom name="c2" type="box" size=".05 .05 .05" pos="0 .3 0"/></body>
    <body name="nogeom" pos="3 0 .5"><freejoint/><inertial pos="0 0 0" mass="1" diaginertia="1 1 1"/></body>
  </worldbody>
"""


def _load(sensors, world=_WORLD, extra=""):
  return mjw.mjcf.from_xml_string(f"<mujoco>{extra}{world}<sensor>{sensors}</sensor></mujoco>")


# geoms: floor 0, ga 1, gb 2, c0 3, c1 4, c2 5; bodies: world 0, a 1, b 2, c 3, nogeom 4
_SIDES = [('geom1="ga" geom2="gb"', (5, 1, 5, 2)), ('geom1="ga" body2="b"', (5, 1, 1, 2)), ('body1="a" geom2="gb"', (1, 1, 5, 2)), ('body1="a" body2="b"', (1, 1, 1, 2)),
          ('body1="c" geom2="floor"', (1, 3, 5, 0)), ('body1="c" body2="nogeom"', (1, 3, 1, 4))]


def test_loader_tables():
  tags = (("distance", 39, 1, 0), ("normal", 40, 3, 2), ("fromto", 41, 6, 0))
  xml = "".join(f'<{tag} {attrs} cutoff="{0.5 * (i + 1)}"/>' for attrs, _ in _SIDES for i, (tag, _, _, _) in enumerate(tags))
  mjm = _load(xml + '<insidesite site="zone" objtype="xbody" objname="a"/><clock/>')
  n = 3 * len(_SIDES)
  assert mjm.nsensor == n + 2
  for k, (attrs, ids) in enumerate(_SIDES):
    for i, (tag, num, dim, datatype) in enumerate(tags):
      s = 3 * k + i
      got = (int(mjm.sensor_objtype[s]), int(mjm.sensor_objid[s]), int(mjm.sensor_reftype[s]), int(mjm.sensor_refid[s]))
      assert got == ids, (attrs, got)
      assert (int(mjm.sensor_type[s]), int(mjm.sensor_dim[s]), int(mjm.sensor_datatype[s]), int(mjm.sensor_needstage[s])) == (num, dim, datatype, 1)
      assert mjm.sensor_cutoff[s] == 0.5 * (i + 1)
  assert (int(mjm.sensor_type[n]), int(mjm.sensor_objtype[n]), int(mjm.sensor_objid[n]), int(mjm.sensor_reftype[n]), int(mjm.sensor_refid[n])) == (38, 2, 1, 6, 0)
  assert (int(mjm.sensor_dim[n]), int(mjm.sensor_datatype[n]), int(mjm.sensor_needstage[n])) == (1, 0, 1)
  assert (mjm.sensor_adr == np.concatenate([[0], np.cumsum(mjm.sensor_dim)[:-1]])).all() and mjm.nsensordata == 10 * len(_SIDES) + 2
  assert mjm.body_geomnum.tolist() == [1, 1, 1, 3, 0] and mjm.body_geomadr.tolist()[:4] == [0, 1, 2, 3]
  assert {k: mjw.mjcf.SENS[k] for k in ("insidesite", "distance", "normal", "fromto")} == {"insidesite": 38, "distance": 39, "normal": 40, "fromto": 41}
  assert (mjw.SensorType.INSIDESITE, mjw.SensorType.GEOMDIST, mjw.SensorType.GEOMNORMAL, mjw.SensorType.GEOMFROMTO, mjw.SensorType.CONTACT) == (38, 39, 40, 41, 42)
  assert _load('<distance geom1="ga" geom2="gb" cutoff="0"/>').sensor_cutoff[0] == 0.0  # (legal)
  for objtype, name, want in (("body", "a", 1), ("xbody", "b", 2), ("geom", "c1", 5), ("site", "zone", 6)):
    mjm = _load(f'<insidesite site="zone" objtype="{objtype}" objname="{name}"/>')
    assert int(mjm.sensor_objtype[0]) == want and int(mjm.sensor_type[0]) == 38


@pytest.mark.parametrize("tag", ["distance", "normal", "fromto"])
@pytest.mark.parametrize("attrs", [
  'geom1="ga" body1="a" geom2="gb"',  # two first objects
  'geom1="ga" geom2="gb" body2="b"',  # two second objects
  'geom2="gb"', 'geom1="ga"', '',  # none
  'geom1="nope" geom2="gb"', 'geom1="ga" body2="nope"',  # unknown names
  'geom1="ga" geom2="ga"', 'body1="a" body2="a"',  # the same object twice
  'geom1="ga" geom2="gb" cutoff="-1"',
])
def test_loader_refuses(tag, attrs):
  with pytest.raises(ValueError):
    _load(f"<{tag} {attrs}/>")


def test_loader_refuses_insidesite():
  with pytest.raises(NotImplementedError, match="camera"):
    _load('<insidesite site="zone" objtype="camera" objname="cam"/>')
  with pytest.raises(ValueError):
    _load('<insidesite site="nope" objtype="body" objname="a"/>')
  massless = """<worldbody><site name="zone" type="box" size=".1 .1 .1"/>
    <body name="parent"><freejoint/><body name="child" pos="0 0 .1"><geom type="sphere" size=".1"/></body></body></worldbody>"""
  with pytest.raises(NotImplementedError, match="massless"):
    _load('<insidesite site="zone" objtype="body" objname="parent"/>', world=massless)
  assert _load('<insidesite site="zone" objtype="xbody" objname="parent"/>', world=massless).nsensor == 1


def test_put_model_tables(humanoid):
  fields = [f[0] for f in _abi.MODEL_FIELDS]
  k = fields.index("sensor_cutoff")
  assert fields[k + 1 : k + 5] == ["nsensor_collision", "sensor_collision_adr", "body_geomnum", "body_geomadr"]
  assert _abi.DEFINES["MJH_ABI_VERSION"] == 45
  assert "sensor_collision_tu.hip" in _abi.UNITS and "sensor_collision.hpp" in _abi.HEADERS
  assert io._MODEL_ARRAYS["sensor_collision_adr"] == (("nsensor",), "int32", False) and io._MODEL_ARRAYS["body_geomnum"] == (("nbody",), "int32", False)
  m = mjw.put_model(humanoid)
  assert m.nsensor_collision == 0 and io.c_model(m).nsensor_collision == 0 and m.sensor_collision_adr.shape == (m.nsensor,)
  assert m.body_geomnum.numpy().tolist() == np.asarray(humanoid.body_geomnum).tolist()
  mjm = _load('<framepos objtype="body" objname="a"/><distance geom1="ga" geom2="gb"/><clock/><fromto body1="c" body2="b"/>')
  m = mjw.put_model(mjm)
  assert m.nsensor_collision == 2 and m.sensor_collision_adr.numpy().tolist() == [1, 3, -1, -1] and m.nsensor_acc == 0
  assert m.body_geomadr.numpy().tolist()[:4] == [0, 1, 2, 3] and m.body_geomnum.numpy().tolist() == [1, 1, 1, 3, 0]
  assert mjw.put_model(_load('<distance body1="c" body2="nogeom"/>')).nsensor_collision == 1  # (a side without geoms is legal)
  mjm.sensor_dim = mjm.sensor_dim.copy()
  mjm.sensor_dim[3] = 3
  with pytest.raises(ValueError, match="sensor_dim"):
    mjw.put_model(mjm)


def test_put_model_refuses():
  hfield = """<asset><hfield name="h" nrow="3" ncol="3" size="1 1 .2 .1" elevation="0 0 0 0 1 0 0 0 0"/>
    <mesh name="tet" vertex="0 0 0 .1 0 0 0 .1 0 0 0 .1"/></asset>"""
  world = """<worldbody><geom name="p1" type="plane" size="1 1 .1"/><geom name="p2" type="plane" size="1 1 .1" pos="0 0 -1"/>
    <geom name="hf" type="hfield" hfield="h" pos="3 0 0"/>
    <body name="a" pos="0 0 .5"><freejoint/><geom name="ga" type="sphere" size=".1"/></body>
    <body name="mb" pos="0 0 1.5"><freejoint/><geom name="gm" type="mesh" mesh="tet"/></body></worldbody>"""
  with pytest.raises(NotImplementedError, match="'dh'.*height"):  # (the message names the sensor)
    mjw.put_model(_load('<distance name="dh" geom1="ga" geom2="hf"/>', world=world, extra=hfield))
  world = world.replace('<geom name="hf" type="hfield" hfield="h" pos="3 0 0"/>', "")
  with pytest.raises(NotImplementedError, match="plane-plane"):
    mjw.put_model(_load('<distance geom1="p1" geom2="p2"/>', world=world, extra=hfield))
  with pytest.raises(NotImplementedError, match="plane-plane"):
    mjw.put_model(_load('<normal body1="world" geom2="p2"/>', world=world, extra=hfield))  # (the world body's geoms include a plane)
  assert mjw.put_model(_load('<distance geom1="p1" geom2="gm"/>', world=world, extra=hfield)).nsensor_collision == 1  # plane against a convex shape
  # (a colliding mesh geom without vertices is refused by the collision tables already; the sensor's own check catches one that does not collide)
  mjm = _load('<fromto geom1="ga" geom2="gm"/>', world=world.replace('type="mesh"', 'type="mesh" contype="0" conaffinity="0"'), extra=hfield)
  mjm.geom_dataid = np.full_like(mjm.geom_dataid, -1)  # (a mesh geom that points at no mesh asset: there are no vertices to search)
  with pytest.raises(NotImplementedError, match="no vertices"):
    mjw.put_model(mjm)


# ---- the expected values on hand-computed poses --------------------------------------------------------------------------------------------
def test_truth_hand_poses():
  I = np.eye(3)
  box = gt.Shape("box", [0, 0, 0], I, [0.1, 0.1, 0.1])
  # 3-4-5 from the box's edge at (0.1, 0.1, z)
  assert abs(T.expected("sphere_box", gt.Shape("sphere", [0.4, 0.5, 0.03], I, [0.05]), box) - 0.45) < 1e-15
  # a sphere of radius 0.2 whose surface reaches 0.1 past the face x = 0.1
  assert abs(T.expected("sphere_box", gt.Shape("sphere", [0.2, 0, 0], I, [0.2]), box) + 0.1) < 1e-15
  # sphere - sphere, centres 3-4-5 apart
  assert abs(T.expected("sphere_sphere", gt.Shape("sphere", [0, 0, 0], I, [0.1]), gt.Shape("sphere", [0.3, 0.4, 0], I, [0.15])) - 0.25) < 1e-15
  # capsules along z and along x (rotated about y), nearest axis points (0, 0, 0.2) and (0.3, 0.4, 0.2)... the second lies at y = 0.4, x >= 0.3
  c1 = gt.Shape("capsule", [0, 0, 0], I, [0.05, 0.2])
  c2 = gt.Shape("capsule", [0.8, 0.4, 0.2], _rot([0, 1, 0], np.pi / 2), [0.03, 0.5])
  assert abs(T.expected("capsule_capsule", c1, c2) - (0.5 - 0.08)) < 1e-12
  # capsule over a box corner region: axis parallel to z at (0.4, 0.5), spanning the box's height
  assert abs(T.expected("capsule_box", gt.Shape("capsule", [0.4, 0.5, 0], I, [0.05, 0.3]), box) - 0.45) < 1e-9
  # sphere beside a cylinder's rim: 3-4-5
  cyl = gt.Shape("cylinder", [0, 0, 0], I, [0.2, 0.5])
  assert abs(T.expected("sphere_cylinder", gt.Shape("sphere", [0.5, 0, 0.9], I, [0.1]), cyl) - 0.4) < 1e-15
  # boxes: separated along a face normal, and overlapping by 0.03 along x (SAT depth)
  assert abs(T.expected("box_box", box, gt.Shape("box", [0.5, 0.05, 0], I, [0.1, 0.2, 0.1])) - 0.3) < 1e-12
  assert abs(T.expected("box_box", box, gt.Shape("box", [0.17, 0.02, 0.01], I, [0.1, 0.1, 0.1])) + 0.03) < 1e-12
  # a plane tilted by 45 degrees about x through the origin: normal (0, -s, s); sphere at (0, 0, 1)
  plane = gt.Shape("plane", [0, 0, 0], _rot([1, 0, 0], np.pi / 4))
  assert abs(T.expected("plane_sphere", plane, gt.Shape("sphere", [0, 0, 1], I, [0.25])) - (np.sqrt(0.5) - 0.25)) < 1e-15
  assert abs(T.expected("plane_box", gt.Shape("plane", [0, 0, 0], I), gt.Shape("box", [0, 0, 0.05], I, [0.1, 0.2, 0.3])) + 0.25) < 1e-15
  # a capsule whose axis enters the box is outside what the closed forms cover
  assert T.expected("capsule_box", gt.Shape("capsule", [0, 0, 0], I, [0.05, 0.3]), box) is None
  # the float32 closed form of the plane pairs agrees with the float64 one
  q = T.poses("plane_cylinder")[3]
  mjm = T.model("plane_cylinder")
  xpos, xmat = T.geom_poses32(mjm, q)
  want, _, _ = T.class_truth("plane_cylinder", mjm, xpos, xmat)
  assert abs(T.plane_closed_form32(xpos[0], xmat[0], "cylinder", xpos[1], xmat[1]) - want) < 1e-6


def test_oracle_reproduces_the_truth():
  """The float64 GJK / EPA against the closed forms on the sweeps' own poses: separated pairs to 1e-12 (the capsule - cylinder sweep: 1e-6,
  GJK's stopping tolerance on two curved shapes), penetrating ones to EPA's stopping tolerance 1e-6."""
  for name in ("sphere_box", "capsule_capsule", "box_box", "sphere_cylinder"):
    mjm = T.model(name)
    _, k1, k2, _ = next(c for c in T.CLASSES if c[0] == name)
    for q in T.poses(name)[:12]:  # (float64 rotations of the same quaternions: exactly orthonormal, so that both sides see one shape)
      xpos, xmat = [q[0:3], q[7:10]], [gt.from_quat(k1, q[0:3], q[3:7]).mat, gt.from_quat(k2, q[7:10], q[10:14]).mat]
      want, _, _ = T.class_truth(name, mjm, xpos, xmat)
      got = T.oracle("f64", k1, xpos[0], xmat[0], k2, xpos[1], xmat[1])[0]
      assert abs(got - want) < (1e-12 if want > 0 else 1e-6), (name, got, want)


# ---- GPU: the pair classes ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run_class(name):
  mjm = T.model(name)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=NW, nconmax=16, njmax=64)
  d.qpos.assign(T.poses(name))
  mjw.forward(m, d)
  return mjm, d.sensordata.numpy().copy(), d.geom_xpos.numpy().astype(np.float64), d.geom_xmat.numpy().astype(np.float64).reshape(NW, -1, 3, 3), d.overflow.numpy().copy()


def _surface_distance(shape, x):
  """|distance| of x to the shape's surface: closed form, first order for an ellipsoid, the largest facet offset for a hull."""
  if shape.kind == "ellipsoid":
    F, g = gt.ellipsoid_implicit(shape, x)
    return abs(float(F / g))
  if shape.kind == "mesh":
    from scipy.spatial import ConvexHull

    eq = ConvexHull(shape.vert).equations
    return abs(float((eq[:, :3] @ shape.local(x) + eq[:, 3]).max()))
  return abs(float(gt.sdf(shape, x)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_pair_class(name):
  mjm, sd, xpos, xmat, ovf = _run_class(name)
  assert (ovf == 0).all()
  tol, worst, nsep, npen = bound(name), dict(dist=0.0, witness=0.0, gap=0.0, normal=0.0), 0, 0
  for w in range(NW):
    want, s1, s2 = T.class_truth(name, mjm, xpos[w], xmat[w])
    d12, n12, f12, d21, n21, f21 = sd[w, 0], sd[w, 1:4], sd[w, 4:10], sd[w, 10], sd[w, 11:14], sd[w, 14:20]
    # swap: the pair is ordered before GJK, so both orders run the same arithmetic
    assert _bits(d12) == _bits(d21) and (_bits(n12) == _bits(-n21)).all() and (_bits(f12[:3]) == _bits(f21[3:])).all() and (_bits(f12[3:]) == _bits(f21[:3])).all(), (name, w)
    frm, to = f12[:3].astype(np.float64), f12[3:].astype(np.float64)
    errs = dict(witness=max(_surface_distance(s1, frm), _surface_distance(s2, to)), gap=abs(np.linalg.norm(to - frm) - abs(float(d12))))
    if want is not None:
      errs["dist"] = abs(float(d12) - want)
      nsep, npen = nsep + (want >= 0), npen + (want < 0)
    if abs(d12) > 1e-3:
      errs["normal"] = float(np.abs(n12 - (to - frm) / np.linalg.norm(to - frm)).max())
      assert errs["normal"] <= 1e-5, (name, w, errs)
    assert abs(np.linalg.norm(n12.astype(np.float64)) - 1.0) <= 1e-6, (name, w)
    for k, v in errs.items():
      worst[k] = max(worst[k], v)
    print(name, w, "want", want, "got", float(d12), {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.get("dist", 0.0), errs["witness"], errs["gap"]) <= tol, (name, w, want, float(d12), errs, tol)
  print(name, "bound", tol, "worst", worst, "separated", nsep, "penetrating", npen)
  assert nsep >= 5 and npen >= 2  # (the sweep covers both regimes)


# ---- GPU: cutoff --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere_box", "box_box"])
def test_gpu_cutoff_rules(name):
  """The same pair beyond the cutoff, inside it and penetrating deeper than it; cutoff 0.05, cutoff 0 and (for the values) cutoff 10."""
  sensors = "".join(f'<{tag} name="{tag[0]}{c}" geom1="g1" geom2="g2" cutoff="{c}"/>' for c in (0.05, 0, 10) for tag in ("distance", "normal", "fromto"))
  mjm = T.model(name, sensors=sensors)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=3, nconmax=16, njmax=64)
  # geom 2 is the box (half extent 0.12 along z); geom 1 sits above its top face: bottom of geom 1 at gap g
  half1 = 0.11 if name == "sphere_box" else 0.12
  q = np.zeros((3, 14), dtype=np.float32)
  q[:, 3] = q[:, 10] = 1.0
  for w, gap in enumerate((0.2, 0.02, -0.08)):
    q[w, 0:3] = [0.01, -0.02, 0.12 + half1 + gap]
  d.qpos.assign(q)
  mjw.forward(m, d)
  sd = d.sensordata.numpy()
  c05, c0, c10 = sd[:, 0:10], sd[:, 10:20], sd[:, 20:30]
  tol = bound(name)
  np.testing.assert_allclose(c10[:, 0], [0.2, 0.02, -0.08], atol=tol, rtol=0)
  # cutoff 0.05
  assert c05[0, 0] == np.float32(0.05) and (c05[0, 1:] == 0).all()
  assert abs(c05[1, 0] - 0.02) <= tol and np.abs(c05[1, 1:] - c10[1, 1:]).max() <= tol
  assert c05[2, 0] == np.float32(-0.05) and np.abs(c05[2, 1:] - c10[2, 1:]).max() <= tol  # (normal / fromto are never clamped)
  np.testing.assert_allclose(c05[1:, 1:4], [[0, 0, -1], [0, 0, 1]], atol=1e-5)  # (penetrating: from geom 2 into geom 1)
  np.testing.assert_allclose(c05[1:, 6] - c05[1:, 9], [0.02, -0.08], atol=2 * tol)  # from.z - to.z = the signed distance along z
  # cutoff 0: separated pairs read 0, penetration is reported unclamped
  assert (c0[:2, :] == 0).all()
  assert abs(c0[2, 0] + 0.08) <= tol and np.abs(c0[2, 1:] - c10[2, 1:]).max() <= tol


# ---- GPU: bodies -------------------------------------------------------------------------------------------------------------------------
def _two_bodies_xml():
  geoms = lambda p: (f'<geom name="{p}0" type="sphere" size=".06"/><geom name="{p}1" type="capsule" size=".04 .09" pos=".2 0 0" euler="0 60 0"/>'
                     f'<geom name="{p}2" type="box" size=".05 .07 .04" pos="0 .2 .05" euler="20 0 30"/>')
  pairs = "".join(f'<distance name="d{i}{j}" geom1="a{i}" geom2="b{j}" cutoff="10"/><fromto name="f{i}{j}" geom1="a{i}" geom2="b{j}" cutoff="10"/>' for i in range(3) for j in range(3))
  return f"""<mujoco><worldbody><body name="a"><freejoint/>{geoms("a")}</body><body name="b"><freejoint/>{geoms("b")}</body></worldbody>
    <sensor><distance name="dab" body1="a" body2="b" cutoff="10"/><normal name="nab" body1="a" body2="b" cutoff="10"/><fromto name="fab" body1="a" body2="b" cutoff="10"/>
    <distance name="dba" body1="b" body2="a" cutoff="10"/><fromto name="fba" body1="b" body2="a" cutoff="10"/>{pairs}</sensor></mujoco>"""


@pytest.mark.gpu
def test_gpu_body_body_is_the_minimum_of_its_pairs():
  mjm = mjw.mjcf.from_xml_string(_two_bodies_xml())
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=NW, nconmax=32, njmax=128)
  rng = np.random.default_rng(5)
  q = np.zeros((NW, 14), dtype=np.float32)
  for w in range(NW):
    u = rng.normal(size=3)
    q[w] = np.concatenate([rng.uniform(-0.1, 0.1, 3), rng.normal(size=4), rng.uniform(-0.1, 0.1, 3) + u / np.linalg.norm(u) * rng.uniform(0.25, 0.8), rng.normal(size=4)])
  d.qpos.assign(q)
  mjw.forward(m, d)
  sd = d.sensordata.numpy()
  assert m.nsensor_collision == 23
  dab, nab, fab, dba, fba = sd[:, 0], sd[:, 1:4], sd[:, 4:10], sd[:, 10], sd[:, 11:17]
  pair = sd[:, 17:].reshape(NW, 9, 7)  # (distance, fromto) of pair 3 i + j
  winners = set()
  for w in range(NW):
    k = int(np.argmin(pair[w, :, 0]))  # (the first of equals, as the kernel's tie rule)
    winners.add(k)
    assert _bits(dab[w]) == _bits(pair[w, k, 0]) and (_bits(fab[w]) == _bits(pair[w, k, 1:])).all(), w
    assert _bits(dba[w]) == _bits(dab[w]) and (_bits(fba[w, :3]) == _bits(fab[w, 3:])).all() and (_bits(fba[w, 3:]) == _bits(fab[w, :3])).all()
    v = (fab[w, 3:] - fab[w, :3]).astype(np.float64)
    assert np.abs(nab[w] - v / np.linalg.norm(v)).max() <= 1e-5
  assert len(winners) >= 4  # (different pairs win in different worlds)


@pytest.mark.gpu
def test_gpu_seventy_spheres_take_a_second_trip():
  balls = "".join(f'<geom name="s{i}_{j}" type="sphere" size=".02" pos="{0.05 * (i - 4.5):.3f} {0.05 * (j - 3):.3f} {0.002 * ((3 * i + 5 * j) % 7):.3f}"/>' for i in range(10) for j in range(7))
  xml = f"""<mujoco><worldbody><body name="raft"><freejoint/>{balls}</body><body name="slab"><freejoint/><geom name="box" type="box" size=".1 .07 .12"/></body></worldbody>
    <sensor><distance name="d" body1="raft" body2="slab" cutoff="10"/><fromto name="f" body1="raft" body2="slab" cutoff="10"/><distance name="r" body1="slab" body2="raft" cutoff="10"/></sensor></mujoco>"""
  mjm = mjw.mjcf.from_xml_string(xml)
  m = mjw.put_model(mjm)
  nw = 16
  d = mjw.make_data(mjm, nworld=nw, nconmax=80, njmax=256)
  rng = np.random.default_rng(11)
  q = np.zeros((nw, 14), dtype=np.float32)
  for w in range(nw):
    u, qr = rng.normal(size=3), rng.normal(size=4)
    if w % 2:  # the slab beyond the raft's +x edge: the nearest sphere is one of the last column, pairs 63..69
      u = gt.from_quat("box", [0, 0, 0], qr).mat @ np.array([1.0, rng.uniform(-0.2, 0.4), rng.uniform(-0.2, 0.2)])
    q[w] = np.concatenate([np.zeros(3), qr, u / np.linalg.norm(u) * rng.uniform(0.3 if w % 2 else 0.15, 0.6), rng.normal(size=4)])
  d.qpos.assign(q)
  mjw.forward(m, d)
  sd, xpos, xmat = d.sensordata.numpy(), d.geom_xpos.numpy().astype(np.float64), d.geom_xmat.numpy().astype(np.float64).reshape(nw, -1, 3, 3)
  tol, late = bound("sphere_box"), 0
  for w in range(nw):
    box = gt.Shape("box", xpos[w, 70], xmat[w, 70], [0.1, 0.07, 0.12])
    each = gt.sdf(box, xpos[w, :70]) - 0.02
    k = int(np.argmin(each))
    late += k >= 64
    print(w, "winner", k, "want", each[k], "got", sd[w, 0])
    assert abs(sd[w, 0] - each[k]) <= tol and _bits(sd[w, 7]) == _bits(sd[w, 0])
    assert abs(np.linalg.norm(sd[w, 1:4].astype(np.float64) - xpos[w, k]) - 0.02) <= tol  # `from` lies on the winning sphere
    assert abs(float(gt.sdf(box, sd[w, 4:7].astype(np.float64)))) <= tol
  assert late >= 1  # (a sphere of the second trip wins somewhere)


@pytest.mark.gpu
def test_gpu_two_penetrating_pairs_of_one_sensor():
  """Both boxes of body `a` sink into the slab, at different depths: the wavefront serves EPA twice for one sensor."""
  xml = """<mujoco><worldbody>
    <body name="a"><freejoint/><geom name="a0" type="box" size=".05 .05 .05" pos="-.15 0 0"/><geom name="a1" type="box" size=".05 .04 .05" pos=".15 0 0" euler="0 0 25"/></body>
    <body name="slab"><freejoint/><geom name="s" type="box" size=".3 .3 .1"/></body></worldbody>
    <sensor><distance name="d" body1="a" geom2="s" cutoff="10"/><fromto name="f" body1="a" geom2="s" cutoff="10"/>
      <distance name="d0" geom1="a0" geom2="s" cutoff="10"/><fromto name="f0" geom1="a0" geom2="s" cutoff="10"/>
      <distance name="d1" geom1="a1" geom2="s" cutoff="10"/><fromto name="f1" geom1="a1" geom2="s" cutoff="10"/></sensor></mujoco>"""
  mjm = mjw.mjcf.from_xml_string(xml)
  m = mjw.put_model(mjm)
  nw = 16
  d = mjw.make_data(mjm, nworld=nw, nconmax=32, njmax=128)
  rng = np.random.default_rng(3)
  q = np.zeros((nw, 14), dtype=np.float32)
  for w in range(nw):
    tilt = rng.uniform(-0.03, 0.03, 2)  # (a few degrees: the boxes' bottoms differ by up to 9 mm, less than the 20 .. 40 mm they sink in)
    q[w] = [0.02, -0.03, 0.1 + 0.05 - rng.uniform(0.02, 0.04), 1, tilt[0], tilt[1], 0, 0, 0, 0, 1, 0, 0, 0]
  d.qpos.assign(q)
  mjw.forward(m, d)
  assert (d.overflow.numpy() == 0).all()
  sd, xpos, xmat = d.sensordata.numpy(), d.geom_xpos.numpy().astype(np.float64), d.geom_xmat.numpy().astype(np.float64).reshape(nw, -1, 3, 3)
  sizes, tol, first = np.asarray(mjm.geom_size, dtype=np.float64), bound("box_box"), 0
  for w in range(nw):
    boxes = [gt.Shape("box", xpos[w, g], xmat[w, g], sizes[g]) for g in range(3)]
    want = [-gt.box_box_sat_depth(boxes[g], boxes[2])[0] for g in (0, 1)]
    assert max(want) < -1e-3  # (both pairs penetrate)
    print(w, "want", want, "got", sd[w, 7], sd[w, 14], "sensor", sd[w, 0])
    assert abs(sd[w, 7] - want[0]) <= tol and abs(sd[w, 14] - want[1]) <= tol
    k = 0 if sd[w, 7] <= sd[w, 14] else 1
    first += k == 0
    assert _bits(sd[w, 0]) == _bits(sd[w, 7 + 7 * k]) and (_bits(sd[w, 1:7]) == _bits(sd[w, 8 + 7 * k : 14 + 7 * k])).all()
  assert 0 < first < nw  # (each box is the deeper one somewhere)


# ---- GPU: paths ----------------------------------------------------------------------------------------------------------------------------
_OTHER = '<framepos name="p" objtype="body" objname="b2"/><clock name="t"/><framequat name="q" objtype="geom" objname="g1"/>'
_DIST = "".join(f'<{tag} name="{tag}" geom1="g1" geom2="g2" cutoff="10"/>' for tag in ("distance", "normal", "fromto"))


@pytest.mark.gpu
def test_gpu_paths():
  name = "sphere_box"
  mjm = T.model(name, sensors=_OTHER[: _OTHER.index("<clock")] + _DIST + _OTHER[_OTHER.index("<clock") :])  # p | distance normal fromto | t q
  plain = T.model(name, sensors=_OTHER)
  m, mp = mjw.put_model(mjm), mjw.put_model(plain)
  d, dp = mjw.make_data(mjm, nworld=NW, nconmax=16, njmax=64), mjw.make_data(plain, nworld=NW, nconmax=16, njmax=64)
  q = T.poses(name)
  col, other = np.arange(3, 13), np.r_[0:3, 13:18]

  def reset(dd):
    dd.qpos.assign(q)
    for k in ("qvel", "qacc_warmstart", "time"):
      getattr(dd, k).assign(np.zeros(getattr(dd, k).shape, dtype=np.float32))

  reset(d)
  mjw.forward(m, d)
  fwd = d.sensordata.numpy().copy()
  assert np.abs(fwd[:, col]).max() > 0
  reset(dp)
  mjw.forward(mp, dp)
  assert (_bits(dp.sensordata.numpy()) == _bits(fwd[:, other])).all()  # the other sensors' slots: as without the collision sensors
  # sensor_pos alone rewrites the slots
  d.sensordata.assign(np.full_like(fwd, 7.0))
  mjw.sensor_pos(m, d)
  assert (_bits(d.sensordata.numpy()[:, col]) == _bits(fwd[:, col])).all()
  # step computes the sensors at the step's initial positions
  reset(d)
  mjw.step(m, d)
  assert (_bits(d.sensordata.numpy()) == _bits(fwd)).all()
  # a captured graph, replayed
  reset(d)
  g = mjw.StepGraph(m, d)
  for _ in range(2):
    reset(d)
    d.sensordata.assign(np.full_like(fwd, 7.0))
    g.launch()
    assert (_bits(d.sensordata.numpy()) == _bits(fwd)).all()
  # sensors disabled: the slots keep their content
  off = T.model(name, sensors=_DIST, option='<option><flag sensor="disable"/></option>')
  mo = mjw.put_model(off)
  do = mjw.make_data(off, nworld=NW, nconmax=16, njmax=64)
  do.qpos.assign(q)
  do.sensordata.assign(np.full(do.sensordata.shape, 7.0, dtype=np.float32))
  mjw.step(mo, do)
  mjw.forward(mo, do)
  assert (do.sensordata.numpy() == 7.0).all()


@pytest.mark.gpu
def test_gpu_batched_geom_size():
  name = "sphere_box"
  mjm = T.model(name)
  m = mjw.put_model(mjm, batch_sizes={"geom_size": NW})
  d = mjw.make_data(mjm, nworld=NW, nconmax=16, njmax=64)
  size = np.tile(np.asarray(mjm.geom_size, dtype=np.float32), (NW, 1, 1))
  size[:, 0, 0] = 0.05 + 0.004 * np.arange(NW)  # the sphere's radius, world by world
  m.geom_size.assign(size)
  d.qpos.assign(np.tile(T.poses(name)[1], (NW, 1)))  # one pose: only the radius differs
  mjw.forward(m, d)
  sd, xpos, xmat = d.sensordata.numpy(), d.geom_xpos.numpy().astype(np.float64), d.geom_xmat.numpy().astype(np.float64).reshape(NW, -1, 3, 3)
  for w in range(NW):
    want = float(gt.sdf(gt.Shape("box", xpos[w, 1], xmat[w, 1], T.SIZES["box"]), xpos[w, 0])) - float(size[w, 0, 0])
    assert abs(sd[w, 0] - want) <= bound(name), (w, sd[w, 0], want)
  assert len(set(sd[:, 0].tolist())) == NW


# ---- GPU: insidesite -----------------------------------------------------------------------------------------------------------------------
_ZONES = (("sphere", ".16"), ("capsule", ".09 .12"), ("ellipsoid", ".12 .2 .09"), ("cylinder", ".14 .1"), ("box", ".12 .15 .08"))
_ZONE_SIZE = {"sphere": [0.16], "capsule": [0.09, 0.12], "ellipsoid": [0.12, 0.2, 0.09], "cylinder": [0.14, 0.1], "box": [0.12, 0.15, 0.08]}
_OBJ = (("body", "o"), ("xbody", "o"), ("geom", "og"), ("site", "os"))


def _insidesite_xml():
  zones = "".join(f'<site name="z{k}" type="{k}" size="{s}" pos="{0.01 * i} -.01 .02" euler="{25 * i} {40 - 15 * i} 10"/>' for i, (k, s) in enumerate(_ZONES))
  sensors = "".join(f'<insidesite name="{k}_{t}" site="z{k}" objtype="{t}" objname="{n}"/>' for k, _ in _ZONES for t, n in _OBJ)
  return f"""<mujoco><worldbody>{zones}<body name="o"><freejoint/><geom name="og" type="box" size=".02 .03 .01" pos=".05 0 .02"/>
    <geom name="ballast" type="sphere" size=".03" pos="-.02 .06 0" density="4000"/><site name="os" pos="0 -.06 .03"/></body></worldbody><sensor>{sensors}</sensor></mujoco>"""


def _site_margin(kind, pos, mat, x):
  """Signed distance of x to the site's surface (first order for the ellipsoid), negative inside."""
  s = gt.Shape(kind, pos, mat, _ZONE_SIZE[kind])
  if kind == "ellipsoid":
    F, g = gt.ellipsoid_implicit(s, x)
    return float(F / g)
  return float(gt.sdf(s, x))


@pytest.mark.gpu
def test_gpu_insidesite():
  mjm = mjw.mjcf.from_xml_string(_insidesite_xml())
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=NW, nconmax=8, njmax=32)
  rng = np.random.default_rng(2)
  q = np.zeros((NW, 7), dtype=np.float32)
  for w in range(NW):
    u = rng.normal(size=3)
    q[w] = np.concatenate([u / np.linalg.norm(u) * rng.uniform(0.02, 0.3), rng.normal(size=4)])
  d.qpos.assign(q)
  mjw.forward(m, d)
  sd = d.sensordata.numpy()
  point = {"body": d.xipos.numpy()[:, 1], "xbody": d.xpos.numpy()[:, 1], "geom": d.geom_xpos.numpy()[:, 0], "site": d.site_xpos.numpy()[:, 5]}
  zpos, zmat = d.site_xpos.numpy().astype(np.float64), d.site_xmat.numpy().astype(np.float64).reshape(NW, -1, 3, 3)
  names, seen = mjm.sensor_names, {}
  for w in range(NW):
    for i, (k, _) in enumerate(_ZONES):
      for t, _ in _OBJ:
        margin = _site_margin(k, zpos[w, i], zmat[w, i], point[t][w].astype(np.float64))
        got = sd[w, mjm.sensor_adr[names.index(f"{k}_{t}")]]
        if abs(margin) < 1e-4:  # (float32 could flip the answer: such a point proves nothing, and the seed above has none)
          raise AssertionError(f"world {w} {k} {t}: the point lies {margin:.1e} from the surface")
        assert got == (1.0 if margin < 0 else 0.0), (w, k, t, margin, got)
        seen.setdefault((k, t), set()).add(margin < 0)
  assert all(v == {True, False} for v in seen.values()) and len(seen) == 20  # every zone x object type was seen inside and outside
  assert np.abs(point["body"] - point["xbody"]).max() > 0.01  # (the four object positions really differ)


# ---- GPU: the launch list -------------------------------------------------------------------------------------------------------------------
def _kernels_of_a_step(m, d):
  """Names of the kernels one step launches (the profiler's device activity records)."""
  import torch
  from torch.profiler import ProfilerActivity, profile

  mjw.step(m, d)  # (first-use set-up: attributes, workspaces)
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CUDA]) as prof:
    mjw.step(m, d)
    torch.cuda.synchronize()
  return [e.name for e in prof.events() if e.name.startswith(("k_", "void k_"))]


@pytest.mark.gpu
def test_gpu_launch_list(humanoid):
  def names(mjm, **kw):
    m = mjw.put_model(mjm)
    d = mjw.make_data(mjm, nworld=8, **kw)
    got = _kernels_of_a_step(m, d)
    assert any("k_" in n for n in got), got  # (the profiler saw the step)
    return got

  sensor = lambda got: [n for n in got if "k_sensor" in n]
  base = names(humanoid, nconmax=24, njmax=64)
  assert not any("k_sensor_collision" in n for n in base) and not any("k_sensor_contact" in n for n in base)
  contact_only = """<mujoco><worldbody><geom name="floor" type="plane" size="5 5 .1"/><body pos="0 0 .09"><freejoint/><geom name="ball" type="sphere" size=".1"/></body></worldbody>
    <sensor>{}</sensor></mujoco>"""
  got = names(mjw.mjcf.from_xml_string(contact_only.format('<contact geom1="ball" geom2="floor" data="found force dist"/>')), nconmax=8, njmax=16)
  assert len(sensor(got)) == 1 and "k_sensor_contact" in sensor(got)[0]
  without = names(mjw.mjcf.from_xml_string(contact_only.format("")), nconmax=8, njmax=16)
  got = names(mjw.mjcf.from_xml_string(contact_only.format('<distance geom1="ball" geom2="floor" cutoff="1"/>')), nconmax=8, njmax=16)
  assert len(sensor(got)) == 1 and "k_sensor_collision" in sensor(got)[0]  # (k_sensor itself has nothing to do)
  assert [n for n in got if "k_sensor" not in n] == without  # the rest of the step is the sensorless model's
