"""Contact sensors (<sensor><contact .../>, mjSENS_CONTACT = 42; csrc/sensor_contact.hpp).

CPU: the loader's tables, the ABI additions, and self-checks of the numpy truth (tests/contact_sensor_truth.py) on hand-made contacts, so
that the yardstick is not merely a copy of the kernel.  GPU: every world's sensordata against the truth fed the engine's own public
contact arrays, contact forces and site poses.

Tolerances: found / dist / pos / normal / tangent and every zero-filled slot are copies -- bitwise.  force / torque: relerr <= 1e-6 (the
same float32 constraint forces summed, possibly in another order).  netforce: relerr <= 1e-5 (at most 64 float32 terms: 64 x 6e-8, with a
margin); force and torque of a netforce slot are measured together as one wrench, because the torque's terms are lever arm x force with
lever arms of at most ~1 m in these scenes and its own value (about the centroid) may cancel to nothing; the centroid is measured on its own.
"""

import numpy as np
import pytest

import conftest
import contact_sensor_truth as truth

import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi, io

# ---- loader ---------------------------------------------------------------------------------------------------------------------------

_LOADER_WORLD = """
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1"/>
    <site name="zone" type="box" size=".1 .1 .1"/>
    <body name="a" pos="0 0 .1"><freejoint/><geom name="ga" type="sphere" size=".1"/>
      <body name="b" pos=".3 0 0"><joint name="jb" type="hinge" axis="0 1 0"/><geom name="gb" type="sphere" size=".1"/></body>
    </body>
  </worldbody>
"""


def _load(sensors, custom=""):
  return mjw.mjcf.from_xml_string(f"<mujoco>{custom}{_LOADER_WORLD}<sensor>{sensors}</sensor></mujoco>")


# attributes -> (objtype, objid, reftype, refid, (dataspec, reduce, num), dim); geoms: floor 0, ga 1, gb 2; bodies: world 0, a 1, b 2
_COMBOS = [
  ('', (0, -1, 0, -1, (1, 0, 1), 1)),
  ('geom1="ga"', (5, 1, 0, -1, (1, 0, 1), 1)),
  ('geom1="ga" geom2="floor" data="found force"', (5, 1, 5, 0, (3, 0, 1), 4)),
  ('geom2="floor" data="force"', (0, -1, 5, 0, (2, 0, 1), 3)),
  ('body1="b" num="3" data="torque"', (1, 2, 0, -1, (4, 0, 3), 9)),
  ('body1="a" body2="b" data="dist" reduce="mindist"', (1, 1, 1, 2, (8, 1, 1), 1)),
  ('subtree1="a" data="pos" num="2" reduce="maxforce"', (2, 1, 0, -1, (16, 2, 2), 6)),
  ('subtree1="a" subtree2="b" data="normal"', (2, 1, 2, 2, (32, 0, 1), 3)),
  ('site="zone" data="tangent"', (6, 0, 0, -1, (64, 0, 1), 3)),
  ('site="zone" geom2="gb" data="found dist"', (6, 0, 5, 2, (9, 0, 1), 2)),
  ('data="found force torque dist pos normal tangent" num="4"', (0, -1, 0, -1, (127, 0, 4), 68)),
  ('geom1="gb" data="force torque pos" reduce="netforce" num="2"', (5, 2, 0, -1, (22, 3, 2), 18)),
]


def test_loader_tables():
  mjm = _load("".join(f'<contact name="c{i}" {attrs}/>' for i, (attrs, _) in enumerate(_COMBOS)) + '<jointpos name="jp" joint="jb"/>')
  n = len(_COMBOS)
  assert mjm.nsensor == n + 1 and (mjm.sensor_type[:n] == 42).all() and (mjm.sensor_datatype[:n] == 0).all() and (mjm.sensor_needstage[:n] == 3).all()
  for i, (attrs, (ot, oi, rt, ri, prm, dim)) in enumerate(_COMBOS):
    got = (int(mjm.sensor_objtype[i]), int(mjm.sensor_objid[i]), int(mjm.sensor_reftype[i]), int(mjm.sensor_refid[i]), tuple(int(x) for x in mjm.sensor_intprm[i]), int(mjm.sensor_dim[i]))
    assert got == (ot, oi, rt, ri, prm, dim), (attrs, got)
    assert dim == prm[2] * truth.slot_layout(prm[0])[1]
  assert mjm.sensor_intprm.shape == (n + 1, 3) and (mjm.sensor_intprm[n] == 0).all()
  assert (mjm.sensor_adr == np.concatenate([[0], np.cumsum(mjm.sensor_dim)[:-1]])).all()
  assert mjm.nsensordata == sum(c[1][5] for c in _COMBOS) + 1
  assert (mjw.ObjType.UNKNOWN, mjw.ObjType.BODY, mjw.ObjType.XBODY, mjw.ObjType.GEOM, mjw.ObjType.SITE) == (0, 1, 2, 5, 6)


@pytest.mark.parametrize("attrs", [
  'data="force found"',  # wrong order
  'data="found found"',  # repeat
  'data="found depth"',  # unknown word
  'data=""',
  'geom1="ga" body1="a"',  # two first objects
  'subtree1="a" site="zone"',
  'geom2="ga" body2="a"',  # two second objects
  'geom1="nope"', 'body2="nope"', 'site="nope"', 'subtree1="nope"',  # unknown names
  'reduce="median"',
  'num="0"',
])
def test_loader_refuses(attrs):
  with pytest.raises(ValueError):
    _load(f"<contact {attrs}/>")


def test_maxmatch_numeric():
  custom = '<custom><numeric name="other" data="3 4"/><numeric name="contact_sensor_maxmatch" data="{}"/><text name="t" data="x"/></custom>'
  assert mjw.put_model(_load("<contact/>")).opt.contact_sensor_maxmatch == 64  # the default
  mjm = _load("<contact/>", custom.format(7))
  assert mjm.numeric_names == ["other", "contact_sensor_maxmatch"] and mjm.numeric_data.tolist() == [3.0, 4.0, 7.0]
  m = mjw.put_model(mjm)
  assert m.opt.contact_sensor_maxmatch == 7 and io.c_model(m).contact_sensor_maxmatch == 7
  for bad in (65, 0):
    with pytest.raises(ValueError, match="wavefront"):
      mjw.put_model(_load("<contact/>", custom.format(bad)))
  m.opt.contact_sensor_maxmatch = 65  # re-bound after put_model: refused when the C struct is rebuilt
  with pytest.raises(ValueError, match="wavefront"):
    io.c_model(m)


def test_abi_and_io(humanoid):
  assert _abi.DEFINES["MJH_ABI_VERSION"] == 45
  assert [f[0] for f in _abi.MODEL_FIELDS[-4:]] == ["nsensor_contact", "contact_sensor_maxmatch", "sensor_intprm", "sensor_contact_adr"]
  assert io._MODEL_ARRAYS["sensor_intprm"] == (("nsensor", 3), "int32", False) and io._MODEL_ARRAYS["sensor_contact_adr"] == (("nsensor",), "int32", False)
  assert "sensor_contact_tu.hip" in _abi.UNITS and "sensor_contact.hpp" in _abi.HEADERS
  m = mjw.put_model(humanoid)
  assert m.nsensor_contact == 0 and io.c_model(m).nsensor_contact == 0 and m.sensor_intprm.shape == (m.nsensor, 3) and m.sensor_contact_adr.shape == (m.nsensor,)
  mjm = _load('<jointpos joint="jb"/><contact geom1="ga"/><clock/><contact data="force" num="2"/>')
  m = mjw.put_model(mjm)
  assert m.nsensor_contact == 2 and m.nsensor_acc == 2  # (contact sensors belong to the acceleration stage)
  assert m.sensor_contact_adr.numpy().tolist() == [1, 3, -1, -1] and m.sensor_intprm.numpy().tolist() == [[0, 0, 0], [1, 0, 1], [0, 0, 0], [2, 0, 2]]
  assert mjw.OverflowType.CONTACT_MATCH == 64
  mjm.sensor_intprm = mjm.sensor_intprm.copy()
  mjm.sensor_intprm[3, 2] = 3  # num no longer agrees with sensor_dim
  with pytest.raises(ValueError, match="sensor_intprm"):
    mjw.put_model(mjm)


# ---- the truth on hand-made contacts ----------------------------------------------------------------------------------------------------

# bodies: 0 world, 1 root, 2 child of 1, 3 child of 2, 4 another root; geoms 0 (world), 1..4 on bodies 1..4, 5 a second geom of body 2
_GEOM_BODYID = np.array([0, 1, 2, 3, 4, 2])
_BODY_PARENTID = np.array([0, 0, 1, 2, 0])
_NO_SITES = dict(site_type=np.zeros(0, int), site_size=np.zeros((0, 3)), site_xpos=np.zeros((0, 3)), site_xmat=np.zeros((0, 9)))


def _rot(axis, angle):
  axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
  K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
  return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _hand_contacts(seed=0):
  rng = np.random.default_rng(seed)
  geom = np.array([[0, 1], [0, 2], [1, 4], [0, 3], [5, 0], [2, 4], [0, 4], [3, 4]])
  n = len(geom)
  frame = np.array([_rot(rng.normal(size=3), rng.uniform(0, 3)) for _ in range(n)]).astype(np.float32)
  return dict(dist=rng.uniform(-0.01, 0.0, n).astype(np.float32), pos=rng.normal(size=(n, 3)).astype(np.float32), frame=frame, geom=geom,
              force=np.concatenate([rng.uniform(1, 9, (n, 1)), rng.normal(size=(n, 5))], axis=1).astype(np.float32))


def _truth(objtype, objid, reftype, refid, intprm, con, sites=_NO_SITES, maxmatch=64):
  return truth.sensor(objtype, objid, reftype, refid, intprm, _GEOM_BODYID, _BODY_PARENTID, sites["site_type"], sites["site_size"], sites["site_xpos"], sites["site_xmat"],
                      con["dist"], con["pos"], con["frame"], con["geom"], con["force"], maxmatch)[0]


def test_truth_swapping_the_objects_flips_the_direction():
  con = _hand_contacts()
  a = _truth(truth.BODY, 4, truth.GEOM, 0, (127, 0, 3), con).reshape(3, -1)
  b = _truth(truth.GEOM, 0, truth.BODY, 4, (127, 0, 3), con).reshape(3, -1)
  assert a[0, 0] == 1 and a[0, 1] > 0  # one match: contact 6, geoms (0, 4)
  lab = truth.labels(127, 1)
  flipped = np.isin(lab, ("normal", "tangent"))
  flipped[[3, 6]] = True  # f2 and f5
  assert (a[:, flipped] == -b[:, flipped]).all() and (a[:, ~flipped] == b[:, ~flipped]).all() and np.abs(a[0, flipped]).min() > 0


def test_truth_subtree_is_the_union_of_its_bodies():
  con = _hand_contacts(1)
  spec = 2 + 4 + 8 + 16 + 32 + 64  # everything but found, which counts the sensor's own matches
  whole = _truth(truth.XBODY, 1, 0, -1, (spec | 1, 0, 8), con).reshape(8, -1)
  n = int(whole[0, 0])
  assert n == 7  # the subtree of body 1 is bodies 1, 2, 3: every contact but (0, 4)
  rows = []
  for body in (1, 2, 3):
    part = _truth(truth.BODY, body, 0, -1, (spec | 1, 0, 8), con).reshape(8, -1)
    rows += [tuple(r[1:]) for r in part[: int(part[0, 0])]]
  assert len(rows) == n and sorted(rows) == sorted(tuple(r[1:]) for r in whole[:n])
  # a contact INSIDE the subtree is seen by both of its bodies, from opposite sides: the union holds for the direction-free fields
  con["geom"][5] = [1, 5]
  whole = _truth(truth.XBODY, 1, 0, -1, (8 + 16, 0, 8), con).reshape(8, -1)
  rows = [tuple(r) for body in (1, 2, 3) for r in _truth(truth.BODY, body, 0, -1, (1 + 8 + 16, 0, 8), con).reshape(8, -1) if r[0] > 0]
  assert len(rows) == 8 and sorted(set(r[1:] for r in rows)) == sorted(tuple(r) for r in whole[:7])


def test_truth_netforce():
  R = _rot([1, 2, 3], 0.7).astype(np.float32)
  one = dict(dist=np.float32([-0.001]), pos=np.float32([[0.3, -0.2, 0.1]]), frame=R[None], geom=np.array([[0, 1]]), force=np.float32([[5, 1, -2, 0.3, 0.1, -0.2]]))
  lab = truth.labels(127, 1)
  out = _truth(truth.GEOM, 0, 0, -1, (127, 3, 1), one)
  f = one["force"][0].astype(np.float64)
  np.testing.assert_allclose(out[lab == "torque"], R.astype(np.float64).T @ f[3:], atol=1e-12)  # about its own position: the rotated contact torque
  np.testing.assert_allclose(out[lab == "force"], R.astype(np.float64).T @ f[:3], atol=1e-12)
  np.testing.assert_allclose(out[lab == "pos"], one["pos"][0], atol=1e-12)
  assert out[lab == "found"] == 1 and out[lab == "dist"] == 0 and out[lab == "normal"].tolist() == [1, 0, 0] and out[lab == "tangent"].tolist() == [0, 1, 0]
  # two equal and opposite contacts on geom 1: once as the first, once as the second geom of the pair
  two = dict(dist=np.float32([0, 0]), pos=np.float32([[0.3, -0.2, 0.1], [-0.5, 0.4, 0.2]]), frame=np.stack([R, R]), geom=np.array([[0, 1], [1, 2]]),
             force=np.float32([[5, 1, -2, 0, 0, 0], [5, 1, -2, 0, 0, 0]]))
  out = _truth(truth.GEOM, 1, 0, -1, (127, 3, 1), two)
  assert np.abs(out[lab == "force"]).max() < 1e-12 and out[lab == "found"] == 2
  np.testing.assert_allclose(out[lab == "pos"], two["pos"].mean(axis=0), atol=1e-7)  # equal weights


def test_truth_sorts_are_stable_and_the_cap_comes_first():
  con = _hand_contacts(2)
  con["dist"] = np.float32([-0.003, -0.001, -0.003, -0.002, -0.001, -0.004, -0.003, -0.002])
  out = _truth(0, -1, 0, -1, (9, 1, 8), con).reshape(8, 2)
  assert out[:, 1].tolist() == sorted(con["dist"].tolist()) and (out[:, 0] == 8).all()
  pos = _truth(0, -1, 0, -1, (16, 1, 8), con).reshape(8, 3)
  order = [int(np.flatnonzero((con["pos"] == p.astype(np.float32)).all(axis=1))[0]) for p in pos]
  assert order == [5, 0, 2, 6, 3, 7, 1, 4]  # ties in contact order
  capped, ovf = truth.sensor(0, -1, 0, -1, (9, 1, 8), _GEOM_BODYID, _BODY_PARENTID, *(_NO_SITES[k] for k in ("site_type", "site_size", "site_xpos", "site_xmat")),
                             con["dist"], con["pos"], con["frame"], con["geom"], con["force"], maxmatch=2)
  capped = capped.reshape(8, 2)
  assert ovf and capped[:2].tolist() == [[2, np.float32(-0.003)], [2, np.float32(-0.001)]] and (capped[2:] == 0).all()  # the first two, not the two nearest


def test_truth_maxforce_separation_for_masses_1_2_4():
  """The GPU test's maxforce cases need criteria that rounding cannot reorder: neighbours differ by more than 1e-3 relative.  Weights in
  the ratio 1 : 2 : 4 give squared forces 1 : 4 : 16."""
  con = _hand_contacts(3)
  con["geom"] = con["geom"][:3]
  con["force"] = np.float32([[2 * 9.81, 0, 0, 0, 0, 0], [4 * 9.81, 0.1, 0, 0, 0, 0], [1 * 9.81, 0, 0.1, 0, 0, 0]])
  key = np.sort(truth.criteria(truth.MAXFORCE, [(0, 1.0), (1, 1.0), (2, 1.0)], con["dist"], con["force"]))
  assert _separated(key)
  out = _truth(0, -1, 0, -1, (2, 2, 3), con).reshape(3, 3)
  assert out[:, 0].tolist() == [np.float32(4 * 9.81), np.float32(2 * 9.81), np.float32(9.81)]


def _separated(sorted_keys):
  k = np.asarray(sorted_keys, dtype=np.float64)
  return len(k) < 2 or bool(np.all(np.diff(k) > 1e-3 * np.maximum(np.abs(k[1:]), np.abs(k[:-1]))))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

# Scene A.  geoms: floor 0, s1 1, s2 2, s4 3, slab 4, upper 5, lower 6.  link1's parent is the world, so the floor ignores `upper`; `lower` rests on it.
def _scene_a(cone="pyramidal", flags=""):
  return f"""
<mujoco>
  <option timestep="0.002" cone="{cone}">{flags}</option>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1"/>
    <site name="zone" type="box" pos=".5 0 0" size=".06 .06 .05"/>
    <site name="row" type="box" pos=".5 0 0" size=".75 .1 .05" euler="0 0 2"/>
    <body name="b1" pos="0 0 .1"><freejoint/><geom name="s1" type="sphere" size=".1" mass="1"/></body>
    <body name="b2" pos=".5 0 .1"><freejoint/><geom name="s2" type="sphere" size=".1" mass="2"/></body>
    <body name="b4" pos="1 0 .1"><freejoint/><geom name="s4" type="sphere" size=".1" mass="4"/><site name="under4" type="cylinder" pos="0 0 -.1" size=".03 .03"/></body>
    <body name="slab" pos="0 1 .05"><freejoint/><geom name="slab" type="box" size=".15 .1 .05" mass="3"/></body>
    <body name="link1" pos="1.5 1 .5">
      <joint name="j1" type="hinge" axis="0 1 0" damping="3"/><geom name="upper" type="capsule" fromto="0 0 0 0 0 -.25" size=".03" mass=".5"/>
      <body name="link2" pos="0 0 -.25"><joint name="j2" type="hinge" axis="0 1 0" damping="3"/><geom name="lower" type="capsule" fromto="0 0 0 0 0 -.3" size=".03" mass=".5"/></body>
    </body>
  </worldbody>
  <sensor>
    <jointpos name="jp" joint="j1"/>
    <contact name="any"/>
    <contact name="all" num="12" data="found force torque dist pos normal tangent"/>
    <contact name="s1" geom1="s1"/>
    <contact name="s1_floor" geom1="s1" geom2="floor" data="found force normal"/>
    <contact name="floor_s1" geom1="floor" geom2="s1" data="found force normal"/>
    <contact name="slab_near" body1="slab" num="3" data="found dist pos" reduce="mindist"/>
    <contact name="slab_all" body1="slab" num="6" data="force torque"/>
    <contact name="chain" subtree1="link1" data="found force pos"/>
    <contact name="zone" site="zone" data="found force"/>
    <contact name="zone_floor" site="zone" geom2="floor" data="found normal tangent"/>
    <contact name="zone_s2" site="zone" geom2="s2" data="found normal tangent"/>
    <contact name="under4" site="under4" data="found dist"/>
    <contact name="f_found" geom1="s2" data="found" num="3"/>
    <contact name="f_force" geom1="s2" data="force"/>
    <contact name="f_torque" geom1="s2" data="torque"/>
    <contact name="f_dist" geom1="s2" data="dist"/>
    <contact name="f_pos" geom1="s2" data="pos"/>
    <contact name="f_normal" geom2="s2" data="normal"/>
    <contact name="f_tangent" body2="b2" data="tangent"/>
    <contact name="near3" num="3" data="found dist" reduce="mindist"/>
    <contact name="strong3" site="row" num="3" data="found force dist" reduce="maxforce"/>
    <contact name="strong1" site="row" data="pos" reduce="maxforce"/>
    <contact name="net_slab" body1="slab" num="2" data="found force torque dist pos normal tangent" reduce="netforce"/>
    <contact name="net_row" site="row" data="force torque pos" reduce="netforce"/>
    <contact name="net_s1" geom1="s1" data="found force pos normal" reduce="netforce"/>
    <clock name="t"/>
  </sensor>
</mujoco>"""


NWORLD_A = 5


def _start_a(mjm, m, d):
  q = d.qpos.numpy()
  for w in range(NWORLD_A):
    q[w, 0:21:7] += 0.01 * w  # the spheres' x
    q[w, 1:21:7] -= 0.004 * w
    q[w, 21] += 0.02 * w  # the slab
    q[w, 28] = 0.5 - 0.02 * w  # j1: the chain's tip starts 5 .. 26 mm inside the floor
    q[w, 29] = 0.05
  q[3, 2] = 0.5  # world 3: sphere s1 in the air -- sensors on it match nothing
  d.qpos.assign(q)


def _world_inputs(mjm, m, d, w, force_all):
  ncon, adr = int(d.ws_ncon.numpy()[w]), int(d.ws_conadr.numpy()[w])
  sl = slice(adr, adr + ncon)
  return dict(geom_bodyid=mjm.geom_bodyid, body_parentid=mjm.body_parentid, site_type=mjm.site_type, site_size=mjm.site_size, site_xpos=d.site_xpos.numpy()[w],
              site_xmat=d.site_xmat.numpy()[w].reshape(-1, 9), dist=d.contact.dist.numpy()[sl], pos=d.contact.pos.numpy()[sl], frame=d.contact.frame.numpy()[sl].reshape(ncon, 3, 3),
              geom=d.contact.geom.numpy()[sl], force=force_all[sl])


def _contact_forces(m, d):
  n = int(d.nacon.numpy()[0])
  ids = mjw.DeviceArray.from_numpy(np.arange(n, dtype=np.int32))
  force = mjw.DeviceArray.zeros((n, 6), dtype=np.float32)
  mjw.contact_force(m, d, ids, False, force)
  return force.numpy()


def _bits(x):
  return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _check_against_truth(mjm, m, d, maxmatch=64, report=None):
  """Every contact sensor of every world against the truth; returns {sensor name: [found per world]}."""
  assert int(d.nacon.numpy()[0]) == int(d.ws_ncon.numpy().sum())  # (the public arrays hold every record)
  force_all, sd = _contact_forces(m, d), d.sensordata.numpy()
  found = {}
  for w in range(d.nworld):
    inp = _world_inputs(mjm, m, d, w, force_all)
    for i in np.flatnonzero(mjm.sensor_type == 42):
      name, prm = mjm.sensor_names[i], mjm.sensor_intprm[i]
      want, ovf = truth.sensor(int(mjm.sensor_objtype[i]), int(mjm.sensor_objid[i]), int(mjm.sensor_reftype[i]), int(mjm.sensor_refid[i]), prm, maxmatch=maxmatch, **inp)
      got = sd[w, mjm.sensor_adr[i] : mjm.sensor_adr[i] + mjm.sensor_dim[i]]
      lab = truth.labels(int(prm[0]), int(prm[2]))
      nmatch = len(truth.matches(int(mjm.sensor_objtype[i]), int(mjm.sensor_objid[i]), int(mjm.sensor_reftype[i]), int(mjm.sensor_refid[i]), inp["geom_bodyid"], inp["body_parentid"],
                                 inp["site_type"], inp["site_size"], inp["site_xpos"], inp["site_xmat"], inp["pos"], inp["geom"]))
      found.setdefault(name, []).append(nmatch)
      if prm[1] == truth.MAXFORCE:  # a condition of the comparison, not a skip: rounding must not be able to reorder the matches
        kept = truth.matches(int(mjm.sensor_objtype[i]), int(mjm.sensor_objid[i]), int(mjm.sensor_reftype[i]), int(mjm.sensor_refid[i]), inp["geom_bodyid"], inp["body_parentid"],
                             inp["site_type"], inp["site_size"], inp["site_xpos"], inp["site_xmat"], inp["pos"], inp["geom"])[:maxmatch]
        assert _separated(np.sort(truth.criteria(truth.MAXFORCE, kept, inp["dist"], inp["force"]))), (name, w)
      if prm[1] == truth.NETFORCE:
        wrench, centroid = np.isin(lab, ("force", "torque")), lab == "pos"
        errs = (conftest.relerr(got[wrench], want[wrench]) if np.abs(want[wrench]).max(initial=0) > 0 else float(np.abs(got[wrench]).max(initial=0)),
                conftest.relerr(got[centroid], want[centroid]) if np.abs(want[centroid]).max(initial=0) > 0 else float(np.abs(got[centroid]).max(initial=0)))
        if report is not None:
          report.append((name, w, "netforce", errs))
        assert max(errs) <= 1e-5, (name, w, errs, got, want)
        exact = ~(wrench | centroid)
      else:
        ft = np.isin(lab, ("force", "torque"))
        for field in ("force", "torque"):
          sel = lab == field
          if sel.any():
            err = conftest.relerr(got[sel], want[sel]) if np.abs(want[sel]).max() > 0 else float(np.abs(got[sel]).max())
            if report is not None:
              report.append((name, w, field, err))
            assert err <= 1e-6, (name, w, field, err, got[sel], want[sel])
        zero = want == 0  # (zero-filled slots and exact zeros of the forces: bitwise as well)
        exact = ~ft | zero
      assert (_bits(got[exact]) == _bits(want[exact])).all(), (name, w, got, want)
  return found


def _run_scene_a(cone):
  mjm = mjw.mjcf.from_xml_string(_scene_a(cone))
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=NWORLD_A, nconmax=16, njmax=64)
  _start_a(mjm, m, d)
  for _ in range(40):
    mjw.step(m, d)
  mjw.forward(m, d)
  return mjm, m, d


@pytest.mark.gpu
@pytest.mark.parametrize("cone", ["pyramidal", "elliptic"])
def test_gpu_scene_a(cone):
  mjm, m, d = _run_scene_a(cone)
  assert m.nsensor_contact == 25 and (d.overflow.numpy() == 0).all()
  report = []
  found = _check_against_truth(mjm, m, d, report=report)
  print(cone, {k: v for k, v in found.items()}, max((np.max(r[3]) for r in report), default=0.0))
  # the scene does what the cases need: every class of sensor matched somewhere, and the lifted sphere matched nothing
  assert found["s1"] == [1, 1, 1, 0, 1] and found["net_s1"][3] == 0 and min(found["any"]) >= 7 and found["any"][3] == min(found["any"])
  assert min(found["slab_all"]) == 4 and min(found["chain"]) >= 1 and min(found["zone"]) == 1 and min(found["under4"]) == 1 and found["strong3"] == [3, 3, 3, 2, 3]
  sd, names = d.sensordata.numpy(), mjm.sensor_names
  a = lambda name: slice(mjm.sensor_adr[names.index(name)], mjm.sensor_adr[names.index(name)] + mjm.sensor_dim[names.index(name)])
  assert (sd[3, a("s1_floor")] == 0).all() and sd[3, a("net_s1")].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
  # both orders of the pair: the same contact seen from either side
  x, y = sd[0, a("s1_floor")], sd[0, a("floor_s1")]
  assert x[0] == y[0] == 1 and x[3] == -y[3] and (x[4:7] == -y[4:7]).all() and (x[1:3] == y[1:3]).all() and x[6] * y[6] < 0
  assert (sd[:, a("jp")][:, 0] == d.qpos.numpy()[:, 28]).all() and (sd[:, a("t")][:, 0] == d.time.numpy()).all()  # (k_sensor's own slots are untouched)
  # strongest first: masses 4, 2, 1
  assert (np.diff(sd[:, a("strong3")].reshape(NWORLD_A, 3, 5)[:, :, 1], axis=1) < 0).all()


@pytest.mark.gpu
def test_gpu_scene_a_paths():
  mjm, m, d = _run_scene_a("pyramidal")
  ref_sd = d.sensordata.numpy().copy()
  # sensor_acc alone rewrites the contact sensors' slots
  con = np.concatenate([np.arange(mjm.sensor_adr[i], mjm.sensor_adr[i] + mjm.sensor_dim[i]) for i in np.flatnonzero(mjm.sensor_type == 42)])
  d.sensordata.assign(np.full_like(ref_sd, 7.0))
  mjw.sensor_acc(m, d)
  out = d.sensordata.numpy()
  assert (_bits(out[:, con]) == _bits(ref_sd[:, con])).all() and (np.delete(out, con, axis=1) == 7.0).all()
  # a captured step graph against eager stepping, and two runs of each against each other
  state = {k: getattr(d, k).numpy().copy() for k in ("qpos", "qvel", "qacc_warmstart", "time")}

  def run(graph):
    for k, v in state.items():
      getattr(d, k).assign(v)
    g = mjw.StepGraph(m, d) if graph else None
    out = []
    for _ in range(5):
      g.launch() if graph else mjw.step(m, d)
      out.append(d.sensordata.numpy().copy())
    return np.stack(out)

  eager, eager2, graph, graph2 = run(False), run(False), run(True), run(True)
  assert (_bits(eager) == _bits(eager2)).all() and (_bits(graph) == _bits(graph2)).all() and (_bits(eager) == _bits(graph)).all()
  assert np.abs(eager[:, :, con]).max() > 0
  # sensors disabled: sensordata is left alone
  mjm2 = mjw.mjcf.from_xml_string(_scene_a("pyramidal", '<flag sensor="disable"/>'))
  m2 = mjw.put_model(mjm2)
  d2 = mjw.make_data(mjm2, nworld=NWORLD_A, nconmax=16, njmax=64)
  d2.sensordata.assign(np.full(d2.sensordata.shape, 7.0, dtype=np.float32))
  mjw.step(m2, d2)
  mjw.forward(m2, d2)
  assert (d2.sensordata.numpy() == 7.0).all()


@pytest.mark.gpu
def test_gpu_contact_sensor_alone_gets_the_launch():
  """No other acceleration-stage sensor in the model: the stage is still launched for the contact sensor."""
  xml = """<mujoco><worldbody><geom name="floor" type="plane" size="5 5 .1"/>
    <body pos="0 0 .09"><freejoint/><geom name="ball" type="sphere" size=".1"/></body></worldbody>
    <sensor><contact name="c" geom1="ball" geom2="floor" data="found force dist"/></sensor></mujoco>"""
  mjm = mjw.mjcf.from_xml_string(xml)
  m = mjw.put_model(mjm)
  assert m.nsensor_acc == 1 and m.nsensor_contact == 1
  d = mjw.make_data(mjm, nworld=3, nconmax=8, njmax=16)
  for _ in range(3):
    mjw.step(m, d)
  sd = d.sensordata.numpy()
  assert (sd[:, 0] == 1).all() and (sd[:, 1] > 0).all() and (sd[:, 4] < 0).all()
  mjw.forward(m, d)
  _check_against_truth(mjm, m, d)


# Scene B: one free body carrying a 10 x 7 grid of small frictionless spheres at one height: 70 contacts with nv = 6
def _scene_b(maxmatch=None):
  balls = "".join(f'<geom name="g{i}_{j}" type="sphere" size=".02" pos="{0.05 * (i - 4.5):.3f} {0.05 * (j - 3):.3f} 0" condim="1" mass=".05"/>' for i in range(10) for j in range(7))
  custom = f'<custom><numeric name="contact_sensor_maxmatch" data="{maxmatch}"/></custom>' if maxmatch else ""
  return f"""
<mujoco>{custom}
  <worldbody>
    <geom name="floor" type="plane" size="5 5 .1" condim="1"/>
    <body name="raft" pos="0 0 .016"><freejoint/>{balls}<site name="patch" type="box" pos="-.15 -.1 -.02" size=".09 .06 .03"/></body>
  </worldbody>
  <sensor>
    <contact name="last" geom1="g9_6" data="found force pos"/>
    <contact name="all" num="70" data="found dist pos"/>
    <contact name="near" num="4" data="found dist" reduce="mindist"/>
    <contact name="net_patch" site="patch" data="found force torque pos" reduce="netforce"/>
  </sensor>
</mujoco>"""


def _run_scene_b(maxmatch=None):
  mjm = mjw.mjcf.from_xml_string(_scene_b(maxmatch))
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=2, nconmax=80, njmax=96)
  q = d.qpos.numpy()
  q[0, 3:7] = [np.cos(0.004), 0, np.sin(0.004), 0]  # tilted by 8 mrad about y / x: every sphere still touches, at its own depth
  q[1, 3:7] = [np.cos(0.004), -np.sin(0.004), 0, 0]
  d.qpos.assign(q)
  mjw.forward(m, d)
  return mjm, m, d


@pytest.mark.gpu
def test_gpu_scene_b_beyond_one_chunk():
  mjm, m, d = _run_scene_b()
  assert d.ws_ncon.numpy().tolist() == [70, 70]
  found = _check_against_truth(mjm, m, d)
  assert found["last"] == [1, 1] and found["all"] == [70, 70] and found["net_patch"] == [12, 12]
  sd, adr = d.sensordata.numpy(), mjm.sensor_adr
  last_rec = [int(np.flatnonzero(d.contact.geom.numpy()[d.ws_conadr.numpy()[w] :][:70, 1] == mjm.geom_names.index("g9_6"))[0]) for w in range(2)]
  assert min(last_rec) >= 64  # (its record sits in the second chunk of 64)
  assert (sd[:, adr[0]] == 1).all() and (sd[:, adr[0] + 1] > 0).all()
  slots = sd[:, adr[1] : adr[1] + 350].reshape(2, 70, 5)
  assert (slots[:, :64, 0] == 64).all() and (slots[:, 64:] == 0).all()
  for w in range(2):
    o = int(d.ws_conadr.numpy()[w])
    assert (_bits(slots[w, :64, 1]) == _bits(d.contact.dist.numpy()[o : o + 64])).all()  # contact order
  assert ((d.overflow.numpy() & int(mjw.OverflowType.CONTACT_MATCH)) != 0).all()


@pytest.mark.gpu
def test_gpu_scene_b_maxmatch_two():
  mjm, m, d = _run_scene_b(maxmatch=2)
  assert m.opt.contact_sensor_maxmatch == 2
  _check_against_truth(mjm, m, d, maxmatch=2)
  sd, i = d.sensordata.numpy(), mjm.sensor_names.index("near")
  for w in range(2):
    o = int(d.ws_conadr.numpy()[w])
    dist = d.contact.dist.numpy()[o : o + 70]
    got = sd[w, mjm.sensor_adr[i] : mjm.sensor_adr[i] + 8].reshape(4, 2)
    assert got[:2, 1].tolist() == sorted(dist[:2].tolist()) and (got[:2, 0] == 2).all() and (got[2:] == 0).all()
    assert dist.min() < dist[:2].min()  # (the two nearest of all would have been others)
  assert ((d.overflow.numpy() & int(mjw.OverflowType.CONTACT_MATCH)) != 0).all()
