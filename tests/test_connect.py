"""Connect equality constraints: the loader and put_model on the CPU, the rows / solve / rollout on the GPU against tests/connect_truth.py.

Tolerances of the GPU tests are those tests/test_gpu.py applies to the same fields against the oracle: SMOOTH 2e-5 (efc_J), EFC 5e-4 (efc_D /
aref / pos / vel), SOLVE 2e-3 (qacc; tests/test_pgs.py uses the same for PGS), 1e-5 for qpos of a trajectory -- all max-norm relative
(conftest.relerr).  None had to be widened.
"""

import copy
import sys

import numpy as np
import pytest

import conftest
import mujoco_warp_amd as mjw
from conftest import relerr
from mujoco_warp_amd import _npmath as nm
from mujoco_warp_amd import io as mjio
from mujoco_warp_amd import types

sys.path.insert(0, conftest.GOLDEN_DIR)
import connect_truth as ct  # noqa: E402
import make_host_tables  # noqa: E402

SMOOTH, EFC, SOLVE = 2e-5, 5e-4, 2e-3
NOCOL = 'contype="0" conaffinity="0"'

# a four-bar linkage in the x-z plane: crank a, coupler b, rocker c, closed by one connect (coupler tip to rocker tip); no damping, no contacts
FOURBAR_XML = f"""
<mujoco>
  <option timestep="0.002" tolerance="1e-10" iterations="200"/>
  <worldbody>
    <body name="a" pos="0 0 1">
      <joint name="ja" type="hinge" axis="0 1 0"/>
      <geom type="capsule" fromto="0 0 0 0 0 -0.3" size="0.02" {NOCOL}/>
      <body name="b" pos="0 0 -0.3">
        <joint name="jb" type="hinge" axis="0 1 0"/>
        <geom type="capsule" fromto="0 0 0 0.4 0 0" size="0.02" {NOCOL}/>
      </body>
    </body>
    <body name="c" pos="0.4 0 1">
      <joint name="jc" type="hinge" axis="0 1 0"/>
      <geom type="capsule" fromto="0 0 0 0 0 -0.3" size="0.025" {NOCOL}/>
    </body>
  </worldbody>
  <equality>
    <connect name="close" body1="b" body2="c" anchor="0.4 0 0"/>
  </equality>
</mujoco>
"""
FOURBAR_Q = np.array([0.5, -0.5, 0.5])  # (a parallelogram stays closed when crank and rocker turn together and the coupler turns back)

# one free body hung from the world by a point off its centre (body2 absent); the geom is centred on the body frame: com = frame origin
HANG_XML = f"""
<mujoco>
  <option timestep="0.002" tolerance="1e-10" iterations="200"/>
  <worldbody>
    <body name="ball" pos="0 0 1">
      <freejoint/>
      <geom type="box" size="0.1 0.06 0.04" density="800" {NOCOL}/>
    </body>
  </worldbody>
  <equality>
    <connect name="hang" body1="ball" anchor="0.1 0.02 0.2"/>
  </equality>
</mujoco>
"""

# one tree with two branches off a hinged base (a ball joint on one, hinge + slide on the other), a free box, a mocap body; connects: the two
# branch tips (one tree, shared ancestors), box to branch tip (two trees), box to world, mocap to box, and the site form
MIXED_XML = f"""
<mujoco>
  <option timestep="0.002"/>
  <default><default class="stiff"><equality solref="0.01 0.8" solimp="0.8 0.9 0.01 0.4 3"/></default></default>
  <worldbody>
    <body name="base" pos="0 0 1" quat="0.9 0.1 0.2 0.3">
      <joint name="jbase" type="hinge" axis="0 1 0"/>
      <geom type="box" size="0.1 0.1 0.05" {NOCOL}/>
      <body name="arma" pos="0.2 0 0" quat="0.7 0.1 -0.6 0.2">
        <joint name="ball" type="ball"/>
        <geom type="capsule" fromto="0 0 0 0.3 0 0" size="0.02" {NOCOL}/>
      </body>
      <body name="armb" pos="-0.2 0 0">
        <joint name="jb1" type="hinge" axis="1 0 0"/>
        <geom type="capsule" fromto="0 0 0 0 0.3 0" size="0.02" {NOCOL}/>
        <body name="armb2" pos="0 0.3 0" quat="0.8 0.3 0.1 -0.2">
          <joint name="jb2" type="slide" axis="0 0 1"/>
          <geom type="sphere" size="0.05" {NOCOL}/>
          <site name="sa" pos="0.03 0.02 0.01"/>
        </body>
      </body>
    </body>
    <body name="box" pos="0.5 0.4 1.2" quat="0.6 -0.3 0.5 0.2">
      <freejoint/>
      <geom type="box" size="0.08 0.06 0.04" {NOCOL}/>
      <site name="sb" pos="-0.05 0.01 0.02"/>
    </body>
    <body name="target" mocap="true" pos="0.6 0.5 1.3" quat="0.9 0.2 -0.1 0.1">
      <geom type="sphere" size="0.02" {NOCOL}/>
    </body>
  </worldbody>
  <equality>
    <connect name="tips" body1="arma" body2="armb2" anchor="0.3 0 0"/>
    <connect name="box_arm" class="stiff" body1="box" body2="arma" anchor="0.08 0 0"/>
    <connect name="box_world" body1="box" anchor="0 0.06 0"/>
    <connect name="mocap_box" body1="target" body2="box" anchor="0.01 0.02 0.03" solref="0.03 1.2"/>
    <connect name="sites" site1="sa" site2="sb"/>
  </equality>
</mujoco>
"""

# four pendula (four trees); joint couplings and connects interleaved in the document
INTERLEAVED_XML = f"""
<mujoco>
  <option timestep="0.002"/>
  <worldbody>
    {"".join(f'<body name="p{i}" pos="{0.3 * i} 0 1"><joint name="h{i}" type="hinge" axis="0 1 0"/><geom type="capsule" fromto="0 0 0 0 0 -0.4" size="0.02" {NOCOL}/></body>' for i in range(4))}
  </worldbody>
  <equality>
    <joint name="e0" joint1="h0" joint2="h1" polycoef="0.1 0.9 0.2 0 0"/>
    <connect name="e1" body1="p0" body2="p2" anchor="0 0 -0.4"/>
    <joint name="e2" joint1="h3"/>
    <connect name="e3" body1="p1" anchor="0 0 -0.2"/>
  </equality>
</mujoco>
"""


def chain_xml(n, nchain=1, connect=""):
  """nchain chains of n hinged links each (axes alternate, so the chains leave the plane), hanging from the world; `connect`: the <equality> body."""
  def links(c, i):
    if i == n:
      return ""
    axis = ("0 1 0", "1 0 0", "0 0 1")[i % 3]
    return (f'<body name="c{c}_{i}" pos="{0.5 * c if i == 0 else 0.03} 0 {1.5 if i == 0 else -0.05}"><joint type="hinge" axis="{axis}"/>'
            f'<geom type="capsule" fromto="0 0 0 0.03 0 -0.05" size="0.01" {NOCOL}/>{links(c, i + 1)}</body>')
  return (f'<mujoco><option timestep="0.002" solver="Newton"/><worldbody>{"".join(links(c, 0) for c in range(nchain))}</worldbody>'
          f'<equality>{connect}</equality></mujoco>')


def _state(mjm, seed, vel=1.0, off=0.05):
  """A state off qpos0 (so the anchors are violated) with non-zero velocities (so Jdot qvel matters)."""
  rng = np.random.default_rng(seed)
  qpos = ct.integrate_pos(mjm, mjm.qpos0, off * rng.standard_normal(mjm.nv))
  return qpos, vel * rng.standard_normal(mjm.nv)


# ------------------------------------------------------------------------------------------------------------------------ CPU: the truth
def test_truth_fd_jacobian_matches_an_analytic_ball_joint():
  """A point at r (body frame) on a body held by a ball joint at the origin: p = R r, and its Jacobian along the body-frame rotation vector is
  -R [r]x, in closed form.  The finite differences agree, their error is flat over a range of steps (the plateau the module's steps sit in),
  and Jdot qvel equals the centripetal term R (w x (w x r))."""
  mjm = mjw.mjcf.from_xml_string(f'<mujoco><worldbody><body name="b"><joint type="ball"/><geom size="0.1" {NOCOL}/></body></worldbody>'
                                 '<equality><connect body1="b" anchor="0.3 -0.2 0.5"/></equality></mujoco>')
  t = ct.Truth(mjm)
  r = np.array([0.3, -0.2, 0.5])
  q = nm.quat_normalize([0.7, 0.2, -0.5, 0.4])
  w = np.array([0.8, -1.1, 0.6])
  R = nm.quat_to_mat(q)
  skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
  exact = -R @ skew(r)
  hs = [10.0 ** k for k in range(-9, -1)]
  err, _ = ct.fd_plateau(lambda h: t.jac(q, 0, h), hs)
  assert np.abs(t.jac(q, 0) - exact).max() < 1e-9
  flat = [h for h, e in zip(hs, err) if e < 1e-9]
  assert min(flat) <= ct.H_J / 10 and max(flat) >= ct.H_J * 10, (flat, err)  # H_J sits inside the plateau, a decade from either edge
  exact_dot = R @ np.cross(w, np.cross(w, r))
  assert np.abs(t.jac_dot_vel(q, w, 0) - exact_dot).max() < 1e-6
  hs = [1e-6, 3e-6, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2]
  err, _ = ct.fd_plateau(lambda h: t.jac_dot_vel(q, w, 0, h), hs)
  flat = [h for h, e in zip(hs, err) if e < 1e-6]
  assert min(flat) < ct.H_FLOW / 2 and max(flat) > ct.H_FLOW * 2, (flat, err)  # (a narrower plateau: a difference of differences)


def test_truth_closed_form_holds_the_anchor():
  """The closed-form qacc of the hanging body drives the anchor's acceleration to aref: J qacc + Jdot qvel = aref + Jdot qvel - force / D."""
  mjm = mjw.mjcf.from_xml_string(HANG_XML)
  t = ct.Truth(mjm)
  qpos, qvel = _state(mjm, 3)
  r = t.rows(qpos, qvel)
  qacc = t.qacc(qpos, qvel, rows=r)
  M, qacc_smooth = t.smooth(qpos, qvel)[:2]
  force = -r["D"] * (r["J"] @ qacc - r["aref"])
  assert np.abs(M @ (qacc - qacc_smooth) - r["J"].T @ force).max() < 1e-9 * np.abs(force).max()


# ------------------------------------------------------------------------------------------------------------------------ CPU: the loader
def test_loader_body_and_site_forms():
  mjm = mjw.mjcf.from_xml_string(MIXED_XML)
  assert mjm.neq == 5 and mjm.eq_names == ["tips", "box_arm", "box_world", "mocap_box", "sites"]
  assert (mjm.eq_type == int(types.EqType.CONNECT)).all()
  assert mjm.eq_objtype.tolist() == [1, 1, 1, 1, 6]
  names = mjm.body_names
  assert mjm.eq_obj1id.tolist()[:4] == [names.index(n) for n in ("arma", "box", "box", "target")]
  assert mjm.eq_obj2id.tolist()[:4] == [names.index("armb2"), names.index("arma"), 0, names.index("box")]  # body2 absent: the world
  assert (mjm.eq_obj1id[4], mjm.eq_obj2id[4]) == (0, 1) and (mjm.eq_data[4] == 0).all()
  # anchor2: the same world point at qpos0, in body 2's (rotated, offset) frame -- the gap at qpos0 is zero
  t = ct.Truth(mjm)
  for e in range(4):
    assert (mjm.eq_data[e, 6:] == 0).all()
    assert np.abs(t.gap(mjm.qpos0, e)).max() < 1e-12
  np.testing.assert_allclose(mjm.eq_data[0, :3], [0.3, 0, 0])
  np.testing.assert_allclose(mjm.eq_data[2, 3:6], mjm.body_pos[names.index("box")] + nm.rot_vec_quat([0, 0.06, 0], nm.quat_normalize(mjm.body_quat[names.index("box")])))
  assert not np.allclose(mjm.eq_data[0, 3:6], mjm.eq_data[0, :3])
  # defaults class and explicit attributes
  np.testing.assert_allclose(mjm.eq_solref, [[0.02, 1], [0.01, 0.8], [0.02, 1], [0.03, 1.2], [0.02, 1]])
  np.testing.assert_allclose(mjm.eq_solimp[1], [0.8, 0.9, 0.01, 0.4, 3])
  np.testing.assert_allclose(mjm.eq_solimp[0], [0.9, 0.95, 0.001, 0.5, 2])


def test_loader_active_and_document_order():
  mjm = mjw.mjcf.from_xml_string(INTERLEAVED_XML.replace('name="e3"', 'name="e3" active="false"'))
  assert mjm.eq_type.tolist() == [2, 0, 2, 0] and mjm.eq_objtype.tolist() == [3, 1, 3, 1]
  assert mjm.eq_names == ["e0", "e1", "e2", "e3"] and mjm.eq_active0.tolist() == [1, 1, 1, 0]
  assert mjm.eq_obj1id.tolist() == [0, 1, 3, 2] and mjm.eq_obj2id.tolist() == [1, 3, -1, 0]
  np.testing.assert_allclose(mjm.eq_data[0, :5], [0.1, 0.9, 0.2, 0, 0])


@pytest.mark.parametrize("eq,exc,match", [
  ('<connect body1="a" anchor="0 0 0" site1="s" site2="s"/>', ValueError, "either"),
  ('<connect/>', ValueError, "either"),
  ('<connect body1="nobody" anchor="0 0 0"/>', ValueError, "nobody"),
  ('<connect body1="a" body2="ghost" anchor="0 0 0"/>', ValueError, "ghost"),
  ('<connect site1="s" site2="nosite"/>', ValueError, "nosite"),
  ('<connect site1="s"/>', ValueError, "site2"),
  ('<connect body1="a"/>', ValueError, "anchor"),
  ('<joint joint1="nojoint"/>', ValueError, "nojoint"),
  ('<weld body1="a"/>', NotImplementedError, "weld"),
  ('<tendon tendon1="t"/>', NotImplementedError, "tendon"),
  ('<flex flex="f"/>', NotImplementedError, "flex"),
  ('<flexvert flex="f"/>', NotImplementedError, "flexvert"),
  ('<flexstrain flex="f"/>', NotImplementedError, "flexstrain"),
])
def test_loader_errors(eq, exc, match):
  with pytest.raises(exc, match=match):
    mjw.mjcf.from_xml_string(f'<mujoco><worldbody><body name="a"><joint name="j"/><geom size=".1"/><site name="s"/></body></worldbody><equality>{eq}</equality></mujoco>')


# ------------------------------------------------------------------------------------------------------------------------ CPU: put_model
def test_put_model_accepts_connects_and_refuses_weld_and_sleep():
  for xml in (FOURBAR_XML, HANG_XML, MIXED_XML, INTERLEAVED_XML):
    mjm = mjw.mjcf.from_xml_string(xml)
    m = mjw.put_model(mjm)
    assert m.has_connect == 1 and io_scalar(m, "has_connect") == 1
    assert m.eq_type.numpy().tolist() == mjm.eq_type.tolist() and m.eq_objtype.numpy().tolist() == mjm.eq_objtype.tolist()
    assert m.eq_kind.numpy().tolist() == [mjm.eq_type.tolist(), mjm.eq_objtype.tolist()]  # (what the library reads: both, as one table)
  assert mjw.put_model(mjw.mjcf.load_xml(conftest.PANDA_XML)).has_connect == 0
  mjm = mjw.mjcf.from_xml_string(INTERLEAVED_XML)
  weld = copy.deepcopy(mjm)
  weld.eq_type[1] = int(types.EqType.WELD)
  with pytest.raises(NotImplementedError, match="'e1'.*weld"):
    mjw.put_model(weld)
  sleepy = copy.deepcopy(mjm)
  sleepy.opt.enableflags |= int(types.EnableBit.SLEEP)
  with pytest.raises(NotImplementedError, match="'e1'.*connect.*sleep"):
    mjw.put_model(sleepy)
  bad = copy.deepcopy(mjm)
  bad.eq_obj2id[1] = 17
  with pytest.raises(ValueError, match="equality 1"):
    mjw.put_model(bad)


def io_scalar(m, name):
  return getattr(mjio.c_model(m), name)


def test_put_model_without_eq_objtype():
  """A host model that does not carry eq_objtype (a duck-typed MjModel): JOINT for joint couplings, BODY for connects."""
  mjm = mjw.mjcf.from_xml_string(INTERLEAVED_XML)
  m = mjw.put_model(make_host_tables.Hidden(mjm, {"eq_objtype", "eq_names"}))
  assert m.eq_objtype.numpy().tolist() == [3, 1, 3, 1] and m.has_connect == 1
  panda = mjw.mjcf.load_xml(conftest.PANDA_XML)
  m = mjw.put_model(make_host_tables.Hidden(panda, {"eq_objtype", "eq_names"}))
  assert (m.eq_objtype.numpy() == 3).all() and m.eq_objtype.shape == (panda.neq,)


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _device(mjm, states, nworld=3, njmax=32, batch_sizes=None, mocap=None):
  """(Model, Data) with world w in states[w % len(states)] = (qpos, qvel)."""
  m = mjw.put_model(mjm, batch_sizes=batch_sizes)
  d = mjw.make_data(mjm, nworld=nworld, nconmax=8, njmax=njmax)
  d.qpos.assign(np.array([states[w % len(states)][0] for w in range(nworld)], dtype=np.float32))
  d.qvel.assign(np.array([states[w % len(states)][1] for w in range(nworld)], dtype=np.float32))
  if mocap is not None:
    d.mocap_pos.assign(np.tile(np.asarray(mocap[0], dtype=np.float32), (nworld, 1, 1)))
    d.mocap_quat.assign(np.tile(np.asarray(mocap[1], dtype=np.float32), (nworld, 1, 1)))
  return m, d


def _f32_state(state):
  """The state as the device holds it (the truth is evaluated at the float32 values, not at their float64 origin)."""
  return state[0].astype(np.float32).astype(np.float64), state[1].astype(np.float32).astype(np.float64)


def _check_rows(d, w, r, nv):
  ne = len(r["id"])
  assert (int(d.ne.numpy()[w]), int(d.nefc.numpy()[w])) == (ne, ne)
  np.testing.assert_array_equal(d.efc.type.numpy()[w, :ne], int(types.ConstraintType.EQUALITY))
  np.testing.assert_array_equal(d.efc.id.numpy()[w, :ne], r["id"])
  J = d.efc.J.numpy()[w, :ne]
  assert relerr(J[:, :nv], r["J"]) <= SMOOTH, relerr(J[:, :nv], r["J"])
  assert (J[:, nv:] == 0).all()
  for name in ("pos", "vel", "D", "aref"):
    got = getattr(d.efc, name).numpy()[w, :ne]
    assert relerr(got, r[name]) <= EFC, (name, relerr(got, r[name]))


_ROW_MODELS = {
  "mixed": lambda: MIXED_XML,
  "interleaved": lambda: INTERLEAVED_XML,
  "fourbar": lambda: FOURBAR_XML,
  # the lane-group widths launch_constraint dispatches on (mjhip.hip lanes64: 32 lanes up to 32 dofs and bodies, 64 beyond): nv just below, at
  # and just above 32, and around 64, where the 64-lane dof loop takes a second trip
  **{f"chain{n}": (lambda n=n: chain_xml(n, 1, f'<connect body1="c0_{n - 1}" anchor="0.03 0 -0.05"/><connect body1="c0_{n // 2}" body2="c0_{n - 2}" anchor="0 0.01 0"/>'))
     for n in (31, 32, 33, 63, 65)},
}


def _rows_case(name):
  mjm = mjw.mjcf.from_xml_string(_ROW_MODELS[name]())
  small = mjm.nv <= 16
  states = [_f32_state(_state(mjm, 10 + k, off=0.05 if small else 0.02)) for k in range(3 if small else 1)]
  mocap = None
  if mjm.nmocap:
    mocap = (np.array([[0.62, 0.47, 1.33]]), np.array([nm.quat_normalize([0.8, 0.3, -0.2, 0.1])]))
  m, d = _device(mjm, states, njmax=32, mocap=mocap)
  assert io_scalar(m, "heavy_colliders") == 0  # (heavy colliders would pin every kernel to 32 lanes: the chains are meant to reach 64)
  mjw.forward(m, d)
  return mjm, m, d, states, mocap


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_ROW_MODELS))
def test_rows_match_truth(name):
  mjm, m, d, states, mocap = _rows_case(name)
  t = ct.Truth(mjm)
  mocap64 = None if mocap is None else (mocap[0].astype(np.float32).astype(np.float64), mocap[1].astype(np.float32).astype(np.float64))
  truth = [t.rows(*s, mocap=mocap64) for s in states]
  assert (d.overflow.numpy() == 0).all()
  for w in range(3):
    _check_rows(d, w, truth[w % len(states)], mjm.nv)


@pytest.mark.gpu
def test_rows_are_bitwise_repeatable():
  a, b = _rows_case("mixed")[2], _rows_case("mixed")[2]
  assert (a.efc.J.numpy() == b.efc.J.numpy()).all() and (a.efc.aref.numpy() == b.efc.aref.numpy()).all()
  a, b = _rows_case("chain65")[2], _rows_case("chain65")[2]
  assert (a.efc.J.numpy() == b.efc.J.numpy()).all() and (a.efc.aref.numpy() == b.efc.aref.numpy()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["NEWTON", "CG", "PGS"])
@pytest.mark.parametrize("scene", ["fourbar", "hang"])
def test_qacc_matches_closed_form(scene, solver):
  mjm = mjw.mjcf.from_xml_string(FOURBAR_XML if scene == "fourbar" else HANG_XML)
  mjm.opt.solver = int(getattr(mjw.SolverType, solver))
  states = [_f32_state(_state(mjm, 20 + k, vel=0.7, off=0.03)) for k in range(3)]
  if scene == "fourbar":
    states = [(ct.integrate_pos(mjm, FOURBAR_Q, s[0] - mjm.qpos0).astype(np.float32).astype(np.float64), s[1]) for s in states]
  m, d = _device(mjm, states)
  mjw.forward(m, d)
  t = ct.Truth(mjm)
  for w in range(3):
    want = t.qacc(*states[w])
    got = d.qacc.numpy()[w]
    print(scene, solver, w, relerr(got, want))
    assert relerr(got, want) <= SOLVE, (w, relerr(got, want))
  assert (d.overflow.numpy() == 0).all()


def _truth_rollout(t, qpos, qvel, nstep, rk4):
  """Hinges only: semi-implicit Euler (no damping: no implicit term) or the classical RK4 in numpy, the acceleration from the closed form."""
  h = float(t.mjm.opt.timestep)
  q, v = np.array(qpos, dtype=np.float64), np.array(qvel, dtype=np.float64)
  for _ in range(nstep):
    if not rk4:
      v = v + h * t.qacc(q, v)
      q = q + h * v
    else:
      k1v, k1a = v, t.qacc(q, v)
      k2v, k2a = v + 0.5 * h * k1a, t.qacc(q + 0.5 * h * k1v, v + 0.5 * h * k1a)
      k3v, k3a = v + 0.5 * h * k2a, t.qacc(q + 0.5 * h * k2v, v + 0.5 * h * k2a)
      k4v, k4a = v + h * k3a, t.qacc(q + h * k3v, v + h * k3a)
      q = q + h / 6.0 * (k1v + 2 * k2v + 2 * k3v + k4v)
      v = v + h / 6.0 * (k1a + 2 * k2a + 2 * k3a + k4a)
  return q, v


@pytest.fixture(scope="module")
def fourbar_rollouts():
  """The float64 rollouts of the four-bar (50 steps, Euler and RK4), computed once."""
  mjm = mjw.mjcf.from_xml_string(FOURBAR_XML)
  t = ct.Truth(mjm)
  start = _f32_state((FOURBAR_Q, np.array([0.3, -0.3, 0.3])))
  return mjm, start, {rk4: _truth_rollout(t, *start, 50, rk4) for rk4 in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["euler", "graph", "rk4"])
def test_fourbar_rollout(fourbar_rollouts, mode):
  mjm, start, truth = fourbar_rollouts
  mjm = copy.deepcopy(mjm)
  mjm.opt.integrator = int(mjw.IntegratorType.RK4 if mode == "rk4" else mjw.IntegratorType.EULER)
  m, d = _device(mjm, [start])
  if mode == "graph":
    g = mjw.StepGraph(m, d)
    d.qpos.assign(np.tile(start[0].astype(np.float32), (3, 1)))  # (building the graph took a warm-up step)
    d.qvel.assign(np.tile(start[1].astype(np.float32), (3, 1)))
    d.time.assign(np.zeros(3, dtype=np.float32))
    for _ in range(50):
      g.launch()
  else:
    for _ in range(50):
      mjw.step(m, d)
  q, v = truth[mode == "rk4"]
  got = d.qpos.numpy()
  print(mode, relerr(got[0], q), relerr(d.qvel.numpy()[0], v))
  assert (got == got[0]).all()
  assert relerr(got[0], q) <= 1e-5, relerr(got[0], q)
  assert np.abs(q - start[0]).max() > 0.05  # (the linkage moved)
  assert (d.overflow.numpy() == 0).all()


@pytest.mark.gpu
def test_eq_active_per_world():
  """World 1 has the connect switched off on the device: it is the stripped model there (the oracle's forward), the others match the truth."""
  mjm = mjw.mjcf.from_xml_string(FOURBAR_XML)
  state = _f32_state((FOURBAR_Q + 0.02, np.array([0.4, -0.2, 0.1])))
  m, d = _device(mjm, [state])
  active = np.ones((3, 1), dtype=np.int32)
  active[1] = 0
  d.eq_active.assign(active)
  mjw.forward(m, d)
  t = ct.Truth(mjm)
  r = t.rows(*state)
  for w in (0, 2):
    _check_rows(d, w, r, mjm.nv)
    assert relerr(d.qacc.numpy()[w], t.qacc(*state, rows=r)) <= SOLVE
  assert (int(d.ne.numpy()[1]), int(d.nefc.numpy()[1])) == (0, 0)
  t.smooth(*state)  # (one oracle forward of the stripped model at the state)
  assert relerr(d.qacc.numpy()[1], t.sim.qacc) <= SOLVE
  # DisableBit.EQUALITY switches the connects off like the joint couplings: every world is the stripped model
  off = copy.deepcopy(mjm)
  off.opt.disableflags |= int(mjw.DisableBit.EQUALITY)
  m, d = _device(off, [state])
  mjw.forward(m, d)
  assert (d.ne.numpy() == 0).all() and (d.nefc.numpy() == 0).all()
  for w in range(3):
    assert relerr(d.qacc.numpy()[w], t.sim.qacc) <= SOLVE


@pytest.mark.gpu
def test_per_world_eq_data():
  mjm = mjw.mjcf.from_xml_string(HANG_XML)
  state = _f32_state(_state(mjm, 31))
  m, d = _device(mjm, [state], batch_sizes={"eq_data": 3})
  data = np.tile(mjm.eq_data[None], (3, 1, 1))
  data[1, 0, :3] = [-0.05, 0.1, 0.15]
  data[2, 0, 3:6] = [0.02, -0.03, 1.25]
  m.eq_data.assign(data.astype(np.float32))
  mjw.forward(m, d)
  t = ct.Truth(mjm)
  for w in range(3):
    _check_rows(d, w, t.rows(*state, eq_data=data[w].astype(np.float32).astype(np.float64)), mjm.nv)
  assert not np.allclose(d.efc.pos.numpy()[0, :3], d.efc.pos.numpy()[1, :3])


@pytest.mark.gpu
def test_njmax_overflow_drops_the_whole_connect():
  """njmax = 5: the second connect (rows 3 .. 5) does not fit.  None of its rows is written -- rows 3 and 4 keep the marker --, it is not
  counted, the overflow flag is up, and the first connect's rows are those of the truth."""
  mjm = mjw.mjcf.from_xml_string(INTERLEAVED_XML.replace('<joint name="e0" joint1="h0" joint2="h1" polycoef="0.1 0.9 0.2 0 0"/>', "").replace('<joint name="e2" joint1="h3"/>', ""))
  assert mjm.eq_type.tolist() == [0, 0]
  state = _f32_state(_state(mjm, 41))
  m, d = _device(mjm, [state], njmax=5)
  marker = np.full((3, 5), -7.0, dtype=np.float32)
  for arr in (d.efc.D, d.efc.aref, d.efc.pos):
    arr.assign(marker)
  J0 = np.full(d.efc.J.shape, -7.0, dtype=np.float32)
  d.efc.J.assign(J0)
  mjw.fwd_position(m, d)
  t = ct.Truth(mjm)
  first = t.rows(*state, eq_active=[1, 0])
  for w in range(3):
    assert (int(d.ne.numpy()[w]), int(d.nefc.numpy()[w])) == (3, 3)
    assert int(d.overflow.numpy()[w]) & 1
    for name in ("pos", "vel", "D", "aref"):
      assert relerr(getattr(d.efc, name).numpy()[w, :3], first[name]) <= EFC, name
    assert relerr(d.efc.J.numpy()[w, :3, : mjm.nv], first["J"]) <= SMOOTH
    for arr in (d.efc.D, d.efc.aref, d.efc.pos):
      assert (arr.numpy()[w, 3:5] == -7.0).all()
    assert (d.efc.J.numpy()[w, 3:5] == -7.0).all()


@pytest.mark.gpu
def test_islands_join_connected_trees():
  """Three 33-hinge chains (nv 99: the per-island solve), chains 0 and 1 joined at their tips: two constraint islands, trees 0 and 1 in the
  first (66 dofs), tree 2 alone; qacc matches the closed form.  (The islands are k_tree_rows' -- Data.ws_nisland / ws_isl_dofadr /
  ws_isl_dofmap; `island()` is the sleep module's pass, and sleeping with a connect is refused.)"""
  mjm = mjw.mjcf.from_xml_string(chain_xml(33, 3, '<connect body1="c0_32" body2="c1_32" anchor="0.03 0 -0.05"/>'))
  assert mjm.nv == 99
  state = _f32_state(_state(mjm, 51, vel=0.5, off=0.02))
  m, d = _device(mjm, [state], njmax=16)
  assert m.tree_solve == 1
  mjw.forward(m, d)
  assert (d.ws_nisland.numpy() == 2).all()
  np.testing.assert_array_equal(d.ws_isl_dofadr.numpy()[:, :3], np.tile([0, 66, 99], (3, 1)))
  np.testing.assert_array_equal(d.ws_isl_dofmap.numpy(), np.tile(np.arange(99), (3, 1)))
  t = ct.Truth(mjm)
  want = t.qacc(*state)
  for w in range(3):
    assert relerr(d.qacc.numpy()[w], want) <= SOLVE, relerr(d.qacc.numpy()[w], want)


@pytest.mark.gpu
def test_cfrc_ext_is_newtons_second_law():
  """One free body connected to the world: the only external force besides gravity is the connect's, so cfrc_ext's force is m (a_com - g)
  (the geom is centred on the body frame: a_com = qacc[0:3]) and its torque, about the subtree com, is r x f with r from the com to the anchor."""
  mjm = mjw.mjcf.from_xml_string(HANG_XML)
  state = _f32_state(_state(mjm, 61, vel=0.8))
  m, d = _device(mjm, [state])
  mjw.forward(m, d)
  mjw.rne_postconstraint(m, d)
  mass, g = float(mjm.body_mass[1]), np.asarray(mjm.opt.gravity, dtype=np.float64)
  quat = nm.quat_normalize(state[0][3:7])
  anchor = state[0][:3] + nm.rot_vec_quat(mjm.eq_data[0, :3], quat)
  for w in range(3):
    f = mass * (d.qacc.numpy()[w, :3].astype(np.float64) - g)
    got = d.cfrc_ext.numpy()[w, 1]
    assert relerr(got[3:], f) <= SOLVE, (got[3:], f)
    assert relerr(got[:3], np.cross(anchor - state[0][:3], f)) <= SOLVE, (got[:3], np.cross(anchor - state[0][:3], f))
    assert np.abs(f).max() > 1.0
    assert (d.cfrc_ext.numpy()[w, 0] == 0).all()
