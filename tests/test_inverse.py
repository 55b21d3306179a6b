"""Inverse dynamics: inverse(), inv_constraint(), Data.qfrc_inverse, invdiscrete (Euler) -- against tests/inverse_truth.py.

The truth is the float64 oracle's forward pass (part A: the force that produces the oracle's qacc is the force that was applied), a numpy
evaluation of the force update off the solution (part B), the oracle's Euler step (part C) and tests/connect_truth.py's rows and closed-form
qacc of a four-bar with a connect (part D).  Bounds are
not chosen: every GPU bound is inverse_truth.GPU_MARGIN x the error of the float32 twin recorded in inverse_truth.TWIN, which the CPU tests
below re-evaluate.  efc_state is compared exactly, except on rows within the twin's own error of a zone boundary (at most 2 % per case).
"""

import copy
import types as pytypes

import numpy as np
import pytest

import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi
from mujoco_warp_amd import io as mjio
from mujoco_warp_amd import types
from tests import inverse_truth as it

A_MODELS = ("pendula", "free_bodies", "pile_pyramidal", "pile_elliptic", "humanoid", "panda", "humanoids3")
CHAINS = tuple(f"chain{n}" for n in it.CHAIN_NV) + (it.BIG_CHAIN,)  # (nv 130: the four-trip instantiation, the largest one)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_exports_and_schema():
  assert callable(mjw.inverse) and callable(mjw.inv_constraint)
  assert types.array_fields(types.Data)["qfrc_inverse"] == (("nworld", "nv"), "float32", False)
  assert types.array_fields(types.Data)["ws_inverse"] == ((2, "nworld", "nv"), "float32", False)  # (invdiscrete's scratch: make_data's, not inverse()'s)
  assert "qfrc_inverse" in mjio._DATA_ARRAYS and "qfrc_inverse" not in mjio._DATA_PTR_FIELDS  # (an argument of mjh_inverse, not a member of MjhData)
  assert {"mjh_inverse", "mjh_inv_constraint"} <= set(_abi.FUNCTIONS)
  assert _abi.DEFINES["MJH_ABI_VERSION"] == 45
  assert "inverse_tu.hip" in _abi.UNITS and "inverse.hpp" in _abi.HEADERS and "inverse_tu.hip" not in _abi.UNIT_FLAGS


def test_library_exports_the_entry_points():
  L = _abi.lib()
  assert hasattr(L, "mjh_inverse") and hasattr(L, "mjh_inv_constraint")
  assert L.mjh_abi_version() == 45


def test_make_data_allocates_qfrc_inverse_and_reset_leaves_it():
  mjm = it.model("pendula")
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=3)
  assert d.qfrc_inverse.shape == (3, mjm.nv) and d.qfrc_inverse.dtype == np.float32 and not d.qfrc_inverse.numpy().any()
  d2 = mjw.put_data(mjm, mjw.MjData(mjm), nworld=2)
  assert d2.qfrc_inverse.shape == (2, mjm.nv) and not d2.qfrc_inverse.numpy().any()
  if d.time.t.device.type == "cpu":  # (the host reset; the device reset is checked on the GPU below)
    d.qfrc_inverse.assign(np.full((3, mjm.nv), 7.0, dtype=np.float32))
    mjw.reset_data(m, d)
    assert (d.qfrc_inverse.numpy() == 7.0).all()
  res = pytypes.SimpleNamespace()
  mjw.get_data_into(res, mjm, d2, 1)
  assert res.qfrc_inverse.shape == (mjm.nv,)


def _flagged(xml_flags, option=""):
  return mjw.mjcf.from_xml_string(f'<mujoco><option {option}><flag {xml_flags}/></option><worldbody><body><joint damping="1"/><geom size=".1"/></body></worldbody></mujoco>')


def test_put_model_accepts_invdiscrete_and_refuses_fwdinv():
  m = mjw.put_model(_flagged('invdiscrete="enable"'))
  assert int(m.opt.enableflags) & int(types.EnableBit.INVDISCRETE)
  with pytest.raises(NotImplementedError, match="FWDINV.*are not implemented"):
    mjw.put_model(_flagged('fwdinv="enable"'))
  with pytest.raises(NotImplementedError, match="OVERRIDE.*are not implemented"):
    mjw.put_model(_flagged('override="enable"'))


@pytest.mark.parametrize("integrator,name", [("RK4", "RK4"), ("implicitfast", "implicitfast"), ("implicit", "implicit")])
def test_invdiscrete_refuses_other_integrators(integrator, name):
  mjm = _flagged('invdiscrete="enable"', f'integrator="{integrator}"')
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=1)
  with pytest.raises(NotImplementedError, match=f"invdiscrete.*{name}"):
    mjw.inverse(m, d)


def test_inverse_refuses_sleeping():
  mjm = _flagged('sleep="enable"', 'solver="Newton"')
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=1)
  with pytest.raises(NotImplementedError, match="inverse.*sleep"):
    mjw.inverse(m, d)
  with pytest.raises(NotImplementedError, match="inverse.*sleep"):
    mjw.inv_constraint(m, d)


def test_force_update_is_minus_the_cost_gradient():
  """force_update against central differences of the cost it is written from (an independent route: the cost, not its derivative)."""
  rng = np.random.default_rng(5)
  D, fl = rng.uniform(0.5, 2.0, 12), rng.uniform(0.1, 0.5, 12)
  ne, nf, contacts = 1, 2, [(5, 3, np.array([0.8, 0.8, 0.01, 0.001, 0.001])), (8, 4, np.array([0.6, 0.5, 0.02, 0.001, 0.001]))]

  def cost(jar):
    s = 0.5 * D[0] * jar[0] ** 2
    for r in (1, 2):
      lim = fl[r] / D[r]
      s += 0.5 * D[r] * jar[r] ** 2 if abs(jar[r]) < lim else fl[r] * (abs(jar[r]) - 0.5 * lim)
    for r in (3, 4):
      s += 0.5 * D[r] * min(jar[r], 0.0) ** 2
    for r0, dim, fr in contacts:
      mu = fr[0] / np.sqrt(2.0)
      N, T = mu * jar[r0], np.linalg.norm(jar[r0 + 1:r0 + dim] * fr[:dim - 1])
      if N >= mu * T:
        continue
      if mu * N + T <= 0:
        s += 0.5 * np.sum(D[r0:r0 + dim] * jar[r0:r0 + dim] ** 2)
      else:
        s += 0.5 * D[r0] / (mu * mu * (1 + mu * mu)) * (N - mu * T) ** 2
    return s

  seen = set()
  for trial in range(40):
    jar = rng.standard_normal(12) * (0.2 if trial % 2 else 2.0)
    if trial % 4 == 3:  # (deep in the bottom zone of both contacts: a strongly negative normal row)
      jar[[5, 8]] = -5.0
    f, st, margin = it.force_update(jar, D, fl, ne, nf, contacts, 2.0)
    seen |= {(int(st[5]), 3), (int(st[8]), 4)} | {int(s) for s in st[1:3]}
    if margin.min() < 1e-3:
      continue
    g = np.array([(cost(jar + 1e-6 * e) - cost(jar - 1e-6 * e)) / 2e-6 for e in np.eye(12)])
    np.testing.assert_allclose(f, -g, atol=1e-6)
  assert {(0, 3), (1, 3), (4, 3), (0, 4), (1, 4), (4, 4), 1, 2, 3} <= seen


@pytest.mark.parametrize("key", it.all_cases(), ids=lambda k: f"{k[0]}-{k[1]}{'' if k[2] else '-noeulerdamp'}")
def test_truth_self_checks_and_twin_floors(key):
  """Every state of every case: the oracle's own inverse force equals the applied forces within 1e-8 (case() drops states that do not);
  the float32 twin stays within the 2 % cap of near-boundary rows and agrees on efc_state beyond them; its recorded floors are reproduced
  within a factor 2."""
  worlds = it.case(*key)
  assert len(worlds) == it.NWORLD
  for w in worlds:
    r = w.rows
    own = r["M"] @ r["qacc"] + r["qfrc_bias"] - r["qfrc_passive"] - r["qfrc_constraint"]
    assert it.scaled_err(own, r["qfrc_smooth"] - r["qfrc_passive"] + r["qfrc_bias"]) <= it.SELF_CHECK
  err, near, bad = it.twin_errors(worlds)
  assert near <= it.STATE_CAP and bad == 0, (near, bad)
  rec = dict(zip(it.FIELDS, it.TWIN[key]))
  for f in it.FIELDS:
    assert rec[f] / 2 <= err[f] <= rec[f] * 2 or (err[f] == 0.0 and rec[f] == 0.0), (f, err[f], rec[f])
  if key[0] == "free_bodies":
    assert 0 in [w.rows["nefc"] for w in worlds] and max(w.rows["nefc"] for w in worlds) > 0
  if key[0] in ("free_bodies", "pile_pyramidal", "pile_elliptic", "humanoid", "humanoids3") or key[0] in CHAINS[1:]:
    assert len({w.rows["nefc"] for w in worlds}) > 1  # (nefc differs inside one block)
  if key[1] == "D":
    assert all(w.rows["ne"] == 3 and w.rows["nefc"] == 3 for w in worlds)  # (one connect: three equality rows, always active)
    assert min(float(np.abs(w.want["efc_force"]).max()) for w in worlds) > 1.0  # (the loop closure carries load in every world)


def test_part_b_visits_every_zone():
  z = it.zones(it.case("pile_elliptic", "B"))
  for condim in (3, 4, 6):
    assert z[condim] == {it.ST_SATISFIED, it.ST_QUADRATIC, it.ST_CONE}, (condim, z[condim])
  dims = {c["dim"] for w in it.case("pile_elliptic", "B") for c in w.rows["contacts"]}
  assert {3, 4, 6} <= dims and {1, 3, 4, 6} <= set(int(x) for x in it.model("pile_elliptic").geom_condim)  # (a contact takes the larger condim of its geoms)
  for name in CHAINS:
    assert it.zones(it.case(name, "B"))["friction"] == {it.ST_QUADRATIC, it.ST_LINEARNEG, it.ST_LINEARPOS}, name
    lim = [w.want["efc_state"][w.rows["ne"] + w.rows["nf"]:] for w in it.case(name, "B")]
    assert {0, 1} <= {int(s) for x in lim for s in x} or name == "chain1", name


# ---------------------------------------------------------------------------------------------------------------- GPU
def _device(name, worlds, mjm=None):
  mjm = it.model(name) if mjm is None else mjm
  ncon, njmax = it.sizes(name)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=len(worlds), nconmax=ncon, njmax=njmax)
  for k in it._INPUTS:
    a = getattr(d, k)
    if a.size:
      a.assign(np.array([w.inputs[k] for w in worlds], dtype=np.float32).reshape(a.shape))
  d.qacc.assign(np.array([w.qacc for w in worlds], dtype=np.float32))
  return mjm, m, d


def _check(key, worlds, mjm, d):
  """The engine's outputs of every world against the expectation; prints every figure, then asserts GPU_MARGIN x the twin's floor."""
  import torch

  torch.cuda.synchronize()
  assert (d.overflow.numpy() == 0).all()
  worst = dict.fromkeys(it.FIELDS, 0.0)
  rows_total = left_out = 0
  for wi, w in enumerate(worlds):
    res = pytypes.SimpleNamespace()
    mjw.get_data_into(res, mjm, d, wi)
    r = w.rows
    assert res.nefc == r["nefc"] and (res.ne, res.nf, res.nl) == (r["ne"], r["nf"], r["nl"]), (wi, res.nefc, r["nefc"])
    perm = it.contact_row_map(r, res.contact_geom, res.contact_pos, res.contact_efc_address[:, 0] if res.ncon else [], res.contact_dim)
    assert perm is not None, (key, wi, "contacts do not match the oracle's")
    worst["qfrc_inverse"] = max(worst["qfrc_inverse"], it.scaled_err(res.qfrc_inverse, w.want["qfrc_inverse"]))
    worst["qfrc_constraint"] = max(worst["qfrc_constraint"], it.scaled_err(res.qfrc_constraint, w.want["qfrc_constraint"]))
    worst["efc_force"] = max(worst["efc_force"], it.scaled_err(res.efc_force, w.want["efc_force"][perm]))
    far = w.want["margin"][perm] > w.jar_err
    rows_total += r["nefc"]
    left_out += int((~far).sum())
    np.testing.assert_array_equal(res.efc_state[far], w.want["efc_state"][perm][far], err_msg=f"{key} world {wi}: efc_state")
  rec = dict(zip(it.FIELDS, it.TWIN[key]))
  for f in it.FIELDS:
    print(f"{key} {f}: gpu {worst[f]:.3e}  twin {rec[f]:.3e}  bound {it.GPU_MARGIN * rec[f]:.3e}")
  assert left_out <= it.STATE_CAP * max(rows_total, 1), (left_out, rows_total)
  for f in it.FIELDS:
    assert worst[f] <= it.GPU_MARGIN * rec[f], (key, f, worst[f], rec[f])


@pytest.mark.gpu
@pytest.mark.parametrize("name", A_MODELS + CHAINS)
def test_gpu_forward_identity(name):
  """A: at the oracle's converged qacc the inverse force is the applied force (and the constraint forces are the oracle's)."""
  key = (name, "A", True)
  worlds = it.case(*key)
  mjm, m, d = _device(name, worlds)
  mjw.inverse(m, d)
  _check(key, worlds, mjm, d)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("pile_elliptic",) + CHAINS)
def test_gpu_off_solution(name):
  """B: accelerations aimed at every zone of the friction-loss rows and of the elliptic contacts (condim 3, 4, 6)."""
  key = (name, "B", True)
  worlds = it.case(*key)
  mjm, m, d = _device(name, worlds)
  mjw.inverse(m, d)
  _check(key, worlds, mjm, d)


@pytest.mark.gpu
@pytest.mark.parametrize("eulerdamp", [True, False], ids=["eulerdamp", "noeulerdamp"])
@pytest.mark.parametrize("name", ("humanoid", "pendula"))
def test_gpu_invdiscrete(name, eulerdamp):
  """C: qacc = (qvel' - qvel) / h of the oracle's Euler step; the inverse force is what was applied before the step; d.qacc comes back bitwise."""
  key = (name, "C", eulerdamp)
  worlds = it.case(*key)
  mjm = copy.deepcopy(it.model(name))
  mjm.opt.integrator = int(types.IntegratorType.EULER)
  mjm.opt.enableflags = int(mjm.opt.enableflags) | int(types.EnableBit.INVDISCRETE)
  mjm.opt.disableflags = it.discrete_flags(mjm, eulerdamp)
  mjm, m, d = _device(name, worlds, mjm)
  before = d.qacc.numpy().copy()
  mjw.inverse(m, d)
  _check(key, worlds, mjm, d)
  assert (d.qacc.numpy().view(np.uint32) == before.view(np.uint32)).all()


@pytest.mark.gpu
def test_gpu_connect():
  """D: the four-bar closed by a connect, at connect_truth's closed-form qacc: the inverse force is the applied force, the three rows' forces
  are -D (J qacc - aref) of connect_truth's rows.  inverse() runs com_vel in front of the rows, as fwd_position arranges."""
  key = ("fourbar", "D", True)
  worlds = it.case(*key)
  mjm, m, d = _device("fourbar", worlds)
  mjw.inverse(m, d)
  _check(key, worlds, mjm, d)


SENSOR_XML = """
<mujoco>
  <option timestep="0.002" integrator="Euler"><flag invdiscrete="enable"/></option>
  <worldbody>
    <body name="a" pos="0 0 1"><joint name="j0" type="hinge" axis="0 1 0" damping="0.3"/><geom type="capsule" fromto="0 0 0 0 0 -.3" size=".03" contype="0" conaffinity="0"/>
      <body name="b" pos="0 0 -.3"><joint name="j1" type="hinge" axis="1 0 0" damping="0.2"/><geom type="capsule" fromto="0 0 0 0 0 -.3" size=".03" contype="0" conaffinity="0"/>
        <body name="c" pos="0 0 -.3"><joint name="j2" type="hinge" axis="0 1 0" damping="0.1"/><geom type="capsule" fromto="0 0 0 0 0 -.3" size=".03" contype="0" conaffinity="0"/>
          <site name="tip" pos="0.02 0.01 -.3"/>
        </body>
      </body>
    </body>
  </worldbody>
  <sensor>
    <jointpos joint="j1"/><jointvel joint="j2"/><gyro site="tip"/><accelerometer site="tip"/>
    <framelinacc objtype="body" objname="b"/><frameangacc objtype="body" objname="c"/>
  </sensor>
</mujoco>
"""


@pytest.mark.gpu
@pytest.mark.parametrize("eulerdamp", [True, False], ids=["eulerdamp", "noeulerdamp"])
def test_gpu_sensors_after_inverse(eulerdamp):
  """A CONSISTENCY check, not a truth: sensordata after inverse() is what forward() leaves at the same state and acceleration, position, velocity
  and acceleration sensors alike.  forward() finds qacc; inverse() (invdiscrete, Euler) is then handed qacc itself (eulerdamp off: k_inverse and
  the acceleration sensors read d.qacc) or the discrete acceleration (M + h B)^-1 M qacc that the conversion maps back to it (eulerdamp on: they
  read qacc_c from the scratch; M in float64 from the oracle).  Bound, from the inputs: the conversion qacc_c = qacc_d + M^-1 (h B qacc_d) rounds
  qacc_d, the product, the solve and the sum, 4 ulp of |qacc|_inf (the correction is 1e-2 of qacc, so the solve's conditioning does not show);
  an acceleration sensor is linear in qacc with one coefficient per dof of at most the chain's length, 0.9 m: nv x 4 ulp x |qacc|_inf, plus
  4 ulp of the largest reading for the different launch (forward() reads the sensors in its fused kernels)."""
  from oracle import ref

  mjm = mjw.mjcf.from_xml_string(SENSOR_XML)
  mjm.opt.disableflags = it.discrete_flags(mjm, eulerdamp)
  nworld, rng = it.NWORLD, np.random.default_rng(11)
  qpos = rng.uniform(-1, 1, (nworld, mjm.nq)).astype(np.float32)
  qvel = rng.uniform(-3, 3, (nworld, mjm.nv)).astype(np.float32)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=nworld)
  d.qpos.assign(qpos)
  d.qvel.assign(qvel)
  mjw.forward(m, d)
  want = d.sensordata.numpy().copy()
  qacc = d.qacc.numpy().copy()
  assert want.shape[1] == 14 and (np.abs(want).max(axis=0) > 0).all()
  given = qacc
  if eulerdamp:
    s = ref.RefSim(mjm)
    h, B = float(mjm.opt.timestep), np.diag(np.asarray(mjm.dof_damping, dtype=np.float64))
    given = np.zeros_like(qacc)
    for w in range(nworld):
      s.qpos[:], s.qvel[:] = qpos[w], qvel[w]
      s.forward()
      M = np.array(s.dense_M(), dtype=np.float64)
      given[w] = np.linalg.solve(M + h * B, M @ qacc[w].astype(np.float64))
    assert np.abs(given - qacc).max() > 1e-4 * np.abs(qacc).max()  # (the conversion is not the identity here)
  d.qacc.assign(given)
  d.sensordata.assign(np.zeros_like(want))
  mjw.inverse(m, d)
  got = d.sensordata.numpy()
  eps = float(np.finfo(np.float32).eps)
  bound = 4 * eps * mjm.nv * float(np.abs(qacc).max()) + 4 * eps * float(np.abs(want).max())
  err = float(np.abs(got - want).max())
  print(f"sensordata after inverse, eulerdamp {eulerdamp}: max abs {err:.3e}  bound {bound:.3e}  largest reading {np.abs(want).max():.3e}")
  assert err <= bound
  assert (d.qacc.numpy().view(np.uint32) == given.view(np.uint32)).all()


@pytest.mark.gpu
def test_gpu_repeatable_and_pure():
  import torch

  name, key = "humanoid", ("humanoid", "A", True)
  worlds = it.case(*key)
  mjm, m, d = _device(name, worlds)
  inputs = {k: getattr(d, k).numpy().copy() for k in ("qpos", "qvel", "ctrl", "act", "qacc")}
  mjw.inverse(m, d)
  first = {k: a.numpy().copy() for k, a in (("qfrc_inverse", d.qfrc_inverse), ("qfrc_constraint", d.qfrc_constraint), ("efc_force", d.efc.force), ("efc_state", d.efc.state))}
  mjw.inverse(m, d)
  torch.cuda.synchronize()
  for k, a in (("qfrc_inverse", d.qfrc_inverse), ("qfrc_constraint", d.qfrc_constraint), ("efc_force", d.efc.force), ("efc_state", d.efc.state)):
    assert (a.numpy().view(np.uint32) == first[k].view(np.uint32)).all(), k
  for k, v in inputs.items():
    assert (getattr(d, k).numpy().view(np.uint32) == v.view(np.uint32)).all(), k
  # inv_constraint alone: the same constraint forces
  d.qfrc_constraint.assign(np.zeros_like(first["qfrc_constraint"]))
  mjw.inv_constraint(m, d)
  assert (d.qfrc_constraint.numpy().view(np.uint32) == first["qfrc_constraint"].view(np.uint32)).all()
  assert (d.qfrc_inverse.numpy().view(np.uint32) == first["qfrc_inverse"].view(np.uint32)).all()  # (untouched)
  # a world's result does not depend on nworld
  for wi in (0, it.NWORLD - 1):
    _, m1, d1 = _device(name, [worlds[wi]])
    mjw.inverse(m1, d1)
    assert (d1.qfrc_inverse.numpy()[0].view(np.uint32) == first["qfrc_inverse"][wi].view(np.uint32)).all(), wi
    assert (d1.efc.force.numpy()[0].view(np.uint32) == first["efc_force"][wi].view(np.uint32)).all(), wi
  # the device reset leaves qfrc_inverse alone
  mjw.reset_data(m, d)
  assert (d.qfrc_inverse.numpy().view(np.uint32) == first["qfrc_inverse"].view(np.uint32)).all()


@pytest.mark.gpu
def test_gpu_inverse_can_be_captured():
  """mjh_inverse neither synchronises nor allocates: a captured graph of it replays to the same bits."""
  import torch

  worlds = it.case("pendula", "A")
  mjm, m, d = _device("pendula", worlds)
  mjw.inverse(m, d)  # (kernel attributes are set outside capture)
  want = d.qfrc_inverse.numpy().copy()
  d.qfrc_inverse.assign(np.zeros_like(want))
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  g = torch.cuda.CUDAGraph()
  with torch.cuda.stream(side):
    with torch.cuda.graph(g, stream=side):
      mjw.inverse(m, d)
  g.replay()
  torch.cuda.synchronize()
  assert (d.qfrc_inverse.numpy().view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["NEWTON", "CG"])
def test_gpu_round_trip_through_the_engine(solver):
  """A CONSISTENCY check, not a truth: forward() with the engine's own solver, then inverse() at the qacc it found.  qfrc_inverse minus the
  applied forces is the gradient the solver drove below its tolerance: |gradient| <= tolerance x meaninertia x nv is its stopping rule, to which
  the float32 floor of the inverse evaluation itself (GPU_MARGIN x the twin's figure of part A) is added."""
  name = "humanoid"
  worlds = it.case(name, "A")
  mjm = copy.deepcopy(it.model(name))
  mjm.opt.solver = int(getattr(mjw.SolverType, solver))
  mjm, m, d = _device(name, worlds, mjm)
  mjw.forward(m, d)
  applied = d.qfrc_smooth.numpy() - d.qfrc_passive.numpy() + d.qfrc_bias.numpy()
  niter = d.solver_niter.numpy()
  mjw.inverse(m, d)
  got = d.qfrc_inverse.numpy()
  assert (niter < int(mjm.opt.iterations)).all()
  bound = float(mjm.opt.tolerance) * float(mjm.stat.meaninertia) * mjm.nv
  for w in range(len(worlds)):
    scale = max(1.0, float(np.abs(applied[w]).max()))
    resid = float(np.linalg.norm(got[w].astype(np.float64) - applied[w]))
    print(f"round trip {solver} world {w}: |qfrc_inverse - applied| {resid:.3e}  solver bound {bound:.3e}  float32 floor {it.GPU_MARGIN * it.TWIN[(name, 'A', True)][0] * scale:.3e}")
    assert resid <= bound + it.GPU_MARGIN * it.TWIN[(name, "A", True)][0] * scale * np.sqrt(mjm.nv)
