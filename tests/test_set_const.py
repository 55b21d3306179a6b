"""Device-side set_const (mujoco_warp_amd/set_const.py, csrc/set_const.hpp) against the float64 host restatement mjcf.set_const.

Truth, per world: a deep copy of the host model with the world's parameters written in (every input field rounded to float32 first, so
host and device start from the same numbers), then mjcf.set_const in float64.

Float32 twin of the truth (what ANY float32 implementation can be expected to reach): host_mass_matrix's M and the Jacobian rows rounded
to float32, np.linalg.cholesky in float32, forward substitutions in float32, the same averaging.

Bound: per-element relative error <= max(1e-4, 8 x the twin's error for that model and world) for dof_invweight0, both columns of
body_invweight0 and meaninertia; entries whose truth is exactly 0 must be exactly 0 on the device.  1e-4 is the project's bound for
factor-derived quantities (FACTOR, tests/test_gpu.py); the 8 x term covers ill-conditioned worlds (the device also forms M in float32).
body_subtreemass is a float32 sum of at most nbody terms in a fixed order: nbody x 2^-24 relative.
"""

import copy
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest

import conftest
import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi
from mujoco_warp_amd import io
from mujoco_warp_amd import mjcf

FACTOR = 1e-4  # (tests/test_gpu.py:25)
F32 = np.float32
INPUTS = ("body_mass", "body_inertia", "body_ipos", "body_iquat", "body_pos", "body_quat", "jnt_pos", "jnt_axis", "dof_armature", "qpos0")
OUTPUTS = ("body_subtreemass", "dof_invweight0", "body_invweight0", "meaninertia")
SCALED = ("body_mass", "body_inertia", "dof_armature")

_LOADERS = {
  "pendula": lambda: mjcf.from_xml_string(conftest.PENDULA_XML),
  "free_bodies": lambda: mjcf.from_xml_string(conftest.FREE_BODIES_XML),
  "panda": lambda: mjcf.load_xml(conftest.PANDA_XML),
  "humanoid": lambda: mjcf.load_xml(conftest.HUMANOID_XML),
  "g1": lambda: mjcf.load_xml(conftest.G1_XML),
  "humanoid3": lambda: mjcf.from_xml_string(conftest.multi_humanoid_xml(3), assets_dir=os.path.dirname(conftest.HUMANOID_XML)),
  "clutter": lambda: mjcf.load_xml(os.path.join(conftest.ROOT, "tests", "models", "clutter_synth.xml")),
}
NWORLDS = {"clutter": 2}  # (nv 136: two worlds are enough for the LDS ceiling), every other model: 5
TWIN_MODELS = ("pendula", "free_bodies", "panda", "humanoid", "g1", "humanoid3")


@functools.lru_cache(maxsize=None)
def _model(name):
  return _LOADERS[name]()


def _clone(mjm):
  """Deep copy of a host model without the device Model make_data caches on it."""
  cached = mjm.__dict__.pop("_mjh_model", None)
  try:
    return copy.deepcopy(mjm)
  finally:
    if cached is not None:
      mjm._mjh_model = cached


def _scaled_worlds(mjm, n, mass_scale=None, arm_scale=None):
  """Float32 rows [n, ...] of body_mass, body_inertia, dof_armature: world 0 unscaled, the others with per-body mass / inertia scales
  uniform in [0.25, 4] and per-dof armature scales uniform in [0.5, 2] (numpy default_rng(7)), unless the scales are given."""
  rng = np.random.default_rng(7)
  if mass_scale is None:
    mass_scale = rng.uniform(0.25, 4.0, (n, mjm.nbody))
    mass_scale[0] = 1.0
  if arm_scale is None:
    arm_scale = rng.uniform(0.5, 2.0, (n, mjm.nv))
    arm_scale[0] = 1.0
  ms, as_ = np.asarray(mass_scale, dtype=F32), np.asarray(arm_scale, dtype=F32)
  return dict(body_mass=F32(mjm.body_mass)[None] * ms, body_inertia=F32(mjm.body_inertia)[None] * ms[:, :, None],
              dof_armature=F32(mjm.dof_armature)[None] * as_)


def _host_world(mjm, params, w):
  """Host copy holding world w: every input field rounded to float32, the given rows written in."""
  c = _clone(mjm)
  for name in INPUTS:
    setattr(c, name, np.asarray(getattr(c, name), dtype=F32).astype(np.float64))
  for name, rows in params.items():
    setattr(c, name, np.asarray(rows[w], dtype=np.float64).reshape(np.shape(getattr(c, name))))
  return c


def _truth(c):
  mjcf.set_const(c)
  return dict(body_subtreemass=np.array(c.body_subtreemass), dof_invweight0=np.array(c.dof_invweight0), body_invweight0=np.array(c.body_invweight0),
              meaninertia=np.array([c.stat.meaninertia]))


def _body_jacobians(c, h):
  """{body: 6 x nv Jacobian at xipos} of the bodies mjcf.set_const gives a non-zero row (same rule, same construction)."""
  out = {}
  for b in range(1, c.nbody):
    if c.body_weldid[b] == 0:
      continue
    bb = b
    while bb > 0 and c.body_dofnum[bb] == 0:
      bb = c.body_parentid[bb]
    if bb == 0:
      continue
    J = np.zeros((6, c.nv))
    off = h["xipos"][b] - h["subtree_com"][c.body_rootid[b]]
    d = c.body_dofadr[bb] + c.body_dofnum[bb] - 1
    while d >= 0:
      ang, lin = h["cdof"][d, :3], h["cdof"][d, 3:]
      J[0:3, d] = lin + np.cross(ang, off)
      J[3:6, d] = ang
      d = c.dof_parentid[d]
    out[b] = J
  return out


def _twin(c):
  """The float32 twin of mjcf.set_const(c): M and J rounded to float32, Cholesky and forward substitution in float32."""
  nv, nb = c.nv, c.nbody
  h = mjcf.host_mass_matrix(c, c.qpos0)
  M = h["M"].astype(F32)
  jac = _body_jacobians(c, h)
  bodies = sorted(jac)
  rhs = np.concatenate([np.eye(nv, dtype=F32)] + [jac[b].astype(F32) for b in bodies], axis=0).T.copy()  # [nv, nrhs]
  L = np.linalg.cholesky(M)
  assert L.dtype == F32
  y = np.zeros_like(rhs)
  for i in range(nv):  # L y = rhs, float32 throughout
    y[i] = (rhs[i] - L[i, :i] @ y[:i]) / L[i, i]
  diag = np.sum(y * y, axis=0, dtype=F32)
  A = diag[:nv]
  dof = np.zeros(nv, dtype=F32)
  for j in range(c.njnt):
    d, t = c.jnt_dofadr[j], c.jnt_type[j]
    if t == mjcf.JNT_FREE:
      dof[d : d + 3] = np.mean(A[d : d + 3])
      dof[d + 3 : d + 6] = np.mean(A[d + 3 : d + 6])
    elif t == mjcf.JNT_BALL:
      dof[d : d + 3] = np.mean(A[d : d + 3])
    else:
      dof[d] = A[d]
  body = np.zeros((nb, 2), dtype=F32)
  for k, b in enumerate(bodies):
    ad = diag[nv + 6 * k : nv + 6 * k + 6]
    tr, ro = np.mean(ad[:3]), np.mean(ad[3:])
    if tr < mjcf.MJ_MINVAL and ro > mjcf.MJ_MINVAL:
      tr = ro
    elif ro < mjcf.MJ_MINVAL and tr > mjcf.MJ_MINVAL:
      ro = tr
    body[b] = [tr, ro]
  return dict(dof_invweight0=dof, body_invweight0=body, meaninertia=np.array([np.mean(np.diag(M), dtype=F32)]))


def _err(got, want):
  """Largest per-element relative error over the entries whose truth is not 0; entries whose truth is exactly 0 must be exactly 0."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape
  zero = want == 0
  assert (got[zero] == 0).all(), "an entry whose truth is exactly 0 is not 0"
  return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if (~zero).any() else 0.0


@functools.lru_cache(maxsize=None)
def _reference(name):
  """(params, per world truth, per world twin error) of a listed model, computed once and shared."""
  mjm = _model(name)
  n = NWORLDS.get(name, 5)
  params = _scaled_worlds(mjm, n)
  truths, twin_err = [], []
  for w in range(n):
    c = _host_world(mjm, params, w)
    tw = _twin(c)
    tr = _truth(c)
    truths.append(tr)
    twin_err.append(max(_err(tw[k], tr[k]) for k in ("dof_invweight0", "body_invweight0", "meaninertia")))
  return params, truths, twin_err


def _put_batched(mjm, n, params, fields=None):
  fields = tuple(params) + OUTPUTS if fields is None else fields
  m = mjw.put_model(mjm, batch_sizes={k: n for k in fields})
  for k, rows in params.items():
    getattr(m, k).assign(np.asarray(rows, dtype=F32))
  return m


def _outputs(m):
  return dict(body_subtreemass=m.body_subtreemass.numpy().copy(), dof_invweight0=m.dof_invweight0.numpy().copy(),
              body_invweight0=m.body_invweight0.numpy().copy(), meaninertia=m.stat.meaninertia.numpy().copy())


def _check_world(out, w, truth, twin_err, nbody, label):
  bound = max(FACTOR, 8.0 * twin_err)
  errs = {k: _err(out[k][w], truth[k] if k != "meaninertia" else truth[k][0]) for k in ("dof_invweight0", "meaninertia")}
  errs["body_invweight0[tr]"] = _err(out["body_invweight0"][w][:, 0], truth["body_invweight0"][:, 0])
  errs["body_invweight0[ro]"] = _err(out["body_invweight0"][w][:, 1], truth["body_invweight0"][:, 1])
  esub = _err(out["body_subtreemass"][w], truth["body_subtreemass"])
  print(f"{label} world {w}: twin {twin_err:.2e} device " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" subtreemass {esub:.2e}")
  for k, v in errs.items():
    assert v <= bound, (label, w, k, v, bound)
  assert esub <= nbody * 2.0**-24, (label, w, esub)
  return max(errs.values())


# ---- non-GPU ---------------------------------------------------------------------------------------------------------------------------
def test_public_functions_are_exported():
  for name in ("set_const", "set_const_0", "set_const_fixed", "set_const_spring"):
    assert callable(getattr(mjw, name)), name
  assert importlib.import_module("mujoco_warp_amd.set_const").set_const is mjw.set_const


def test_abi_lists_the_entry_point_within_v45():
  assert "mjh_set_const" in _abi.FUNCTIONS
  assert _abi.DEFINES["MJH_ABI_VERSION"] == 45
  assert _abi.DEFINES["MJH_SET_CONST_FIXED"] == 1 and _abi.DEFINES["MJH_SET_CONST_0"] == 2
  assert "set_const_tu.hip" in _abi.UNITS and "set_const.hpp" in _abi.HEADERS and "set_const_tu.hip" not in _abi.UNIT_FLAGS  # (no fast division)


def test_batch_plan_leading_dimensions():
  sc = importlib.import_module("mujoco_warp_amd.set_const")
  ins = dict.fromkeys(INPUTS, 1)
  outs = dict.fromkeys(("dof_invweight0", "body_invweight0", "meaninertia", "body_subtreemass"), 1)
  assert sc.batch_plan(ins, outs) == 1
  assert sc.batch_plan({**ins, "body_mass": 4, "body_inertia": 4}, dict.fromkeys(outs, 4)) == 4
  with pytest.raises(ValueError, match="body_invweight0"):  # an output not batched to N: its name is in the message
    sc.batch_plan({**ins, "body_mass": 4}, {**dict.fromkeys(outs, 4), "body_invweight0": 1})
  with pytest.raises(ValueError, match="batch_sizes"):
    sc.batch_plan({**ins, "body_mass": 4}, outs)
  with pytest.raises(ValueError, match="body_mass"):  # mixed leading dimensions 2 and 4
    sc.batch_plan({**ins, "body_mass": 2, "dof_armature": 4}, dict.fromkeys(outs, 4))
  with pytest.raises(ValueError):  # outputs batched wider than the inputs: world w of the output has no world w of the input
    sc.batch_plan(ins, dict.fromkeys(outs, 3))


def test_unbatched_outputs_raise_on_a_model():
  """The check runs before anything touches the device: a humanoid with per-world masses and shared outputs."""
  m = mjw.put_model(_model("humanoid"), batch_sizes={"body_mass": 3})
  for fn in (mjw.set_const, mjw.set_const_0, mjw.set_const_fixed):
    with pytest.raises(ValueError, match="batch_sizes"):
      fn(m, None)
  mjw.set_const_spring(m, None)  # the documented no-op


STATIC_BOX_XML = """
<mujoco>
  <worldbody>
    <body name="shelf" pos="0 0 1"><geom type="box" size=".2 .2 .1" density="500"/>
      <body name="knob" pos="0 0 .2"><geom type="sphere" size=".05" density="500"/></body>
    </body>
  </worldbody>
</mujoco>
"""


def test_nv0_takes_the_early_return():
  mjm = mjcf.from_xml_string(STATIC_BOX_XML)
  assert mjm.nv == 0
  m = mjw.put_model(mjm)
  m.body_mass.assign(F32(mjm.body_mass)[None] * F32(2))
  m.stat.meaninertia.fill_(7.0)
  m.body_invweight0.fill_(3.0)
  mjw.set_const(m, None)  # (no device: the library is never reached)
  c = _host_world(mjm, dict(body_mass=F32(mjm.body_mass)[None] * F32(2)), 0)
  truth = _truth(c)
  assert _err(m.body_subtreemass.numpy()[0], truth["body_subtreemass"]) <= mjm.nbody * 2.0**-24
  assert m.body_subtreemass.numpy()[0, 0] > 0
  assert (m.stat.meaninertia.numpy() == 1).all() and (m.body_invweight0.numpy() == 0).all()


@pytest.mark.parametrize("name", TWIN_MODELS)
def test_twin_agrees_with_truth(name):
  """The float32 twin stays within 2.5e-5 of mjcf.set_const on every world of the listed models: 1e-4 is the bound in force."""
  _, _, twin_err = _reference(name)
  print(name, "worst twin error", max(twin_err))
  assert max(twin_err) <= 2.5e-5


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_LOADERS))
def test_fields_against_truth(name):
  mjm = _model(name)
  params, truths, twin_err = _reference(name)
  n = len(truths)
  m = _put_batched(mjm, n, params)
  mjw.set_const(m, None)
  out = _outputs(m)
  worst = max(_check_world(out, w, truths[w], twin_err[w], mjm.nbody, name) for w in range(n))
  print(f"{name}: worst device error {worst:.2e}, worst twin error {max(twin_err):.2e}")


@pytest.mark.gpu
def test_partial_batching_is_deterministic():
  """Only body_mass and body_inertia are per world (N = 67); qpos0, the armature and the poses keep leading dimension 1."""
  mjm = _model("humanoid")
  n = 67
  rng = np.random.default_rng(11)
  scale = rng.uniform(0.25, 4.0, (n, mjm.nbody))
  scale[0] = 1.0
  scale[13] = scale[40] = scale[66] = scale[5]  # worlds with identical parameters
  p = _scaled_worlds(mjm, n, mass_scale=scale, arm_scale=np.ones((n, mjm.nv)))
  params = dict(body_mass=p["body_mass"], body_inertia=p["body_inertia"])
  m = _put_batched(mjm, n, params)
  assert m.dof_armature.shape[0] == 1 and m.qpos0.shape[0] == 1 and m.body_pos.shape[0] == 1
  mjw.set_const(m, None)
  a = _outputs(m)
  mjw.set_const(m, None)
  b = _outputs(m)
  for k in OUTPUTS:
    assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all(), k  # two calls: the same bits
    for w in (13, 40, 66):
      assert (a[k][w].view(np.uint32) == a[k][5].view(np.uint32)).all(), (k, w)  # identical worlds: the same bits
  for w in (0, 5, 31, 64, 66):
    c = _host_world(mjm, params, w)
    tw, tr = _twin(c), _truth(c)
    _check_world(a, w, tr, max(_err(tw[k], tr[k]) for k in tw), mjm.nbody, "humanoid/partial")


@pytest.mark.gpu
def test_unbatched_in_place_mass_change():
  mjm = _model("humanoid")
  m = mjw.put_model(mjm)
  params = _scaled_worlds(mjm, 2)
  params = {k: v[1:] for k, v in params.items() if k != "dof_armature"}
  for k, rows in params.items():
    getattr(m, k).assign(rows)
  mjw.set_const(m, None)
  c = _host_world(mjm, params, 0)
  tw, tr = _twin(c), _truth(c)
  _check_world(_outputs(m), 0, tr, max(_err(tw[k], tr[k]) for k in tw), mjm.nbody, "humanoid/in place")


@pytest.mark.gpu
def test_unbatched_in_place_qpos0_change():
  """A free body's qpos0 moved and turned: the constants are those of the new pose (the box's rotational weight about world axes changes)."""
  mjm = _model("free_bodies")
  m = mjw.put_model(mjm)
  q = F32(mjm.qpos0).copy()
  q[0:3] += F32([0.3, -0.2, 0.5])
  quat = np.array([0.8, 0.3, -0.4, 0.2])
  q[3:7] = F32(quat / np.linalg.norm(quat))
  m.qpos0.assign(q[None])
  mjw.set_const(m, None)
  params = dict(qpos0=q[None])
  c = _host_world(mjm, params, 0)
  tw, tr = _twin(c), _truth(c)
  _check_world(_outputs(m), 0, tr, max(_err(tw[k], tr[k]) for k in tw), mjm.nbody, "free_bodies/qpos0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["humanoid", "pendula", "free_bodies"])
def test_exact_scaling_law(name):
  """World 1 = world 0 with body_mass, body_inertia and dof_armature times 4: a power of two commutes with every float32 operation of the
  path, so the outputs scale by exactly 4 (4 ulp are allowed for hardware reciprocal / rsqrt seeds)."""
  mjm = _model(name)
  params = _scaled_worlds(mjm, 2, mass_scale=np.stack([np.ones(mjm.nbody), np.full(mjm.nbody, 4.0)]), arm_scale=np.stack([np.ones(mjm.nv), np.full(mjm.nv, 4.0)]))
  m = _put_batched(mjm, 2, params)
  mjw.set_const(m, None)
  o = _outputs(m)
  np.testing.assert_allclose(o["dof_invweight0"][1], o["dof_invweight0"][0] / 4, rtol=5e-7, atol=0)
  np.testing.assert_allclose(o["body_invweight0"][1], o["body_invweight0"][0] / 4, rtol=5e-7, atol=0)
  np.testing.assert_allclose(o["meaninertia"][1], 4 * o["meaninertia"][0], rtol=5e-7, atol=0)
  np.testing.assert_allclose(o["body_subtreemass"][1], 4 * o["body_subtreemass"][0], rtol=5e-7, atol=0)
  assert (o["dof_invweight0"][0] > 0).all()
  print(name, "exact:", all((o[k][1] == o[k][0] * s).all() for k, s in (("dof_invweight0", 0.25), ("body_invweight0", 0.25), ("meaninertia", 4), ("body_subtreemass", 4))))


def _efc_d(m, mjm, nworld):
  d = mjw.make_data(mjm, nworld=nworld, nconmax=24, njmax=64)
  mjw.reset_data_keyframe(m, d, 0)
  mjw.forward(m, d)
  return d.efc.D.numpy().copy(), d.nefc.numpy().copy()


@pytest.mark.gpu
def test_constraint_weights_follow_the_masses():
  """End to end: the humanoid at its contact keyframe, 4 worlds scaled by 1, 0.5, 2, 4.  After set_const every world's efc.D is that of a
  single-world model built from the world's host copy; before, the x 4 world is about 4 x off."""
  mjm = _model("humanoid")
  scales = (1.0, 0.5, 2.0, 4.0)
  params = _scaled_worlds(mjm, 4, mass_scale=np.array(scales)[:, None] * np.ones(mjm.nbody), arm_scale=np.array(scales)[:, None] * np.ones(mjm.nv))
  want = []
  for w in range(4):
    c = _host_world(mjm, params, w)
    mjcf.set_const(c)
    D, nefc = _efc_d(mjw.put_model(c), c, 1)
    want.append(D[0, : int(nefc[0])])
  assert len(want[0]) > 0
  m = _put_batched(mjm, 4, params)
  stale, nefc = _efc_d(m, mjm, 4)
  assert [int(x) for x in nefc] == [len(x) for x in want]
  e_stale = _err(stale[3, : len(want[3])], want[3])
  mjw.set_const(m, None)
  fresh, _ = _efc_d(m, mjm, 4)
  errs = [_err(fresh[w, : len(want[w])], want[w]) for w in range(4)]
  print("efc.D: stale x4 world", e_stale, "after set_const", errs)
  assert e_stale > 100 * FACTOR
  assert max(errs) <= FACTOR


def _model_arrays(m):
  get = lambda n: getattr(m.opt, n[4:]) if n.startswith("opt_") else getattr(m.stat, n[5:]) if n.startswith("stat_") else getattr(m, n)
  return {n: get(n) for n in io._MODEL_PTR_FIELDS}


def _snapshot(arrays):
  return {n: a.numpy().copy() for n, a in arrays.items()}


def _same_bits(a, b):
  return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_nothing_else_moves():
  import torch

  mjm = _model("humanoid")
  m = mjw.put_model(mjm)
  da = mjw.make_data(mjm, nworld=64, nconmax=24, njmax=64)
  db = mjw.make_data(mjm, nworld=64, nconmax=24, njmax=64)
  for d in (da, db):
    mjw.reset_data_keyframe(m, d, 0)
  graph = mjw.StepGraph(m, db)
  for i in range(3):
    mjw.step(m, da)
    graph.launch()
  m.body_mass.assign(m.body_mass.numpy() * F32(2))
  m.body_inertia.assign(m.body_inertia.numpy() * F32(2))
  torch.cuda.synchronize()
  data0 = _snapshot({n: io._get_data_field(da, n) for n in io._DATA_PTR_FIELDS})
  marr = _model_arrays(m)
  model0, ptr0 = _snapshot(marr), {n: a.ptr for n, a in marr.items()}
  mjw.set_const(m, da)
  torch.cuda.synchronize()
  data1 = _snapshot({n: io._get_data_field(da, n) for n in io._DATA_PTR_FIELDS})
  for n in data0:
    assert _same_bits(data0[n], data1[n]), f"Data.{n} changed"
  marr1 = _model_arrays(m)
  outs = {"body_subtreemass", "dof_invweight0", "body_invweight0", "stat_meaninertia"}
  for n, a in marr1.items():
    assert a is marr[n] and a.ptr == ptr0[n], f"Model.{n} was re-bound"
    if n in outs:
      assert not _same_bits(model0[n], a.numpy()), f"Model.{n} did not change"
    else:
      assert _same_bits(model0[n], a.numpy()), f"Model.{n} changed"
  # the graph captured before the call keeps replaying the same kernels on the same pointers, now with the new constants
  for i in range(3):
    mjw.step(m, da)
    graph.launch()
  torch.cuda.synchronize()
  assert _same_bits(da.qpos.numpy(), db.qpos.numpy()) and _same_bits(da.qvel.numpy(), db.qvel.numpy())


@pytest.mark.gpu
def test_fixed_and_qpos0_parts_split():
  mjm = _model("humanoid")
  m = mjw.put_model(mjm)
  mjw.set_const(m, None)
  base = _outputs(m)
  m.body_mass.assign(m.body_mass.numpy() * F32(1.5))
  mjw.set_const_fixed(m, None)
  a = _outputs(m)
  assert not _same_bits(a["body_subtreemass"], base["body_subtreemass"])
  for k in ("dof_invweight0", "body_invweight0", "meaninertia"):
    assert _same_bits(a[k], base[k]), k
  m.body_subtreemass.assign(base["body_subtreemass"])
  mjw.set_const_0(m, None)
  b = _outputs(m)
  assert _same_bits(b["body_subtreemass"], base["body_subtreemass"])
  for k in ("dof_invweight0", "body_invweight0", "meaninertia"):
    assert not _same_bits(b[k], base[k]), k
  mjw.set_const(m, None)
  c = _outputs(m)
  assert _same_bits(c["body_subtreemass"], a["body_subtreemass"])
  for k in ("dof_invweight0", "body_invweight0", "meaninertia"):
    assert _same_bits(c[k], b[k]), k  # (the qpos0 part does not depend on the stored subtree masses)


@pytest.mark.gpu
def test_c_abi_nv0_and_argument_checks():
  """mjh_set_const on a model without dofs writes the degenerate constants; bad arguments are refused before any launch."""
  import torch

  mjm = mjcf.from_xml_string(STATIC_BOX_XML)
  m = mjw.put_model(mjm)
  m.stat.meaninertia.fill_(7.0)
  m.body_invweight0.fill_(3.0)
  m.body_subtreemass.zero_()
  L, cm = _abi.lib(), ctypes.byref(io.c_model(m))
  stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  p = lambda a: ctypes.c_void_p(a.ptr)
  assert L.mjh_set_const(cm, 1, p(m.body_subtreemass), None, p(m.body_invweight0), p(m.stat.meaninertia), 3, stream) == 0
  torch.cuda.synchronize()
  c = _host_world(mjm, {}, 0)
  assert _err(m.body_subtreemass.numpy()[0], _truth(c)["body_subtreemass"]) <= mjm.nbody * 2.0**-24
  assert (m.stat.meaninertia.numpy() == 1).all() and (m.body_invweight0.numpy() == 0).all()
  assert L.mjh_set_const(cm, 0, p(m.body_subtreemass), None, None, None, 1, stream) == _abi.DEFINES["MJH_E_ARG"]
  assert L.mjh_set_const(cm, 1, p(m.body_subtreemass), None, None, None, 4, stream) == _abi.DEFINES["MJH_E_ARG"]
