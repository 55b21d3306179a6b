"""Float64 truth for inverse dynamics (tests/test_inverse.py).  No MuJoCo is installed; the truth comes from the float64 oracle's FORWARD pass:

  A  forward identity   after RefSim.forward() at tolerance 1e-12 the force that produces the oracle's qacc is what was applied:
                        qfrc_inverse = qfrc_smooth - qfrc_passive + qfrc_bias (the oracle's own fields: qfrc_applied + qfrc_actuator +
                        J' xfrc_applied), qfrc_constraint and efc_force are the oracle's.  No formula of the kernel is restated.
  B  off-solution qacc  force_update below: the per-row force update written from the constraint COST (force = -d cost / d jar), in numpy,
                        on the oracle's rows; qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - J' force.
  C  discrete           RefSim.step() with Euler; qacc = (qvel' - qvel) / h; the expectation is A's, at the state before the step.
  D  connects           tests/connect_truth.Truth on the four-bar of tests/test_connect.py: its rows and its closed-form qacc; the expectation
                        is the applied force (the stripped oracle's qfrc_smooth - qfrc_passive + qfrc_bias).

The float32 TWIN evaluates the same quantities with RefSim(real="f32") rows and float32 numpy arithmetic; its error against the float64
expectation is the floor a float32 engine is measured against (TWIN below; the GPU bound is GPU_MARGIN x the recorded figure).
"""

import functools

import numpy as np

import mujoco_warp_amd as mjw
from oracle import ref
from tests import conftest
from tests import connect_truth as ct

ST_SATISFIED, ST_QUADRATIC, ST_LINEARNEG, ST_LINEARPOS, ST_CONE = 0, 1, 2, 3, 4
NWORLD = 5
GPU_MARGIN = 4.0  # a different summation order and the engine's v_rcp / v_rsq paths
STATE_CAP = 0.02  # rows per case that may be left out of the exact efc_state comparison (next to a zone boundary)
SELF_CHECK = 1e-8  # the oracle's own M qacc + bias - passive - J' force against the applied forces, relative


# ---- models -------------------------------------------------------------------------------------------------------------------------
def chain_xml(n):
  """A hinge chain of n dofs, every joint limited and with friction loss, motors on every fourth joint; no contacts."""
  body, close = "", ""
  for i in range(n):
    axis = ("0 1 0", "1 0 0", "0 0 1")[i % 3]
    body += (f'<body name="b{i}" pos="0 0 {-0.06 if i else 0}"><joint name="j{i}" type="hinge" axis="{axis}" range="-20 20" limited="true" '
             f'frictionloss="{0.02 + 0.01 * (i % 4)}" damping="0.02" armature="0.005"/><geom type="capsule" fromto="0 0 0 0 0 -.06" size=".01" '
             f'contype="0" conaffinity="0"/>')
    close += "</body>"
  motors = "".join(f'<motor joint="j{i}" gear="0.5"/>' for i in range(0, n, 4))
  return f'<mujoco><option timestep="0.002"/><worldbody>{body}{close}</worldbody><actuator>{motors}</actuator></mujoco>'


def pile_xml(elliptic):
  """conftest.PILE_XML; elliptic: with elliptic cones and contacts of condim 1, 3, 4 and 6 in one scene."""
  xml = conftest.PILE_XML
  if elliptic:
    xml = xml.replace('solver="CG"', 'solver="CG" cone="elliptic"')
    xml = xml.replace('<geom type="capsule" size=".06 .15"/>', '<geom type="capsule" size=".06 .15" condim="4"/>')
    xml = xml.replace('<geom type="capsule" size=".05 .12"/>', '<geom type="capsule" size=".05 .12" condim="6"/>')
  return xml


# the four-bar linkage of tests/test_connect.py (that module is written to be imported by pytest only): crank a, coupler b, rocker c in the x-z
# plane, closed by one connect; FOURBAR_Q is a closed parallelogram
NOCOL = 'contype="0" conaffinity="0"'
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
FOURBAR_Q = np.array([0.5, -0.5, 0.5])

CHAIN_NV = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
BIG_CHAIN = "chain130"  # three 64-lane trips round up to the four-trip instantiation of k_inverse, the largest one built
MODELS = {
  "pendula": lambda: mjw.mjcf.from_xml_string(conftest.PENDULA_XML),
  "free_bodies": lambda: mjw.mjcf.from_xml_string(conftest.FREE_BODIES_XML),
  "pile_pyramidal": lambda: mjw.mjcf.from_xml_string(pile_xml(False)),
  "pile_elliptic": lambda: mjw.mjcf.from_xml_string(pile_xml(True)),
  "humanoid": lambda: mjw.mjcf.load_xml(conftest.HUMANOID_XML),
  "panda": lambda: mjw.mjcf.load_xml(conftest.PANDA_XML),
  "humanoids3": lambda: mjw.mjcf.from_xml_string(conftest.multi_humanoid_xml(3)),
  **{f"chain{n}": (lambda n=n: mjw.mjcf.from_xml_string(chain_xml(n))) for n in CHAIN_NV + (130,)},
}
SIZES = {"humanoid": (24, 64), "humanoids3": (48, 160), "panda": (16, 32), "chain63": (8, 160), "chain64": (8, 160), "chain65": (8, 160),
         BIG_CHAIN: (8, 288)}  # (nconmax, njmax); default (32, 96)


@functools.lru_cache(maxsize=None)
def model(name):
  if name == "fourbar":  # (part D only: not in MODELS, the oracle cannot run a model with connects)
    return mjw.mjcf.from_xml_string(FOURBAR_XML)
  return MODELS[name]()


def sizes(name):
  return SIZES.get(name, (32, 96))


# ---- the force update, from the constraint cost -------------------------------------------------------------------------------------
def force_update(jar, D, floss, ne, nf, contacts, impratio, dt=np.float64):
  """(force, state, margin) of every row at jar = J qacc - aref.  The cost of a row, s(jar), and force = -ds/djar:
     equality        D jar^2 / 2 everywhere;
     friction loss   the same inside |jar| < f / D, linear with slope -+f outside (three zones);
     limit, contact  D jar^2 / 2 for jar < 0, nothing otherwise (pyramidal and frictionless contacts are such rows);
     elliptic contact (rows r0 .. r0 + dim, friction coefficients fr): in N = mu jar_0, u_j = fr_j jar_j, T = |u|, mu = fr_0 / sqrt(impratio):
                     nothing for N >= mu T (top), every row its own quadratic for mu N + T <= 0 (bottom), dm (N - mu T)^2 / 2 with
                     dm = D_0 / (mu^2 (1 + mu^2)) between (middle).
  margin: distance of the row's jar (its contact's N, T) from the nearest zone boundary, inf where there is none (equality rows)."""
  jar, D, floss = (np.asarray(x, dtype=dt) for x in (jar, D, floss))
  n = len(jar)
  force, state, margin = np.zeros(n, dtype=dt), np.zeros(n, dtype=np.int32), np.full(n, np.inf)
  for r in range(n):
    if r < ne:
      force[r], state[r] = -D[r] * jar[r], ST_QUADRATIC
    elif r < ne + nf:
      lim = floss[r] / D[r]
      margin[r] = min(abs(jar[r] + lim), abs(jar[r] - lim))
      if jar[r] <= -lim:
        force[r], state[r] = floss[r], ST_LINEARNEG
      elif jar[r] >= lim:
        force[r], state[r] = -floss[r], ST_LINEARPOS
      else:
        force[r], state[r] = -D[r] * jar[r], ST_QUADRATIC
    else:
      margin[r] = abs(jar[r])
      if jar[r] < 0:
        force[r], state[r] = -D[r] * jar[r], ST_QUADRATIC
  inv = dt(1.0) / np.sqrt(dt(impratio))
  for r0, dim, fr in contacts:
    fr = np.asarray(fr, dtype=dt)
    mu = fr[0] * inv
    u = jar[r0 + 1:r0 + dim] * fr[:dim - 1]
    N, T = mu * jar[r0], np.sqrt(np.sum(u * u))
    margin[r0:r0 + dim] = min(abs(N - mu * T), abs(mu * N + T))
    if N >= mu * T:
      force[r0:r0 + dim], state[r0:r0 + dim] = 0, ST_SATISFIED
    elif mu * N + T <= 0:
      force[r0:r0 + dim], state[r0:r0 + dim] = -D[r0:r0 + dim] * jar[r0:r0 + dim], ST_QUADRATIC
    else:
      dm = D[r0] / (mu * mu * (dt(1.0) + mu * mu))
      resid = N - mu * T
      force[r0] = -dm * resid * mu
      force[r0 + 1:r0 + dim] = dm * resid * mu * (u / T) * fr[:dim - 1]
      state[r0:r0 + dim] = ST_CONE
  return force, state, margin


# ---- states through the oracle --------------------------------------------------------------------------------------------------------
_INPUTS = ("qpos", "qvel", "act", "ctrl", "qfrc_applied", "xfrc_applied")


def _f32(x):
  return np.asarray(x, dtype=np.float32).astype(np.float64)


def _sim(name, real="f64", integrator=None):
  ncon, njmax = sizes(name)
  return ref.RefSim(model(name), nconmax=ncon, njmax=njmax, solver=2, tolerance=1e-12, iterations=200, integrator=integrator, real=real)


def _inputs(name, w):
  """The inputs of world w, as float32 holds them: a short oracle rollout under the bench's control noise (chains: a random pose at and
  beyond the joint limits), then nonzero ctrl, qfrc_applied and xfrc_applied."""
  mjm = model(name)
  rng = np.random.default_rng(1000 + 17 * w + len(name))
  s = _sim(name)
  if name.startswith("chain"):
    s.qpos[:] = rng.uniform(-0.45, 0.45, mjm.nq)  # (range: +-0.349 rad)
    s.qvel[:] = rng.uniform(-2.0, 2.0, mjm.nv)
  else:
    s.reset(key=0 if int(getattr(mjm, "nkey", 0)) else None)
    for i in range(2 + 5 * w):
      s.ctrl_noise(i, w, 0.1, 0.1)
      s.step()
    if name == "free_bodies" and w % 2:  # (every other world: the bodies in the air, nefc == 0)
      s.qpos[2::7] += 1.0
  if mjm.nu:
    s.ctrl[:] = s.ctrl + rng.uniform(-0.2, 0.2, mjm.nu)
  scale = float(mjm.stat.meaninertia)
  s.qfrc_applied[:] = rng.uniform(-1, 1, mjm.nv) * scale
  s.xfrc_applied[1:] = rng.uniform(-1, 1, (mjm.nbody - 1, 6)) * scale
  return {k: _f32(getattr(s, k)).copy() for k in _INPUTS}


def _load(s, inp):
  for k in _INPUTS:
    getattr(s, k)[...] = inp[k]


def _rows(s):
  """The rows and smooth terms of a RefSim after forward(), copied."""
  n = int(s.nefc)
  out = {k: np.array(getattr(s, "efc_" + k)[:n]) for k in ("J", "D", "aref", "frictionloss", "force", "state", "type", "id")}
  out.update(nefc=n, ne=int(s.ne), nf=int(s.nf), nl=int(s.nl), M=np.array(s.dense_M(), dtype=s.R.np_real), overflow=int(s.overflow))
  for k in ("qacc", "qfrc_bias", "qfrc_passive", "qfrc_smooth", "qfrc_constraint", "qfrc_actuator"):
    out[k] = np.array(getattr(s, k))
  ell = int(s.mjm.opt.cone) == 1
  con = []
  for c in range(int(s.ncon)):
    r0, dim = int(s.con_efc_address[c][0]), int(s.con_dim[c])
    if r0 >= 0:
      con.append(dict(r0=r0, dim=dim if (ell or dim == 1) else 2 * (dim - 1), geom=tuple(int(g) for g in s.con_geom[c]), pos=np.array(s.con_pos[c], dtype=np.float64),
                      friction=np.array(s.con_friction[c], dtype=np.float64), elliptic=ell and dim > 1))
  out["contacts"] = con
  return out


def _ell(rows):
  return [(c["r0"], min(c["dim"], rows["nefc"] - c["r0"]), c["friction"]) for c in rows["contacts"] if c["elliptic"]]


def evaluate(rows, qacc, impratio, dt=np.float64):
  """force_update and the inverse force at qacc on the given rows, in arithmetic `dt`."""
  c = lambda x: np.asarray(x, dtype=dt)
  qacc = c(qacc)
  jar = c(rows["J"]) @ qacc - c(rows["aref"]) if rows["nefc"] else np.zeros(0, dtype=dt)
  force, state, margin = force_update(jar, rows["D"], rows["frictionloss"], rows["ne"], rows["nf"], _ell(rows), impratio, dt)
  qc = c(rows["J"]).T @ force if rows["nefc"] else np.zeros(len(qacc), dtype=dt)
  qinv = c(rows["M"]) @ qacc + c(rows["qfrc_bias"]) - c(rows["qfrc_passive"]) - qc
  return dict(jar=jar, efc_force=force, efc_state=state, margin=margin, qfrc_constraint=qc, qfrc_inverse=qinv)


def scaled_err(got, want):
  """max |got - want| / max(1, |want|_inf)."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  if want.size == 0:
    return 0.0
  return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


FIELDS = ("qfrc_inverse", "qfrc_constraint", "efc_force")


class World:
  """One world of a case: inputs, the float64 rows, the qacc handed to the engine (float32 values), the float64 expectation there and the
  float32 twin's result."""


def _perturbation(name, w, rows, impratio):
  """Off-solution qacc of part B, aimed at the zones: world 0 a small random vector; world 1 puts every dof with friction loss inside the
  quadratic zone of its row (J of such a row is the dof's unit vector); worlds 2 / 3 / 4 move the elliptic contacts towards their top / bottom /
  middle zone (least squares on the contacts' rows) and add random vectors of growing size, which send other rows across their boundaries."""
  rng = np.random.default_rng(77 + w + len(name))
  nv = len(rows["qacc"])
  k = w % 5
  q = rows["qacc"] + rng.standard_normal(nv) * (0.1, 1.0, 10.0, 100.0, 1000.0)[k]
  if k == 1:
    for r in range(rows["ne"], rows["ne"] + rows["nf"]):
      dof = int(np.flatnonzero(rows["J"][r])[0])
      q[dof] = rows["aref"][r] + rng.uniform(-0.8, 0.8) * rows["frictionloss"][r] / rows["D"][r]
  ell = _ell(rows)
  if k >= 2 and ell:
    idx = np.concatenate([np.arange(r0, r0 + dim) for r0, dim, _ in ell])
    target = np.concatenate([np.concatenate([[{2: 1.0, 3: -1.0, 4: -0.1}[k]], rng.standard_normal(dim - 1) * {2: 0.05, 3: 0.05, 4: 1.0}[k]]) for _, dim, _ in ell])
    # (rcond: the stacked contact rows are nearly dependent -- contacts that share a body --; the untruncated pseudo-inverse answered with
    # accelerations of 1e6 whose J qacc cancels to 1e-4 of its terms, which measures the rounding of the rows and not the force update)
    q = rows["qacc"] + np.linalg.lstsq(rows["J"][idx], target * 50.0 - (rows["J"][idx] @ rows["qacc"] - rows["aref"][idx]), rcond=1e-2)[0]
  return q


def discrete_flags(mjm, eulerdamp):
  """disableflags of part C: the model's, with DisableBit.EULERDAMP cleared or set."""
  return (int(mjm.opt.disableflags) & ~(1 << 15)) | (0 if eulerdamp else 1 << 15)


@functools.lru_cache(maxsize=None)
def case(name, part="A", eulerdamp=True):
  """[World] * NWORLD of model `name` for part A, B or C (worlds whose oracle solve did not converge to SELF_CHECK are dropped and
  replaced by the next seed: the list always has NWORLD entries)."""
  if part == "D":
    return _connect_case(name)
  mjm = model(name)
  impratio = float(mjm.opt.impratio)
  h = float(mjm.opt.timestep)
  out, seed = [], 0
  s64 = _sim(name, integrator=0 if part == "C" else None)
  s32 = _sim(name, "f32", integrator=0 if part == "C" else None)
  if part == "C":  # (the humanoid's file disables eulerdamp: both settings are set explicitly)
    for s in (s64, s32):
      s.cm.disableflags = discrete_flags(mjm, eulerdamp)
  while len(out) < NWORLD and seed < 4 * NWORLD:
    inp = _inputs(name, seed)
    seed += 1
    _load(s64, inp)
    s64.forward()
    r64 = _rows(s64)
    want_inv = r64["qfrc_smooth"] - r64["qfrc_passive"] + r64["qfrc_bias"]
    own = r64["M"] @ r64["qacc"] + r64["qfrc_bias"] - r64["qfrc_passive"] - r64["qfrc_constraint"]
    if r64["overflow"] or scaled_err(own, want_inv) > SELF_CHECK:
      continue  # (not converged: dropped, the bound is not widened)
    _load(s32, inp)
    s32.forward()
    r32 = _rows(s32)
    if r32["nefc"] != r64["nefc"] or (r32["type"] != r64["type"]).any():
      continue  # (a contact at the edge of its margin in float32: no twin for this state)
    w = World()
    w.inputs, w.rows, w.rows32 = inp, r64, r32
    qacc_c = r64["qacc"]  # the continuous-time acceleration everything is evaluated at
    if part == "A":
      w.qacc = _f32(qacc_c)
      w.want = dict(qfrc_inverse=want_inv, qfrc_constraint=r64["qfrc_constraint"], efc_force=r64["force"], efc_state=r64["state"],
                    margin=evaluate(r64, qacc_c, impratio)["margin"])
    elif part == "B":
      w.qacc = _f32(_perturbation(name, len(out), r64, impratio))
      w.want = evaluate(r64, w.qacc, impratio)
    else:
      s64.step()
      _load(s32, inp)  # (the twin's factor of M is the state's; nothing of the step is used)
      w.qacc = _f32((np.array(s64.qvel) - inp["qvel"]) / h)
      w.want = dict(qfrc_inverse=want_inv, qfrc_constraint=r64["qfrc_constraint"], efc_force=r64["force"], efc_state=r64["state"],
                    margin=evaluate(r64, qacc_c, impratio)["margin"])
      _load(s64, inp)
    # the float32 twin at the same float32 qacc
    q32 = w.qacc.astype(np.float32)
    if part == "C" and eulerdamp and not (int(mjm.opt.disableflags) & (1 << 6)):
      damp = np.asarray(mjm.dof_damping, dtype=np.float32)
      s32.forward()
      q32 = (q32 + np.float32(h) * s32.solve_m(damp * q32)).astype(np.float32)
    w.twin = evaluate(r32, q32, impratio, np.float32)
    w.jar_err = float(np.max(np.abs(w.twin["margin"][np.isfinite(w.want["margin"])] - w.want["margin"][np.isfinite(w.want["margin"])]), initial=0.0))
    out.append(w)
  assert len(out) == NWORLD, (name, part, len(out))
  return out


# ---- part D: connects ------------------------------------------------------------------------------------------------------------------
def _anchor_gap(mjm, e, xpos, xmat, dt):
  """p1 - p2 of connect e from the given body poses, in arithmetic `dt` (connect_truth.Truth.gap on poses that are already there)."""
  data = np.asarray(mjm.eq_data, dtype=dt).reshape(-1, 11)[e]
  p = []
  for side, obj in enumerate((int(mjm.eq_obj1id[e]), int(mjm.eq_obj2id[e]))):
    if int(mjm.eq_objtype[e]) == ct.OBJ_SITE:
      b, local = int(mjm.site_bodyid[obj]), np.asarray(mjm.site_pos[obj], dtype=dt)
    else:
      b, local = obj, data[3 * side:3 * side + 3]
    p.append(np.asarray(xpos[b], dtype=dt) + np.asarray(xmat[b], dtype=dt).reshape(3, 3) @ local)
  return p[0] - p[1]


def _connect_case(name):
  """[World] * NWORLD of part D.  Float64: connect_truth.Truth -- rows from finite differences of the oracle's kinematics, qacc from the closed
  form, every row an equality row; the smooth terms are the oracle's on the model without its connects, with qfrc_applied and xfrc_applied set.

  The float32 twin.  What a float32 engine cannot avoid on a connect row is the rounding of the GAP: p1 - p2 is the difference of two world
  positions of order 1 m, each known to a few ulp (6e-8), and aref = -k imp gap - b vel multiplies it by k = 1 / (dmax timeconst dampratio)^2,
  2770 / s^2 at the default solref; the force is D times that.  A twin that rounds the truth's finished rows keeps the gap's RELATIVE precision
  and misses this term altogether.  So the twin takes the body poses, M, qfrc_bias and qfrc_passive from RefSim(real="f32") of the stripped
  model, forms the gap from those poses in float32, vel = J qvel in float32, D and aref from connect_truth.efc_row at these values (rounded
  to float32), and evaluates force and J' force in float32.  J and Jdot qvel are the float64 finite differences rounded to float32 (a finite
  difference cannot be taken in float32): their own rounding in an engine, relative 1e-7 of entries of order 0.3, is not in the twin, which
  makes the bound tighter, not wider."""
  mjm = model(name)
  t = ct.Truth(mjm)
  s32 = ref.RefSim(t.stripped, nconmax=8, njmax=64, tolerance=1e-12, iterations=200, real="f32")
  scale = float(mjm.stat.meaninertia)
  refsafe = not (int(mjm.opt.disableflags) & (1 << 12))
  out = []
  for wi in range(NWORLD):
    rng = np.random.default_rng(4000 + wi)
    inp = {k: _f32(getattr(t.sim, k)) * 0.0 for k in _INPUTS}
    inp["qpos"] = _f32(ct.integrate_pos(mjm, FOURBAR_Q, 0.03 * rng.standard_normal(mjm.nv)))
    inp["qvel"] = _f32(0.7 * rng.standard_normal(mjm.nv))
    inp["qfrc_applied"] = _f32(rng.uniform(-1, 1, mjm.nv) * scale)
    inp["xfrc_applied"][1:] = _f32(rng.uniform(-1, 1, (mjm.nbody - 1, 6)) * scale)
    for s in (t.sim, s32):
      _load(s, inp)
    r = t.rows(inp["qpos"], inp["qvel"])
    jdv = np.concatenate([t.jac_dot_vel(inp["qpos"], inp["qvel"], e) for e in t.connects])
    qacc = t.qacc(inp["qpos"], inp["qvel"], rows=r)  # (one oracle forward of the stripped model at the state, applied forces included)
    s64 = t.sim
    ne = len(r["id"])
    rows = dict(J=r["J"], D=r["D"], aref=r["aref"], frictionloss=np.zeros(ne), nefc=ne, ne=ne, nf=0, nl=0, contacts=[], M=np.array(s64.dense_M()),
                qacc=qacc, **{k: np.array(getattr(s64, k)) for k in ("qfrc_bias", "qfrc_passive", "qfrc_smooth")})
    w = World()
    w.inputs, w.rows, w.qacc = inp, rows, _f32(qacc)
    w.want = evaluate(rows, qacc, float(mjm.opt.impratio))
    rows["qfrc_constraint"] = w.want["qfrc_constraint"]
    w.want["qfrc_inverse"] = rows["qfrc_smooth"] - rows["qfrc_passive"] + rows["qfrc_bias"]  # the applied force, from the oracle's own fields
    # the twin
    s32.forward()
    f = np.float32
    J32, D32, aref32 = r["J"].astype(f), np.zeros(ne, dtype=f), np.zeros(ne, dtype=f)
    for i, e in enumerate(t.connects):
      gap = _anchor_gap(mjm, e, s32.xpos, s32.xmat.reshape(-1, 3, 3), f)
      b = [int(x) for x in (mjm.eq_obj1id[e], mjm.eq_obj2id[e])]
      invweight = float(f(mjm.body_invweight0[b[0], 0]) + f(mjm.body_invweight0[b[1], 0]))
      for k in range(3):
        vel = J32[3 * i + k] @ inp["qvel"].astype(f)
        D, aref = ct.efc_row(float(mjm.opt.timestep), refsafe, float(gap[k]), float(np.sqrt(np.sum(gap * gap))), invweight,
                             np.asarray(mjm.eq_solref, dtype=f).reshape(-1, 2)[e], np.asarray(mjm.eq_solimp, dtype=f).reshape(-1, 5)[e], float(vel))
        D32[3 * i + k], aref32[3 * i + k] = f(D), f(aref) - f(jdv[3 * i + k])
    rows32 = dict(rows, J=J32, D=D32, aref=aref32, M=np.array(s32.dense_M(), dtype=f), qfrc_bias=np.array(s32.qfrc_bias), qfrc_passive=np.array(s32.qfrc_passive))
    w.rows32 = rows32
    w.twin = evaluate(rows32, w.qacc.astype(f), float(mjm.opt.impratio), f)
    w.jar_err = 0.0  # (equality rows have no zone boundary)
    out.append(w)
  return out


def twin_errors(worlds):
  """{field: worst scaled error of the float32 twin over the worlds}, and the share of rows whose twin state differs AFTER leaving out the rows
  within the twin's own jar error of a zone boundary."""
  err = {f: max(scaled_err(w.twin[f], w.want[f]) for w in worlds) for f in FIELDS}
  rows = sum(len(w.want["efc_state"]) for w in worlds)
  near = sum(int((w.want["margin"] <= w.jar_err).sum()) for w in worlds)
  bad = sum(int(((w.twin["efc_state"] != w.want["efc_state"]) & (w.want["margin"] > w.jar_err)).sum()) for w in worlds)
  return err, (near / rows if rows else 0.0), bad


def zones(worlds):
  """Coverage of part B: {"friction": states seen on friction-loss rows, 3 / 4 / 6: zones seen on elliptic contacts of that condim}."""
  seen = {"friction": set(), 3: set(), 4: set(), 6: set()}
  for w in worlds:
    r = w.rows
    seen["friction"] |= set(int(x) for x in w.want["efc_state"][r["ne"]:r["ne"] + r["nf"]])
    for c in r["contacts"]:
      if c["elliptic"] and c["dim"] in seen:
        seen[c["dim"]].add(int(w.want["efc_state"][c["r0"]]))
  return seen


def contact_row_map(rows, geom, pos, efc_address, dim):
  """Row permutation engine -> oracle: the engine may order contact rows differently; contacts are matched by geom pair (and, where a pair has
  several, by nearest position).  geom [ncon, 2], pos [ncon, 3], efc_address [ncon], dim [ncon]: the engine's contacts of the world.
  Returns perm with oracle_row = perm[engine_row] (identity on equality, friction and limit rows), or None if the contacts do not match."""
  perm = np.arange(rows["nefc"])
  free = list(rows["contacts"])
  for g, p, adr, dm in zip(geom, pos, efc_address, dim):
    if adr < 0:
      continue
    cands = [c for c in free if set(c["geom"]) == set(int(x) for x in g)]
    if not cands:
      return None
    best = min(cands, key=lambda c: float(np.linalg.norm(c["pos"] - p)))
    free.remove(best)
    for j in range(best["dim"]):
      if adr + j < rows["nefc"] and best["r0"] + j < rows["nefc"]:
        perm[adr + j] = best["r0"] + j
  return perm if not free else None


# ---- the float32 twin's recorded floors -------------------------------------------------------------------------------------------------
# python -m tests.inverse_truth   (CPU, a few seconds per model) prints this table: the twin's worst scaled error per field, per case.
# tests/test_inverse.py re-evaluates it (within a factor 2) and bounds the GPU by GPU_MARGIN x these figures.
TWIN = {
  ('pendula', 'A', True): (7.21e-07, 1.97e-06, 3.21e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('free_bodies', 'A', True): (3.30e-03, 1.56e-04, 2.06e-04),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('pile_pyramidal', 'A', True): (8.99e-04, 5.96e-05, 2.48e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('pile_elliptic', 'A', True): (7.57e-04, 3.63e-05, 1.57e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('humanoid', 'A', True): (8.85e-04, 9.00e-05, 6.03e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('panda', 'A', True): (1.49e-06, 4.88e-07, 4.88e-07),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('humanoids3', 'A', True): (5.69e-03, 4.05e-04, 2.14e-04),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain1', 'A', True): (6.27e-06, 5.80e-06, 5.67e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain15', 'A', True): (1.98e-05, 7.90e-06, 7.80e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain16', 'A', True): (1.61e-05, 1.28e-05, 1.26e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain17', 'A', True): (1.92e-05, 9.01e-06, 8.89e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain31', 'A', True): (5.63e-05, 6.21e-06, 6.15e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain32', 'A', True): (9.61e-05, 1.22e-05, 1.20e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain33', 'A', True): (6.33e-05, 8.04e-06, 8.02e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain63', 'A', True): (9.18e-05, 5.66e-06, 5.72e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain64', 'A', True): (8.40e-05, 6.23e-06, 6.18e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain65', 'A', True): (1.14e-04, 5.11e-06, 5.08e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('pile_elliptic', 'B', True): (3.79e-05, 5.44e-06, 3.53e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain1', 'B', True): (1.50e-07, 1.15e-07, 1.15e-07),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain15', 'B', True): (5.40e-06, 5.40e-06, 5.40e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain16', 'B', True): (1.15e-05, 1.31e-05, 1.29e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain17', 'B', True): (1.25e-05, 7.12e-06, 7.12e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain31', 'B', True): (5.27e-05, 5.74e-06, 5.68e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain32', 'B', True): (3.98e-05, 5.46e-06, 5.36e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain33', 'B', True): (1.44e-05, 5.44e-06, 5.23e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain63', 'B', True): (5.61e-05, 5.37e-06, 5.43e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain64', 'B', True): (6.37e-05, 4.09e-06, 4.13e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain65', 'B', True): (5.01e-05, 1.43e-06, 1.42e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain130', 'A', True): (8.22e-04, 4.37e-06, 4.34e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('chain130', 'B', True): (1.30e-04, 2.60e-06, 2.58e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('fourbar', 'D', True): (8.60e-04, 3.76e-04, 4.14e-04),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('humanoid', 'C', True): (9.01e-04, 9.16e-05, 6.03e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('humanoid', 'C', False): (8.85e-04, 9.00e-05, 6.03e-05),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('pendula', 'C', True): (5.36e-07, 1.92e-06, 3.12e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
  ('pendula', 'C', False): (7.21e-07, 1.97e-06, 3.21e-06),  # near-boundary rows 0.000%, twin state mismatches beyond them 0
}


def all_cases():
  keys = [(n, "A", True) for n in MODELS] + [(n, "B", True) for n in ("pile_elliptic",) + tuple(f"chain{k}" for k in CHAIN_NV) + (BIG_CHAIN,)]
  return keys + [(n, "C", e) for n in ("humanoid", "pendula") for e in (True, False)] + [("fourbar", "D", True)]


if __name__ == "__main__":
  for key in all_cases():
    err, near, bad = twin_errors(case(*key))
    print(f"  {key!r}: ({err['qfrc_inverse']:.2e}, {err['qfrc_constraint']:.2e}, {err['efc_force']:.2e}),  # near-boundary rows {near:.3%}, twin state mismatches beyond them {bad}")
