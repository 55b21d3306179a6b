"""The smooth-dynamics kernels (csrc/smooth.hpp) over tree shapes and lane-class edges: every case of tests/tree_models.py, 19 worlds in 19
different states, every world against its own float64 oracle run, field by field and row by row -- through `forward` (k_fwd_pos + the
velocity role of k_mid) and through the stage API (k_fwd_pos / k_fwd_vel / k_factor_smooth, k_solve_m).

One comparison function (`compare`) serves the GPU tests and the CPU twin test, which feeds it the float32 build of the oracle in place of
the device and divides every bound by 4: a case the float32 restatement of the algorithm cannot resolve to a quarter of a bound says nothing
about a kernel, and has to change (armature, masses, chain length), not the bound.

Bounds
  whole field   conftest.relerr <= SMOOTH (2e-5), factor fields (qLD, qLDiagInv, qacc_smooth) <= FACTOR (1e-4): test_gpu.py's figures
  per row       max|d row| <= tol x max(max|oracle row|, floor x max|oracle field|), tol as above; a row is a body / dof / joint / geom /
                site / actuator, for M and qLD the CSR row of a dof.  FLOOR per field class, started at 1e-3 and raised only as far as the
                twin needs with its factor 4.  In brackets the smallest floor at which the twin's worst row -- over all cases, worlds and
                fields of the class -- meets bound / 4, and the case that sets it (0: every row meets it relative to its own maximum):
                  pose    1e-3  (0)                poses of bodies, joints, geoms and sites, subtree_com
                  spatial 1e-3  (0)                cinert, crb, cdof, cdof_dot, cvel, cacc, cfrc_int
                  inertia 1e-3  (0)                M, as CSR rows and as rows of the dense symmetric matrix
                  force   1.3e-1  (1.18e-1, deep; 9e-2 l16_body, 7e-2 l32_dof)   generalised and actuator forces, actuator lengths and velocities
                  factor  6e-2    (5.5e-2, deep; 2e-2 l64_in)                    qLD, qLDiagInv, qacc_smooth, under FACTOR
                A generalised force is a sum over a subtree in which terms cancel, and a row of M^-1 mixes every dof: an entry far below the
                field's maximum carries the field's absolute error, not its own relative one.  (Figures: profiles/smooth_sweep.txt; the tests
                print them again with -s.)
  backward      from the outputs under test alone, in float64 on the host, every case: max|L'DL - M| / max|M|, max|M qacc_smooth - qfrc_smooth| /
                max|qfrc_smooth|, max|M solve_m(y) - y| / max|y| and max|mul_m(x) - M x| / max|M x|, each <= FACTOR (the twin's worst over all cases: 1.0e-5, solve_m
                on `big`).  The stage path holds two factors, the `factor_m` stage's and the 32-lane factor kernel's: each gets the forward
                comparison and its own L'DL residual
  A factor field whose twin error exceeds FACTOR / 4 (cond(M) of a long chain) is not compared forward in that case: the backward checks
  stand in for it.  `factor_branch` decides that from the twin alone; at most `deep` and `big` may take it (asserted).
"""

import functools

import numpy as np
import pytest

import mujoco_warp_amd as mjw
import tree_models as tm
from conftest import relerr
from mujoco_warp_amd import _npmath as nm
from mujoco_warp_amd import io
from oracle import ref
from test_gpu import _SMOOTH_FIELDS, FACTOR, SMOOTH

NWORLD = 19  # more than one workgroup at every worlds-per-workgroup count the launchers choose (1 .. 16), the last one partial: 19 is prime
FLOOR = {"pose": 1e-3, "spatial": 1e-3, "inertia": 1e-3, "force": 1.3e-1, "factor": 6e-2}
_CLASS = dict(
  xpos="pose", xquat="pose", xmat="pose", xipos="pose", ximat="pose", xanchor="pose", xaxis="pose", geom_xpos="pose", geom_xmat="pose",
  subtree_com="pose", site_xpos="pose", site_xmat="pose", cinert="spatial", cdof="spatial", crb="spatial", cvel="spatial", cdof_dot="spatial",
  cacc="spatial", cfrc_int="spatial", M="inertia", qfrc_spring="force", qfrc_damper="force", qfrc_gravcomp="force", qfrc_passive="force",
  qfrc_bias="force", actuator_length="force", actuator_velocity="force", actuator_force="force", qfrc_actuator="force", qfrc_smooth="force",
  qLD="factor", qLDiagInv="factor", qacc_smooth="factor")
FIELDS = tuple(_SMOOTH_FIELDS) + ("qfrc_gravcomp", "actuator_length", "actuator_velocity", "qLD", "qLDiagInv", "qacc_smooth", "site_xpos", "site_xmat")
assert set(FIELDS) == set(_CLASS)
# the stage API, stage by stage, with what each stage writes (csrc/mjhip.hip mjh_stage; actuator_velocity comes with com_vel, the length with the force)
STAGES = (
  ("kinematics", ("xpos", "xquat", "xmat", "xipos", "ximat", "xanchor", "xaxis", "geom_xpos", "geom_xmat", "site_xpos", "site_xmat")),
  ("com_pos", ("subtree_com", "cinert", "cdof")),
  ("crb", ("crb", "M")),
  ("factor_m", ("qLD", "qLDiagInv")),
  ("com_vel", ("cvel", "cdof_dot", "actuator_velocity")),
  ("passive", ("qfrc_spring", "qfrc_damper", "qfrc_gravcomp", "qfrc_passive")),
  ("rne", ("qfrc_bias", "cacc", "cfrc_int")),
  ("fwd_actuation", ("actuator_length", "actuator_force", "qfrc_actuator")),
  ("fwd_acceleration", ("qfrc_smooth", "qacc_smooth")),
)
assert sorted(f for _, fs in STAGES for f in fs) == sorted(FIELDS)


@functools.lru_cache(maxsize=None)
def model(case):
  return mjw.mjcf.from_xml_string(tm.tree_xml(case))


@functools.lru_cache(maxsize=None)
def states(case):
  """qpos / qvel / ctrl / act / a right-hand side for solve_m, [NWORLD, n] each, every world different: qpos0 plus seeded noise (quaternions
  perturbed and normalised), seeded velocities, controls and activations; float32-exact values, so that the oracle and the device read the same
  numbers.  World 3's free and ball quaternions are scaled by 1.7 (both sides normalise on load), world 7 is at rest."""
  mjm = model(case)
  r = np.random.default_rng(1000 + tm.CASES[case]["seed"])
  qpos = np.tile(np.asarray(mjm.qpos0, dtype=np.float64), (NWORLD, 1))
  for w in range(NWORLD):
    for j in range(mjm.njnt):
      t, a = int(mjm.jnt_type[j]), int(mjm.jnt_qposadr[j])
      if t == 0:
        qpos[w, a : a + 3] += 0.1 * r.standard_normal(3)
        a += 3
      if t in (0, 1):
        q = qpos[w, a : a + 4] + 0.4 * r.standard_normal(4)
        qpos[w, a : a + 4] = q / np.linalg.norm(q) * (1.7 if w == 3 else 1.0)
      else:
        qpos[w, a] += (0.05 if t == 2 else 0.5) * r.standard_normal()
  qvel = 0.5 * r.standard_normal((NWORLD, mjm.nv))
  qvel[7] = 0.0
  out = dict(qpos=qpos, qvel=qvel, ctrl=r.uniform(-1, 1, (NWORLD, mjm.nu)), act=r.uniform(-1, 1, (NWORLD, mjm.na)), rhs=r.standard_normal((NWORLD, mjm.nv)))
  return {k: v.astype(np.float32).astype(np.float64) for k, v in out.items()}


def site_frames(mjm, xpos, xquat):
  """site_xpos / site_xmat of one world in float64 from body poses (the oracle keeps no site fields)."""
  pos = np.array([xpos[b] + nm.rot_vec_quat(np.asarray(p, dtype=np.float64), xquat[b]) for b, p in zip(mjm.site_bodyid, mjm.site_pos)]).reshape(-1, 3)
  mat = np.array([nm.quat_to_mat(nm.quat_normalize(nm.quat_mul(xquat[b], np.asarray(q, dtype=np.float64)))) for b, q in zip(mjm.site_bodyid, mjm.site_quat)]).reshape(-1, 9)
  return pos, mat


@functools.lru_cache(maxsize=None)
def oracle_run(case, real="f64"):
  """Every field of FIELDS, [NWORLD, ...] in float64, from one oracle `forward` per world (real="f32": the float32 twin), with the twin's own
  solve_m(rhs) and mul_m(solve_m(rhs)).  Computed once per case and shared by every test; callers do not write to it."""
  mjm, st = model(case), states(case)
  s = ref.RefSim(mjm, nconmax=8, njmax=16, real=real)
  out = {k: [] for k in FIELDS + ("solve_m", "mul_m")}
  for w in range(NWORLD):
    for k in ("qpos", "qvel", "ctrl", "act"):
      if st[k].shape[1]:
        getattr(s, k)[:] = st[k][w]
    s.forward()
    assert s.nefc == 0 and s.ncon == 0
    sp, sm = site_frames(mjm, np.asarray(s.xpos, dtype=np.float64), np.asarray(s.xquat, dtype=np.float64))
    x = s.solve_m(st["rhs"][w])
    for k in out:
      v = sp if k == "site_xpos" else sm if k == "site_xmat" else x if k == "solve_m" else s.mul_m(x) if k == "mul_m" else getattr(s, k)
      out[k].append(np.array(v, dtype=np.float64))
  return {k: np.array(v) for k, v in out.items()}


def dense_m(mjm, M):
  """[nv, nv] symmetric from one world's CSR rows (lower triangle: the ancestors of a dof, then the dof itself)."""
  D = np.zeros((mjm.nv, mjm.nv))
  for i in range(mjm.nv):
    a, n = int(mjm.M_rowadr[i]), int(mjm.M_rownnz[i])
    D[i, mjm.M_colind[a : a + n]] = M[a : a + n]
  return D + np.tril(D, -1).T


def dense_ld(mjm, qLD):
  """(unit lower triangular L, diagonal D) of M = L' D L from one world's qLD: the CSR layout of M, D on the diagonal."""
  L = np.tril(dense_m(mjm, qLD))
  D = np.diag(L).copy()
  np.fill_diagonal(L, 1.0)
  return L, D


def _rowmax(mjm, name, x):
  """max|.| per row of one world's field: axis 0 of a [rows, k] field, the elements of a [rows] field, the CSR rows of M / qLD."""
  x = np.abs(x)
  if name in ("M", "qLD"):
    return np.maximum.reduceat(x, np.asarray(mjm.M_rowadr, dtype=np.int64))
  return x.reshape(x.shape[0], -1).max(axis=1) if x.size else x.reshape(0)


def backward(mjm, got, w):
  """The four residuals of the header from one world's outputs (solve_m / mul_m: when `got` has them)."""
  M = dense_m(mjm, got["M"][w])
  L, D = dense_ld(mjm, got["qLD"][w])
  res = {"L'DL-M": np.abs(L.T @ np.diag(D) @ L - M).max() / np.abs(M).max(),
         "M.qacc-qfrc": np.abs(M @ got["qacc_smooth"][w] - got["qfrc_smooth"][w]).max() / np.abs(got["qfrc_smooth"][w]).max()}
  for k in got:  # a second version of the factor ("qLD|k_factor_smooth": see compare)
    if k.startswith("qLD|"):
      L, D = dense_ld(mjm, got[k][w])
      res["L'DL-M|" + k[4:]] = np.abs(L.T @ np.diag(D) @ L - M).max() / np.abs(M).max()
  if "solve_m" in got:
    x, y = got["solve_m"][w], got["rhs"][w]
    res["M.solve_m(y)-y"] = np.abs(M @ x - y).max() / np.abs(y).max()
    res["mul_m(x)-M.x"] = np.abs(got["mul_m"][w] - M @ x).max() / np.abs(M @ x).max()
  return res


def compare(case, path, got, want, div=1.0, skip=()):
  """(failures, figures): `got` (the device's fields, or the twin's) against the oracle's `want`, [NWORLD, ...] each, under the header's bounds
  divided by `div`.  skip: the factor fields whose forward comparison the backward checks replace (factor_branch).  A failure names case, path,
  world, field and row.  figures: per field class the worst whole-field error, the worst row as a fraction of its bound and the floor that row
  would need; the worst backward residuals."""
  mjm = model(case)
  fails = []
  fig = {c: dict(whole=0.0, row=0.0, floor=0.0) for c in FLOOR}
  fig["backward"], fig["writers"] = {}, {}  # (writers: the whole-field error of every factor field, one entry per kernel that wrote it)
  for w in range(NWORLD):
    fields = [(name, got[name][w], want[name][w]) for name in FIELDS if name not in skip]
    # "field|kernel": the same field as a second kernel wrote it (the stage path keeps qLD / qLDiagInv of both kernels that publish them)
    fields += [(name, got[name][w], want[name.split("|")[0]][w]) for name in got if "|" in name and name.split("|")[0] not in skip]
    fields.append(("dense M", dense_m(mjm, got["M"][w]), dense_m(mjm, want["M"][w])))
    for name, g, o in fields:
      cls = _CLASS.get(name.split("|")[0], "inertia")
      tol = (FACTOR if cls == "factor" else SMOOTH) / div
      g = np.asarray(g, dtype=np.float64).reshape(o.shape)
      if not np.isfinite(g).all():
        fails.append(f"{case} {path} world {w} {name}: not finite")
        continue
      if o.size == 0:
        continue
      e = relerr(g, o)
      fig[cls]["whole"] = max(fig[cls]["whole"], e)
      if cls == "factor":
        fig["writers"][name] = max(fig["writers"].get(name, 0.0), e)
      if e > tol:
        fails.append(f"{case} {path} world {w} {name}: whole-field error {e:.3e} > {tol:.1e}")
      base = name.split("|")[0]
      drow, orow, fmax = _rowmax(mjm, base, g - o), _rowmax(mjm, base, o), np.abs(o).max()
      bound = tol * np.maximum(orow, FLOOR[cls] * fmax)
      with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(drow > 0, drow / bound, 0.0)  # (a field that is zero throughout -- world 7's velocities -- must be exactly so)
        need = np.where(drow > tol * orow, drow / (tol * fmax), 0.0)
      i = int(np.argmax(frac))
      fig[cls]["row"] = max(fig[cls]["row"], float(frac[i]))
      fig[cls]["floor"] = max(fig[cls]["floor"], float(need.max()))
      if frac[i] > 1:
        fails.append(f"{case} {path} world {w} {name} row {i}: |d| {drow[i]:.3e} > {bound[i]:.3e} (row max {orow[i]:.3e}, field max {fmax:.3e})")
    for k, v in backward(mjm, got, w).items():
      fig["backward"][k] = max(fig["backward"].get(k, 0.0), float(v))
      if not v <= FACTOR / div:
        fails.append(f"{case} {path} world {w} backward {k}: {v:.3e} > {FACTOR / div:.1e}")
  return fails, fig


def summary(case, path, fig, skip):
  cls = "  ".join(f"{c} {fig[c]['whole']:.1e}/{fig[c]['row']:.2f}/{max(fig[c]['floor'], 0):.0e}" for c in FLOOR)
  back = " ".join(f"{k} {v:.1e}" for k, v in fig["backward"].items())
  if any("|" in k for k in fig["writers"]):  # the stage path: qLD / qLDiagInv of factor_m (k_fwd_pos) and of the factor kernel, apart
    back += "  factor fields: " + " ".join(f"{k} {v:.1e}" for k, v in fig["writers"].items())
  return f"{case:10s} {path:6s} [whole/row fraction/floor needed] {cls}  backward: {back}  lanes (k_fwd_pos and its factor_m, k_fwd_vel, k_mid, k_factor_smooth / k_solve_m) {tm.lane_groups(model(case).nbody, model(case).nv)}" + (f"  BACKWARD ONLY: {sorted(skip)}" if skip else "")


@functools.lru_cache(maxsize=None)
def factor_branch(case):
  """The factor fields of a case that float32 cannot resolve forward: those whose twin error exceeds FACTOR / 4 in some world."""
  twin, want = oracle_run(case, "f32"), oracle_run(case)
  return frozenset(f for f in ("qLD", "qLDiagInv", "qacc_smooth") if max(relerr(twin[f][w], want[f][w]) for w in range(NWORLD)) > FACTOR / 4)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", list(tm.CASES))
def test_case_has_its_sizes_and_properties(case):
  cfg = tm.CASES[case]
  xml = tm.tree_xml(case)
  assert xml == tm.tree_xml(case) and xml == tm.tree_xml(dict(cfg))  # deterministic
  mjm = model(case)
  assert (mjm.nbody, mjm.nv) == (cfg["nbody"], cfg["nv"])
  facts, tab = io._tree_tables(mjm)
  jt = np.asarray(mjm.jnt_type)
  stacks = [tuple(int(t) for t in jt[a : a + n]) for a, n in zip(mjm.body_jntadr, mjm.body_jntnum) if n > 0]
  assert mjm.nu % 2 == 1 and mjm.na == 1 and not io._actuator_facts(mjm)[0]["trn_general"]
  assert int(np.sum(np.asarray(mjm.body_gravcomp) != 0)) >= (mjm.nbody - 1) // 3 and int(np.sum(mjm.jnt_actgravcomp)) == 1
  assert mjm.nsite >= (mjm.nbody - 1) // 3 and mjm.ngeom > mjm.nbody - 1 and max(mjm.body_jntnum) <= 4
  assert (np.asarray(mjm.jnt_stiffness)[jt >= 2] != 0).any()
  assert set(int(t) for t in mjm.geom_type) <= {2, 3}  # spheres and capsules: the light collision instantiation, which leaves the lane choice to the sizes
  if not cfg.get("one_joint"):
    assert (2, 2, 3) in stacks and (np.asarray(mjm.body_jntnum)[1:] == 0).any()
    ball = np.flatnonzero(jt == 1)
    assert len(ball) and (np.abs(np.asarray(mjm.jnt_pos)[ball]).max(axis=1) > 0).all() and (np.asarray(mjm.jnt_stiffness)[ball] != 0).any()
    assert (np.asarray(mjm.jnt_stiffness)[jt == 0] != 0).any() == (jt == 0).any()
  pos_g, vel_g, mid_g, fac_g = tm.lane_groups(mjm.nbody, mjm.nv)
  want_lanes = dict(l16_in=(32, 32, 16), l16_body=(32, 32, 32), l16_dof=(32, 32, 32), l32_in=(32, 32, 32), l32_body=(64, 64, 64), l32_dof=(32, 64, 64),
                    l64_in=(64, 64, 64), l64_body=(64, 64, 64), l64_dof=(64, 64, 64))
  if case in want_lanes:
    assert (pos_g, vel_g, mid_g) == want_lanes[case]
  nword = (mjm.nv + 31) // 32
  assert tab["body_dofmask"].shape == (mjm.nbody, nword)
  if case in ("l32_dof", "l64_in", "l64_dof", "big"):
    assert nword == dict(l32_dof=2, l64_in=2, l64_dof=3, big=5)[case] and tab["body_dofmask"][:, -1].any()
    gc = np.flatnonzero(np.asarray(mjm.body_gravcomp) != 0)
    assert tab["body_dofmask"][gc, -1].any()  # a compensated body hangs below a dof of the last mask word
  if case == "wide":
    assert int(np.diff(tab["body_leveladr"]).max()) == 70 > pos_g and int(tab["body_subtreenum"][1]) == 71
  if case == "deep":
    assert facts["nbodylevel"] == 41 and int(np.max(mjm.M_rownnz)) == 40 > fac_g
  if case == "big":
    assert mjm.nbody > 64 and mjm.nv > 128 and mjm.ngeom > 64 and mjm.njnt > 64 and mjm.nsite > 32
  if case.startswith("forest"):
    # the two kernels that factor: k_fwd_pos (the `factor_m` stage) and the 32-lane factor kernel.  forest_par: 64 and 32 lanes, true in both;
    # forest_seq (21 bodies): both run with 32 lanes, one evaluation -- at 64 lanes the formula would be false for it as well (30 < 36)
    par = {G: tm.ld_by_tree(facts["ntree"], facts["tree_nvmax"], mjm.nv, G) for G in (pos_g, fac_g)}
    assert facts["ntree"] == len(cfg["trees"]) > 1 and facts["tree_nvmax"] == max(nd for _, nd in cfg["trees"])
    assert (sorted(par) == [32, 64] and all(par.values())) if case == "forest_par" else (sorted(par) == [32] and not any(par.values()))
    assert case == "forest_par" or not tm.ld_by_tree(facts["ntree"], facts["tree_nvmax"], mjm.nv, 64)
  elif cfg["shape"] != "forest":
    assert facts["ntree"] == 1


def test_generator_shapes_outside_the_table():
  """Every shape at sizes the table does not use: exact counts, and the tree the shape names."""
  for shape, nbody, nv in (("comb", 22, 27), ("chain", 9, 14), ("star", 12, 12), ("random", 40, 31)):
    mjm = mjw.mjcf.from_xml_string(tm.tree_xml(dict(shape=shape, nbody=nbody, nv=nv, seed=5)))
    assert (mjm.nbody, mjm.nv) == (nbody, nv)
    parent = [int(p) for p in mjm.body_parentid[1:]]
    if shape == "comb":  # vertebra k is body 2 k + 1 and hangs on vertebra k - 1, its leaf is the next body
      assert parent == [max(b - 2, 0) if b % 2 else b - 1 for b in range(1, nbody)]
    elif shape == "chain":
      assert parent == list(range(nbody - 1))
    elif shape == "star":
      assert parent == [0] + [1] * (nbody - 2)


def test_states_differ_in_every_world():
  for case in ("l16_in", "forest_seq"):
    st, mjm = states(case), model(case)
    assert len({tuple(q) for q in st["qpos"]}) == NWORLD and (st["qvel"][7] == 0).all() and (np.abs(st["qvel"]).max(axis=1) > 0).sum() == NWORLD - 1
    a = int(mjm.jnt_qposadr[np.flatnonzero(np.asarray(mjm.jnt_type) == 1)[0]])
    n = np.linalg.norm(st["qpos"][:, a : a + 4], axis=1)
    assert abs(n[3] - 1.7) < 1e-6 and np.abs(np.delete(n, 3) - 1).max() < 1e-6


@pytest.mark.parametrize("case", list(tm.CASES))
def test_float32_twin_resolves_the_case_with_margin(case):
  """The GPU test's comparison with every bound divided by 4, on the float32 build of the oracle: what keeps the GPU test honest."""
  want = oracle_run(case)
  got = dict(oracle_run(case, "f32"), rhs=states(case)["rhs"])
  skip = factor_branch(case)
  assert not skip or case in ("deep", "big"), (case, skip)
  fails, fig = compare(case, "twin", got, want, div=4.0, skip=skip)
  print(summary(case, "twin", fig, skip))
  assert not fails, "\n".join(fails[:20])


def test_backward_residual_convention():
  """dense_m / dense_ld restate the layouts correctly: the float64 oracle's own outputs leave residuals at rounding level."""
  for case in ("l16_in", "forest_par"):
    want = dict(oracle_run(case), rhs=states(case)["rhs"])
    for w in (0, 7):
      assert max(backward(model(case), want, w).values()) < 1e-12


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------


def _device(case):
  mjm, st = model(case), states(case)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=NWORLD, nconmax=8, njmax=16)
  for k in ("qpos", "qvel", "ctrl", "act"):
    if st[k].shape[1]:
      getattr(d, k).assign(st[k].astype(np.float32))
  return mjm, m, d


def _fetch(d, names):
  return {k: getattr(d, k).numpy().astype(np.float64) for k in names}


def _check(case, path, got):
  skip = factor_branch(case)
  assert not skip or case in ("deep", "big"), (case, skip)
  fails, fig = compare(case, path, got, oracle_run(case), skip=skip)
  print(summary(case, path, fig, skip))
  assert not fails, "\n".join(fails[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(tm.CASES))
def test_forward_matches_oracle_in_every_world(case):
  """The product path: `forward` (k_fwd_pos, then the velocity role of k_mid at the case's lane count)."""
  mjm, m, d = _device(case)
  facts, _ = io._tree_tables(mjm)
  assert (m.nbodylevel, m.ntree, m.tree_nvmax) == (facts["nbodylevel"], facts["ntree"], facts["tree_nvmax"]) and not m.heavy_colliders and not m.trn_general
  mjw.forward(m, d)
  assert (d.nefc.numpy() == 0).all() and (d.overflow.numpy() == 0).all()
  _check(case, "forward", _fetch(d, FIELDS))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(tm.CASES))
def test_stage_api_matches_oracle_in_every_world(case):
  """The stage API: every stage on its own launch, its outputs poisoned first and fetched straight after it; then solve_m and mul_m on a
  right-hand side per world.  qLD / qLDiagInv have two writers: `factor_m` (k_fwd_pos: factor_ld at that kernel's lane count, 64 above 32 bodies --
  the only place that instantiation's factor is visible) and, overwriting them, `fwd_acceleration` (the 32-lane factor kernel).  Both are compared:
  factor_m's as "qLD" / "qLDiagInv", the later ones as "qLD|k_factor_smooth" / "qLDiagInv|k_factor_smooth", each with its own L'DL residual."""
  mjm, m, d = _device(case)
  got = {}
  for fn, fields in STAGES:
    for name in fields + (("qLD", "qLDiagInv") if fn == "fwd_acceleration" else ()):
      getattr(d, name).fill_(float("inf"))
    getattr(mjw, fn)(m, d)
    got.update(_fetch(d, fields))
  got.update({k + "|k_factor_smooth": v for k, v in _fetch(d, ("qLD", "qLDiagInv")).items()})
  y = states(case)["rhs"].astype(np.float32)
  ya, xa, ra = mjw.DeviceArray.from_numpy(y), mjw.DeviceArray.zeros(y.shape), mjw.DeviceArray.zeros(y.shape)
  mjw.solve_m(m, d, xa, ya)
  mjw.mul_m(m, d, ra, xa)
  got.update(rhs=y.astype(np.float64), solve_m=xa.numpy().astype(np.float64), mul_m=ra.numpy().astype(np.float64))
  _check(case, "stages", got)
