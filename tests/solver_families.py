"""The smallest scene of the suite that reaches each solver mapping (`mjw.solver_kernel`), in a state with active contacts.

A plain helper module like tree_models.py, shared by tests/test_gpu.py (the shared line-search loop is live in every mapping) and
tools/solver_family_ab.py (bitwise A/B of two builds, one scene per mapping).  `CASES` maps a case name to (family, builder, knobs); `device(case)`
returns (family, mjm, m, d, knobs) with `d` warmed up by the engine's own steps from the state the family's existing tests start from: the
humanoid's and the G1's keyframe 0 under the benchmark's control noise, test_elliptic.py's sliding keyframe, the three-humanoid batch of
test_constraint_islands_nv81 (apart / two touching / all three touching: 32-lane islands, a 64-lane island, the generic solver),
test_clutter.py's scene, the mixed elliptic case of the constraint sweep at 64 lanes, and for "big" (nv > 64 in one kinematic tree: no
per-island solve, csrc/solver_big.hpp alone) the 65-hinge chain of inverse_truth.py, every joint limited and with friction loss, thrown
past its limits.
"""

import os

import numpy as np

import mujoco_warp_amd as mjw

_TESTS = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_TESTS)
_HUMANOID = os.path.join(_ROOT, "benchmarks", "humanoid", "humanoid.xml")
_G1 = os.path.join(_ROOT, "benchmarks", "unitree_g1", "scene_flat.xml")
_CLUTTER = os.path.join(_TESTS, "models", "clutter_synth.xml")
CG, NEWTON = int(mjw.SolverType.CG), int(mjw.SolverType.NEWTON)


def _humanoid(solver):
  mjm = mjw.mjcf.load_xml(_HUMANOID)
  mjm.opt.solver = solver
  return dict(mjm=mjm, nconmax=24, njmax=64, warm=28)  # (landing: 36 rows, searches of several rounds in all four mappings)


def _elliptic(solver, condim=3):
  from test_elliptic import ELLIPTIC_XML

  mjm = mjw.mjcf.from_xml_string(ELLIPTIC_XML.format(condim=condim))
  mjm.opt.solver = solver
  if solver == CG:
    mjm.opt.iterations = 200  # (as test_gpu_elliptic_matches_oracle: CG on these cone scenes takes up to ~90 iterations)
  return dict(mjm=mjm, nconmax=32, njmax=128, warm=10)


def _g1(solver):
  mjm = mjw.mjcf.load_xml(_G1)
  mjm.opt.solver = solver
  return dict(mjm=mjm, nconmax=48, njmax=192, warm=24)


def _mix64_ell(solver):
  import constraint_models as cm

  mjm = mjw.mjcf.from_xml_string(cm.constraint_xml("g64_mix_ell"))
  mjm.opt.solver = solver
  mjm.opt.iterations, mjm.opt.ls_iterations = 100, 50
  st = [cm.world_state("g64_mix_ell", mjm, w) for w in (0, 3)]  # the worlds whose counts the case's name states

  def state(m, d):
    for f in ("qpos", "qvel"):
      getattr(d, f).assign(np.array([st[w % 2][f] for w in range(d.nworld)], dtype=np.float32))
    if mjm.neq:
      d.eq_active.assign(np.array([st[w % 2]["eq_active"] for w in range(d.nworld)], dtype=np.int32))

  return dict(mjm=mjm, nconmax=16, njmax=192, warm=3, state=state)


def _three_humanoids(solver):
  import conftest

  mjm = mjw.mjcf.from_xml_string(conftest.multi_humanoid_xml(3), assets_dir=os.path.dirname(_HUMANOID))
  mjm.opt.solver = solver

  def state(m, d):  # world w % 3: 0 apart, 1 the second humanoid moved onto the first, 2 the third onto both
    q = d.qpos.numpy()
    for w in range(d.nworld):
      if w % 3 >= 1:
        q[w, 28:31] = q[w, 0:3] + np.array([0.12, 0.05, 0.0], dtype=np.float32)
      if w % 3 == 2:
        q[w, 56:59] = q[w, 0:3] + np.array([-0.1, -0.05, 0.0], dtype=np.float32)
    d.qpos.assign(q)

  return dict(mjm=mjm, nconmax=100, njmax=192, warm=30, state=state, nworld=3)


def _chain65(solver):
  from inverse_truth import chain_xml

  mjm = mjw.mjcf.from_xml_string(chain_xml(65))
  mjm.opt.solver = solver

  def state(m, d):  # seeded: a third of the joints beyond their +-20 degree range, every dof moving (friction-loss rows in all three zones)
    rng = np.random.default_rng(65)
    d.qpos.assign((0.3 * rng.standard_normal((d.nworld, mjm.nq))).astype(np.float32))
    d.qvel.assign(rng.standard_normal((d.nworld, mjm.nv)).astype(np.float32))

  return dict(mjm=mjm, nconmax=8, njmax=160, warm=3, state=state)


def _clutter(solver):
  mjm = mjw.mjcf.load_xml(_CLUTTER)
  mjm.opt.enableflags = 0  # (test_gpu_elliptic_islands_without_sleep: the per-island elliptic solves without the sleep machinery)
  mjm.opt.solver = solver
  if solver == CG:
    mjm.opt.iterations, mjm.opt.ls_iterations = 200, 50
  return dict(mjm=mjm, nconmax=256, njmax=384, warm=60, nworld=2)


# name: (family that mjw.solver_kernel must report, builder, developer knobs)
CASES = {
  "cgp": ("cgp", lambda: _humanoid(CG), dict(MJH_CG_KERNEL="cgp")),
  "cgw": ("cgw", lambda: _humanoid(CG), dict(MJH_CG_KERNEL="cgw")),
  "pair": ("pair", lambda: _humanoid(CG), dict(MJH_CG_KERNEL="pair")),
  "newton_mfma": ("newton_mfma", lambda: _humanoid(NEWTON), {}),
  "cg32_ell": ("cg32_ell", lambda: _elliptic(CG), {}),
  "newton32_ell": ("newton32_ell", lambda: _elliptic(NEWTON), {}),
  "cg64": ("cg64", lambda: _g1(CG), {}),
  "newton64": ("newton64", lambda: _g1(NEWTON), {}),
  "cg64_ell": ("cg64_ell", lambda: _mix64_ell(CG), {}),
  "newton64_ell": ("newton64_ell", lambda: _mix64_ell(NEWTON), {}),
  "tree+big-cg": ("tree+big", lambda: _three_humanoids(CG), {}),
  "tree+big-newton": ("tree+big", lambda: _three_humanoids(NEWTON), {}),
  "tree+big-ell-cg": ("tree+big", lambda: _clutter(CG), {}),
  "tree+big-ell-newton": ("tree+big", lambda: _clutter(NEWTON), {}),
  "big-cg": ("big", lambda: _chain65(CG), {}),
  "big-newton": ("big", lambda: _chain65(NEWTON), {}),
}
# scenes of the bitwise A/B beyond the smallest one per family: the other condims of test_elliptic.py
AB_EXTRA = {
  f"{fam}-condim{c}": (fam, (lambda s=s, c=c: _elliptic(s, c)), {}) for fam, s in (("cg32_ell", CG), ("newton32_ell", NEWTON)) for c in (4, 6)
}


def device(case, nworld=4, warm=None):
  """(family, mjm, m, d, knobs) of a case: `d` holds `nworld` worlds (the case's own count where it fixes one) after the case's warm-up steps,
  taken with `knobs` set."""
  from mujoco_warp_amd import _abi

  family, build, knobs = {**CASES, **AB_EXTRA}[case]
  c = build()
  mjm = c["mjm"]
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=c.get("nworld", nworld), nconmax=c["nconmax"], njmax=c["njmax"])
  if mjm.nkey:
    mjw.reset_data_keyframe(m, d, 0)
  if "state" in c:
    c["state"](m, d)
  with _abi.dev_knobs(**knobs):
    for i in range(c["warm"] if warm is None else warm):
      if mjm.nu:
        mjw.ctrl_noise(m, d, i)
      mjw.step(m, d)
  return family, mjm, m, d, knobs
