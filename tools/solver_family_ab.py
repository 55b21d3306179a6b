"""Bitwise A/B of two builds over one scene per solver mapping (tests/solver_families.py: CASES + AB_EXTRA).

  python tools/solver_family_ab.py dump <out.npz>          (MJH_LIB selects the library, as in tools/ab_lib.sh; one process per library)
  python tools/solver_family_ab.py compare <a.npz> <b.npz>

dump: per scene, the warm-up steps of the helper module and then 20 steps; qacc, qfrc_constraint, efc.force, efc.state, solver_niter, overflow,
qpos and qvel at the end, the mapping `solver_kernel` reports, and the same 20 steps again from the same warmed-up state with
opt.ls_iterations = 1.  compare: numpy.array_equal of every field between the two dumps, and per scene whether the ls_iterations = 1 run
changed the compared fields (a scene whose line searches all end at the Newton point would prove nothing about the bracketing loop).
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

FIELDS = ("qacc", "qfrc_constraint", "efc.force", "efc.state", "solver_niter", "overflow", "qpos", "qvel")
NSTEP = 20


def _get(d, f):
  o = d
  for part in f.split("."):
    o = getattr(o, part)
  return o.numpy().copy()


def dump(path):
  import mujoco_warp_amd as mjw
  import solver_families as sf
  from mujoco_warp_amd._abi import dev_knobs

  out = {}
  for case in list(sf.CASES) + list(sf.AB_EXTRA):
    family, mjm, m, d, knobs = sf.device(case)
    state = {f: getattr(d, f).numpy().copy() for f in ("qpos", "qvel", "qacc_warmstart", "ctrl", "act", "time") if getattr(d, f).size}
    with dev_knobs(**knobs):
      out[f"{case}/family"] = np.array(mjw.solver_kernel(m, d) + ("" if mjw.solver_kernel(m, d) == family else f" (expected {family})"))
      for tag, ls in (("", int(mjm.opt.ls_iterations)), ("ls1/", 1)):
        m.opt.ls_iterations = ls
        for f, v in state.items():
          getattr(d, f).assign(v)
        d.overflow.assign(np.zeros(d.nworld, dtype=np.int32))
        for i in range(NSTEP):
          if mjm.nu:
            mjw.ctrl_noise(m, d, 1000 + i)
          mjw.step(m, d)
        for f in FIELDS:
          out[f"{case}/{tag}{f}"] = _get(d, f)
    print(case, str(out[f"{case}/family"]), "nefc", d.nefc.numpy().tolist(), "niter", out[f"{case}/solver_niter"].tolist(), flush=True)
  np.savez(path, **out)


def compare(pa, pb):
  a, b = np.load(pa), np.load(pb)
  assert sorted(a.files) == sorted(b.files)
  cases = sorted({k.split("/")[0] for k in a.files})
  bad = 0
  for case in cases:
    same = [f for f in FIELDS if np.array_equal(a[f"{case}/{f}"], b[f"{case}/{f}"]) and np.array_equal(a[f"{case}/ls1/{f}"], b[f"{case}/ls1/{f}"])]
    moved = [f for f in FIELDS if not np.array_equal(b[f"{case}/{f}"], b[f"{case}/ls1/{f}"])]
    fam_ok = str(a[f"{case}/family"]) == str(b[f"{case}/family"]) and "expected" not in str(b[f"{case}/family"])
    ok = len(same) == len(FIELDS) and fam_ok
    bad += not ok
    print(f"{case:22s} {str(b[case + '/family']):14s} worlds {b[case + '/qacc'].shape[0]}  niter max {int(b[case + '/solver_niter'].max()):3d}  "
          f"{'all %d fields array_equal (also at ls_iterations = 1)' % len(FIELDS) if ok else 'DIFFERS: ' + str(sorted(set(FIELDS) - set(same)))}  "
          f"ls_iterations = 1 changes: {', '.join(moved) if moved else 'NOTHING (loop not shown live)'}")
  print(f"{len(cases)} scenes, {bad} differ")
  return 1 if bad else 0


if __name__ == "__main__":
  if len(sys.argv) == 3 and sys.argv[1] == "dump":
    dump(sys.argv[2])
  elif len(sys.argv) == 4 and sys.argv[1] == "compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))
  else:
    raise SystemExit(__doc__)
