"""Cost of inverse dynamics on the benchmark humanoid: the k_inverse launch next to the solver launch of the same states, and inverse() next to
forward().  8192 worlds after 100 steps of the bench's control noise; everything in one process, on one stream, alternated repetition by
repetition.  The solver launch is timed by the library's per-launch event pairs (timed_steps(per_kernel=True, plain_kernels=True): the "solve"
class of one plain step, whose state is put back afterwards); k_inverse -- one launch -- and the two composite calls by HIP event pairs around the call.
python tools/inverse_cost.py [nworld] [out file]"""
import ctypes, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi, io
from mujoco_warp_amd.forward import _stream

nworld = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
REPS, WARM = 30, 5
mjm = mjw.mjcf.load_xml(os.path.join(ROOT, "benchmarks", "humanoid", "humanoid.xml"))


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b) * 1e3  # us


def median(x):
  return float(np.median(x))


print(f"inverse dynamics, humanoid, {nworld} worlds, njmax 64, after 100 noisy steps; medians of {REPS} repetitions after {WARM} warm-up, microseconds", file=out)
for solver in ("CG", "NEWTON"):
  mjm.opt.solver = int(getattr(mjw.SolverType, solver))
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=nworld, nconmax=24, njmax=64)
  mjw.reset_data_keyframe(m, d, 0)
  mjw.timed_steps(m, d, 100)
  mjw.forward(m, d)
  torch.cuda.synchronize()
  state = {k: getattr(d, k).t.clone() for k in ("qpos", "qvel", "ctrl", "time", "qacc_warmstart", "qacc", "solver_niter")}
  nefc = d.nefc.numpy()
  L = _abi.lib()
  cm, cd = io.c_model(m), io.c_data(d)
  k_inverse = lambda: _abi.check(L.mjh_inv_constraint(ctypes.byref(cm), ctypes.byref(cd), d.qacc.ptr, d.qfrc_inverse.ptr, _stream()))
  t = {"k_inverse": [], "solve launch": [], "inverse()": [], "forward()": []}
  for rep in range(WARM + REPS):
    row = {"k_inverse": timed(k_inverse), "inverse()": timed(lambda: mjw.inverse(m, d)), "forward()": timed(lambda: mjw.forward(m, d))}
    _, pk = mjw.timed_steps(m, d, 1, noise_std=-1.0, per_kernel=True, plain_kernels=True)
    row["solve launch"] = pk[mjw.KERNEL_NAMES.index("solve")] * 1e3
    for k, v in state.items():  # (the plain step moved the state: back to the states being measured)
      getattr(d, k).t.copy_(v)
    mjw.forward(m, d)
    if rep >= WARM:
      for k, v in row.items():
        t[k].append(v)
  jbytes = float(np.minimum(nefc, 64).sum()) * d.nv_pad * 4
  print(f"solver {solver} ({mjw.solver_kernel(m, d)}): mean nefc {nefc.mean():.1f}, J bytes read by k_inverse {jbytes / 1e6:.1f} MB", file=out)
  for k in t:
    print(f"  {k:14s} {median(t[k]):9.1f} us   (min {min(t[k]):.1f}, max {max(t[k]):.1f})", file=out)
  print(f"  k_inverse / solve launch = {median(t['k_inverse']) / median(t['solve launch']):.3f};  inverse() / forward() = {median(t['inverse()']) / median(t['forward()']):.3f};"
        f"  J read at {jbytes / (median(t['k_inverse']) * 1e-6) / 1e9:.0f} GB/s", file=out)
out.flush()
