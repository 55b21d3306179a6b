"""Cost of a masked reset: reset_data and reset_data_keyframe on the benchmark humanoid with about 10 % of the mask set, timed by a host clock around the
call plus a device synchronise, after warm-up.  With a baseline package (the Python of an older commit, which resets through host numpy, loaded
against the SAME library through MJH_LIB) the two are alternated call by call in one process.
python tools/reset_cost.py [nworld] [out file] [directory that holds the baseline's mujoco_warp_amd package]
Also prints the duration of one step (timed_steps, HIP events) so that a reset can be put beside what it interrupts."""
import importlib.util, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi

nworld = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
base_dir = sys.argv[3] if len(sys.argv) > 3 else None
REPS, WARM = 30, 5
HUMANOID = os.path.join(ROOT, "benchmarks", "humanoid", "humanoid.xml")


def load_baseline(path):
  """The baseline's package under another name, bound to the library this process has loaded (one HIP context, one set of kernels)."""
  os.environ["MJH_LIB"] = _abi.LIB_PATH
  spec = importlib.util.spec_from_file_location("mjw_baseline", os.path.join(path, "mujoco_warp_amd", "__init__.py"), submodule_search_locations=[os.path.join(path, "mujoco_warp_amd")])
  mod = importlib.util.module_from_spec(spec)
  sys.modules["mjw_baseline"] = mod
  spec.loader.exec_module(mod)
  return mod


def prepare(pkg):
  mjm = pkg.mjcf.load_xml(HUMANOID)
  m = pkg.put_model(mjm)
  d = pkg.make_data(mjm, nworld=nworld, nconmax=24, njmax=64)
  pkg.reset_data_keyframe(m, d, 0)
  for _ in range(20):
    pkg.step(m, d)
  return m, d


variants = {"new": (mjw, *prepare(mjw))}
if base_dir:
  base = load_baseline(base_dir)
  variants["baseline"] = (base, *prepare(base))
mask_host = np.random.default_rng(0).random(nworld) < 0.1
masks = {"new": mjw.device.DeviceArray.from_numpy(mask_host)}  # the new path reads the mask where an RL loop produces it: on the device
if base_dir:
  masks["baseline"] = sys.modules["mjw_baseline.device"].DeviceArray.from_numpy(mask_host)  # (the old path fetches it with .numpy())
calls = {"reset_data": lambda pkg, m, d, mask: pkg.reset_data(m, d, mask), "reset_data_keyframe": lambda pkg, m, d, mask: pkg.reset_data_keyframe(m, d, 0, mask)}

times = {(c, v): [] for c in calls for v in variants}
for cname, call in calls.items():
  for rep in range(WARM + REPS):
    for vname, (pkg, m, d) in variants.items():  # alternated call by call
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      call(pkg, m, d, masks[vname])
      torch.cuda.synchronize()
      if rep >= WARM:
        times[cname, vname].append(1e6 * (time.perf_counter() - t0))
      pkg.step(m, d)  # (the worlds move on between resets, as in a rollout)
# the two paths leave the same state behind (compared before the step timing below moves the new variant on)
same = None
if base_dir:
  (_, _, dn), (_, _, db) = variants["new"], variants["baseline"]
  same = {k: bool(np.array_equal(getattr(dn, k).numpy(), getattr(db, k).numpy())) for k in ("qpos", "qvel", "time", "qacc_warmstart", "nefc")}
m, d = variants["new"][1:]
step_ms = min(mjw.timed_steps(m, d, 200, step0=0)[0] for _ in range(3)) / 200

print(f"# {nworld} worlds, humanoid, {int(mask_host.sum())} of them ({100 * mask_host.mean():.1f} %) in the mask; host clock around call + device synchronise, {REPS} repetitions after "
      f"{WARM} warm-up calls, variants alternated call by call in one process; one step (HIP events, best of 3 x 200): {1e3 * step_ms:.1f} us", file=out)
for cname in calls:
  med = {}
  for vname in variants:
    t = np.array(times[cname, vname])
    med[vname] = float(np.median(t))
    print(f"{cname:20s} {vname:9s} median {med[vname]:10.1f} us   min {t.min():10.1f}   max {t.max():10.1f}   quartiles {np.percentile(t, 25):10.1f} .. {np.percentile(t, 75):10.1f}   "
          f"= {med[vname] / (1e3 * step_ms):8.2f} steps", file=out)
  if "baseline" in med:
    print(f"{cname:20s} baseline / new = {med['baseline'] / med['new']:.1f}x  (slowest new call {max(times[cname, 'new']):.1f} us, fastest baseline call {min(times[cname, 'baseline']):.1f} us)", file=out)
if same is not None:
  print(f"state after the run identical in both variants: {same}", file=out)
