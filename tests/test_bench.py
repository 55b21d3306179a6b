"""bench.py's --dump-outputs writer: float32 / float64 files only, and above the size cap a fixed, seeded sample of the worlds."""

import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


class _Arr:
  def __init__(self, a):
    self.a = a

  def numpy(self):
    return self.a


def _data(nworld, seed=0):
  rng = np.random.default_rng(seed)
  d = type("D", (), {})()
  for k in bench.OUTPUT_FIELDS:
    if k in ("solver_niter", "nefc", "ws_ncon", "overflow"):
      setattr(d, k, _Arr(rng.integers(0, 50, nworld).astype(np.int32)))
    elif k == "act":
      setattr(d, k, _Arr(np.zeros((nworld, 0), np.float32)))  # (na = 0: no file)
    else:
      setattr(d, k, _Arr(rng.standard_normal((nworld, 5)).astype(np.float32)))
  return d


def test_step_outputs_are_float32_or_float64():
  out = bench.step_outputs(_data(16))
  assert "act" not in out and set(out) == set(bench.OUTPUT_FIELDS) - {"act"}
  assert out["qpos"].dtype == np.float32 and out["nefc"].dtype == np.float64
  np.testing.assert_array_equal(out["nefc"], _data(16).nefc.a)  # int32 counters are exact in float64


def test_dump_writes_every_world_below_the_cap(tmp_path):
  out = bench.step_outputs(_data(64))
  bench.write_outputs(str(tmp_path), out, world_offset=128)
  for k, a in out.items():
    np.testing.assert_array_equal(np.load(tmp_path / f"{k}.npy"), a)
  np.testing.assert_array_equal(np.load(tmp_path / "world_id.npy"), np.arange(128, 192))


def test_dump_above_the_cap_is_a_fixed_sample(tmp_path, monkeypatch):
  monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
  out = bench.step_outputs(_data(1000))
  for sub in ("a", "b"):
    bench.write_outputs(str(tmp_path / sub), out, world_offset=0)
  files = glob.glob(str(tmp_path / "a" / "*.npy"))
  assert sum(os.path.getsize(f) - 128 for f in files) <= 4096  # (128: the .npy header)
  ids = np.load(tmp_path / "a" / "world_id.npy")
  assert 0 < len(ids) < 1000 and (np.diff(ids) > 0).all()
  np.testing.assert_array_equal(ids, np.load(tmp_path / "b" / "world_id.npy"))
  np.testing.assert_array_equal(np.load(tmp_path / "a" / "qvel.npy"), out["qvel"][ids.astype(int)])
  for f in files:
    assert np.load(f).dtype in (np.float32, np.float64)
