"""Actuator and sensor delays: reading and initialising the history buffers of Data.history.

Same names and signatures as the reference's history.read_ctrl / read_sensor / init_ctrl_history / init_sensor_history
(the reference's mujoco_warp/_src/history.py:634, 718, 796, 881); every call is one launch of csrc/history.hpp on torch's current HIP
stream and returns without synchronising.  `step` and `forward` apply the delays themselves ("Delays").
"""

import ctypes
from typing import Optional

import numpy as np

from . import _abi
from . import io
from . import types
from .device import DeviceArray
from .forward import _stream


def _check_id(m, kind, i):
  n = m.nsensor if kind == "sensor" else m.nu
  if not 0 <= int(i) < n:
    raise ValueError(f"{kind} id {i} out of range [0, {n})")
  hist = m._history_host[f"{'sensor' if kind == 'sensor' else 'actuator'}_history"][int(i)]
  return int(hist[0]), (int(m._history_host["sensor_dim"][int(i)]) if kind == "sensor" else 1)


def _read(m, d, kind, i, time, interp, result):
  nsample, dim = _check_id(m, kind, i)
  if int(interp) not in (-1, 0, 1, 2):
    raise ValueError(f"interp must be -1 (the model's), 0 (zero-order hold), 1 (linear) or 2 (cubic), got {interp}")
  if tuple(time.shape) != (d.nworld,) or np.dtype(time.dtype) != np.float32:
    raise ValueError(f"time must be a float32 array of shape ({d.nworld},)")
  want = ((d.nworld,), (d.nworld, 1)) if kind == "ctrl" else ((d.nworld, dim),)
  if tuple(result.shape) not in want or np.dtype(result.dtype) != np.float32:
    raise ValueError(f"result must be a float32 array of shape {want[-1]}")
  _abi.check(_abi.lib().mjh_history_read(ctypes.byref(io.c_model(m)), ctypes.byref(io.c_data(d)), int(kind == "sensor"), int(i), time.ptr, int(interp),
                                         result.ptr, dim, _stream()))


def read_ctrl(m: types.Model, d: types.Data, ctrlid: int, time: DeviceArray, interp: int, result: DeviceArray):
  """result[w] = the ctrl of actuator `ctrlid` its history buffer holds for time[w] - delay (reference history.read_ctrl): time [nworld] float32,
  interp -1 (the model's) / 0 zero-order hold / 1 linear / 2 cubic, result [nworld] (or [nworld, 1]).  An actuator without a buffer returns Data.ctrl."""
  _read(m, d, "ctrl", ctrlid, time, interp, result)


def read_sensor(m: types.Model, d: types.Data, sensorid: int, time: DeviceArray, interp: int, result: DeviceArray):
  """result[w, :] = the reading of sensor `sensorid` its history buffer holds for time[w] - delay (reference history.read_sensor); result
  [nworld, sensor_dim].  A sensor without a buffer returns its slice of Data.sensordata."""
  _read(m, d, "sensor", sensorid, time, interp, result)


def _init(m, d, kind, i, times, values, phase):
  nsample, dim = _check_id(m, kind, i)
  if nsample < 1:
    raise ValueError(f"{kind} {i} has no history buffer (nsample = 0)")
  t_dev = None
  if times is not None:
    t_np = np.asarray(times.numpy() if hasattr(times, "numpy") else times, dtype=np.float32).reshape(-1)
    if len(t_np) != nsample:
      raise ValueError(f"times must have nsample = {nsample} entries, got {len(t_np)}")
    for k in range(len(t_np) - 1):  # (reference history.py:816-820)
      if not t_np[k + 1] - t_np[k] >= types.MJ_MINVAL:
        raise ValueError(f"times must be strictly increasing, got times[{k}]={t_np[k]} >= times[{k + 1}]={t_np[k + 1]}")
    t_dev = times if isinstance(times, DeviceArray) and np.dtype(times.dtype) == np.float32 else DeviceArray.from_numpy(t_np)
  if tuple(values.shape) != (d.nworld, nsample * dim) or np.dtype(values.dtype) != np.float32:
    raise ValueError(f"values must be a float32 array of shape ({d.nworld}, {nsample * dim})")
  if phase is not None and (tuple(phase.shape) != (d.nworld,) or np.dtype(phase.dtype) != np.float32):
    raise ValueError(f"phase must be a float32 array of shape ({d.nworld},)")
  _abi.check(_abi.lib().mjh_history_init(ctypes.byref(io.c_model(m)), ctypes.byref(io.c_data(d)), int(kind == "sensor"), int(i),
                                         t_dev.ptr if t_dev is not None else None, values.ptr, nsample * dim, phase.ptr if phase is not None else None, _stream()))
  return t_dev  # (kept alive by the caller's frame until the launch is queued; the stream orders the rest)


def init_ctrl_history(m: types.Model, d: types.Data, ctrlid: int, times: Optional[DeviceArray], values: DeviceArray):
  """Fills the history buffer of actuator `ctrlid` in every world (reference history.init_ctrl_history): values [nworld, nsample], oldest
  first, at times [nsample] (strictly increasing, else ValueError) or, with times None, at -1e10; the user slot is kept."""
  _init(m, d, "ctrl", ctrlid, times, values, None)


def init_sensor_history(m: types.Model, d: types.Data, sensorid: int, times: Optional[DeviceArray], values: DeviceArray, phase: DeviceArray):
  """Fills the history buffer of sensor `sensorid` in every world (reference history.init_sensor_history): values [nworld, nsample * dim],
  oldest first; phase [nworld] goes to the buffer's user slot."""
  _init(m, d, "sensor", sensorid, times, values, phase)
