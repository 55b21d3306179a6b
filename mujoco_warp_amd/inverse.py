"""Inverse dynamics (reference _src/inverse.py): thin shims over mjh_inverse / mjh_inv_constraint (include/mjhip.h, csrc/inverse.hpp).

`inverse(m, d)` reads the state and `d.qacc` and writes `d.qfrc_inverse`, the generalized force that produces that acceleration (applied +
actuator forces, the generalized forces of xfrc_applied), together with `d.efc.force`, `d.efc.state` and `d.qfrc_constraint` evaluated at
it.  One launch sequence on torch's current HIP stream, no synchronisation, like every stage function.
"""

import ctypes

from . import _abi
from . import io
from . import types
from .forward import _stream

_INTEGRATOR_NAME = {int(types.IntegratorType.RK4): "RK4", int(types.IntegratorType.IMPLICITFAST): "implicitfast", int(types.IntegratorType.IMPLICIT): "implicit"}


def _invdiscrete(m):
  return bool(int(m.opt.enableflags) & int(types.EnableBit.INVDISCRETE))


def _check(m, d):
  if int(m.opt.enableflags) & int(types.EnableBit.SLEEP):
    raise NotImplementedError("inverse dynamics with sleeping enabled is not implemented (the two-pass collision and the asleep-tree shortcuts are not defined for it).")
  if _invdiscrete(m) and int(m.opt.integrator) != int(types.IntegratorType.EULER):
    raise NotImplementedError(f"discrete inverse dynamics (invdiscrete) is not implemented for the {_INTEGRATOR_NAME.get(int(m.opt.integrator), int(m.opt.integrator))} "
                              "integrator: only Euler is.")
  if getattr(d, "qfrc_inverse", None) is None or getattr(d, "ws_inverse", None) is None:
    raise ValueError("Data.qfrc_inverse / Data.ws_inverse missing (allocate Data with make_data/put_data)")


def inverse(m: types.Model, d: types.Data):
  """Inverse dynamics (reference inverse.py:148): fwd_position, fwd_velocity, the position / velocity sensors, the constraint forces at
  d.qacc, the acceleration sensors; d.qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint.  fwd_actuation is not called, as in
  the reference.  With EnableBit.INVDISCRETE (Euler only) d.qacc is the discrete acceleration (qvel' - qvel) / h; d.qacc itself is never written."""
  _check(m, d)
  scratch = d.ws_inverse if _invdiscrete(m) else None  # (make_data's: nothing is allocated here, so every call can be captured)
  L = _abi.lib()
  _abi.check(L.mjh_inverse(ctypes.byref(io.c_model(m)), ctypes.byref(io.c_data(d)), d.qfrc_inverse.ptr, scratch.ptr if scratch is not None else None, _stream()))


def inv_constraint(m: types.Model, d: types.Data):
  """Inverse constraint solver (reference inverse.py:129): d.efc.force, d.efc.state and d.qfrc_constraint at d.qacc, on the rows
  make_constraint left -- one launch, no iterations."""
  if int(m.opt.enableflags) & int(types.EnableBit.SLEEP):
    raise NotImplementedError("inverse dynamics with sleeping enabled is not implemented (the two-pass collision and the asleep-tree shortcuts are not defined for it).")
  L = _abi.lib()
  _abi.check(L.mjh_inv_constraint(ctypes.byref(io.c_model(m)), ctypes.byref(io.c_data(d)), d.qacc.ptr, None, _stream()))
