"""Device-side mj_setConst: recompute the constants MuJoCo derives from the inertial parameters after they were changed on the device
(domain randomisation through put_model(..., batch_sizes=...) or an in-place `assign`).

  set_const_fixed(m, d)   m.body_subtreemass                                       (reference set_const.py:35-59)
  set_const_0(m, d)       m.dof_invweight0, m.body_invweight0, m.stat.meaninertia  (reference set_const.py:170-190, 208-375), at qpos0
  set_const(m, d)         both
  set_const_spring(m, d)  nothing: this engine has no tendons (ntendon is always 0), so no spring rest length depends on qpos_spring

One launch of csrc/set_const.hpp for all model-worlds restates mjcf.set_const (the float64 host version) in float32: subtree masses by
leaf-to-root accumulation of body_mass; kinematics, subtree COM, cinert, cdof, CRB and M (with dof_armature) at qpos0;
meaninertia = mean(diag M); A = diag(M^-1) averaged over the translational / rotational triples of free and ball joints; per moving body
the means of the translational and rotational diagonals of J M^-1 J' at the body's inertial frame, with MuJoCo's MJ_MINVAL swap rule.

Batching.  Inputs (body_mass, body_inertia, body_ipos, body_iquat, body_pos, body_quat, jnt_pos, jnt_axis, dof_armature, qpos0) are read
per world by the usual modulo rule, so a field with leading dimension 1 is shared.  With N the largest leading dimension among them,
every input has leading dimension 1 or N and every output the call writes has leading dimension N -- anything else raises ValueError
(computing world 0 only would leave the other worlds inconsistent, silently).  Outputs are written in place: the same device memory, no
field is re-bound, so a StepGraph captured before the call stays valid and sees the new values at its next replay.

`d` and `restore`.  The kernel keeps every intermediate in LDS and registers and never touches Data: `d` is accepted for signature
compatibility with the reference, may be None and is left bit for bit unchanged; `restore` has nothing to do.  (The reference runs its
stage kernels through Data and restores it afterwards when asked; this contract is the stronger one.)

nv == 0: the subtree masses are computed, meaninertia is 1 and body_invweight0 is 0; no kernel is launched.

Out of scope:
  * actuator_acc0 and dampratio resolution: the loader refuses dampratio, and actuator_acc0 is not a device field;
  * cam_*0 and light_*0: ncam is 0;
  * connect eq_data: the second anchor (eq_data[3:6]) is computed by the loader at qpos0 and is per-world data of its own -- after moving
    body frames or qpos0 on the device, write the anchors you mean (weld equalities are not built);
  * the host-only sleep tables dof_length and tree_sleep_policy;
  * set_length_range.
"""

import ctypes

from . import _abi
from . import io

_FIXED = _abi.DEFINES["MJH_SET_CONST_FIXED"]
_QPOS0 = _abi.DEFINES["MJH_SET_CONST_0"]

# Model fields each part reads / writes (meaninertia lives in m.stat; its batch_sizes key is "meaninertia")
INPUTS = {_FIXED: ("body_mass",),
          _QPOS0: ("body_mass", "body_inertia", "body_ipos", "body_iquat", "body_pos", "body_quat", "jnt_pos", "jnt_axis", "dof_armature", "qpos0")}
OUTPUTS = {_FIXED: ("body_subtreemass",), _QPOS0: ("dof_invweight0", "body_invweight0", "meaninertia")}


def _fields(table, what):
  return tuple(dict.fromkeys(n for bit in (_FIXED, _QPOS0) if what & bit for n in table[bit]))


def batch_plan(inputs: dict, outputs: dict) -> int:
  """N, the number of model-worlds a call computes, from the leading dimensions {field: n} of its inputs and outputs (host only).

  Raises ValueError when an input's leading dimension is neither 1 nor N, or an output's is not N."""
  n = max(inputs.values())
  mixed = {k: v for k, v in inputs.items() if v not in (1, n)}
  if mixed:
    raise ValueError(f"set_const: input fields must have leading dimension 1 or {n} (the largest among them); got {mixed}")
  short = [k for k, v in outputs.items() if v != n]
  if short:
    raise ValueError(f"set_const: {n} model-worlds are randomised but the output fields {short} do not have leading dimension {n}: "
                     f"add them to put_model's batch_sizes, e.g. batch_sizes={{{', '.join(f'{k!r}: {n}' for k in short)}, ...}}")
  return n


def _field(m, name):
  return m.stat.meaninertia if name == "meaninertia" else getattr(m, name)


def _subtreemass_nv0(m):
  """nv == 0 (nothing moves): leaf-to-root accumulation on the array's own device, no kernel."""
  t = m.body_mass.t.clone()
  parent = m.body_parentid.numpy()
  for b in range(int(m.nbody) - 1, 0, -1):
    t[:, int(parent[b])] += t[:, b]
  return t


def _run(m, what):
  ins = {n: int(_field(m, n).shape[0]) for n in _fields(INPUTS, what)}
  outs = {n: int(_field(m, n).shape[0]) for n in _fields(OUTPUTS, what)}
  n = batch_plan(ins, outs)
  if int(m.nv) == 0:
    if what & _FIXED:
      m.body_subtreemass.t.copy_(_subtreemass_nv0(m))
    if what & _QPOS0:
      m.stat.meaninertia.fill_(1.0)
      m.body_invweight0.zero_()
    return
  from .forward import _stream

  ptr = lambda name: ctypes.c_void_p(_field(m, name).ptr) if name in outs else None
  _abi.check(_abi.lib().mjh_set_const(ctypes.byref(io.c_model(m)), n, ptr("body_subtreemass"), ptr("dof_invweight0"), ptr("body_invweight0"),
                                      ptr("meaninertia"), what, _stream()))


def set_const_fixed(m, d=None):
  """Recompute m.body_subtreemass from m.body_mass (in place; `d` is not touched and may be None)."""
  _run(m, _FIXED)


def set_const_0(m, d=None, restore: bool = True):
  """Recompute m.dof_invweight0, m.body_invweight0 and m.stat.meaninertia at qpos0 (in place; `d` is not touched and may be None;
  `restore` has nothing to do)."""
  _run(m, _QPOS0)


def set_const_spring(m, d=None, restore: bool = True):
  """No-op: the quantities the reference derives from qpos_spring are tendon spring lengths, and this engine has no tendons."""


def set_const(m, d=None, restore: bool = True):
  """set_const_fixed and set_const_0 in one launch (in place; `d` is not touched and may be None; `restore` has nothing to do)."""
  _run(m, _FIXED | _QPOS0)
