"""Float64 truth for connect equality constraints (tests/test_connect.py).

No MuJoCo is installed and the oracle (oracle/mjref.c) knows joint equalities only, so the truth is built here -- on routes that do
not restate the kernel's formulas wherever such a route exists:

  kinematics   xpos, xmat, subtree_com, dense M, qacc_smooth: the oracle's RefSim, run on a copy of the host model WITHOUT its connects;
  pos          p1 - p2 from those poses (an anchor, or a site's position, carried by its body's pose);
  J            central finite differences of p1 - p2 along every dof: qpos is moved by the tangent step +-h e_i (quaternion joints: the
               rotation vector in the body frame, MuJoCo's convention for the dofs of a ball / free joint);
  Jdot qvel    central differences of that J along the flow q (+) +-h qvel;
  D, aref      a float64 restatement of constraint._efc_row (the one formula there is no other route to), aref -= Jdot qvel;
  qacc         the closed form of the unconstrained minimum -- every row an equality row, always active:
               (M + J' D J) qacc = M qacc_smooth + J' D aref.

H_J / H_FLOW are taken from the measured plateau of the finite differences' error (fd_plateau; tests/test_connect.py checks both the
plateau and an analytic ball-joint Jacobian).
"""

import copy

import numpy as np

from mujoco_warp_amd import _npmath as nm
from oracle import ref

EQ_CONNECT, OBJ_SITE = 0, 6
JNT_FREE, JNT_BALL = 0, 1
# finite-difference steps (float64): the error of a central difference is ~ h^2 |f'''| + eps |f| / h; test_connect.py measures the plateau
# of both differences on a ball joint with a closed form -- J is flat within 1e-9 for h in 1e-7 .. 1e-4; Jdot qvel is a difference of
# differences (its inner error, 1e-10, is divided by the outer step): 1e-5 off at h = 1e-5, 2.5e-5 off at 1e-2, within 1e-6 for 1e-4 .. 1e-3
H_J, H_FLOW = 1e-6, 3e-4


def strip_connects(mjm):
  """A copy of the host model without its connect equalities (what the oracle can run)."""
  s = copy.deepcopy(mjm)
  keep = np.flatnonzero(np.asarray(mjm.eq_type) != EQ_CONNECT)
  for name in ("eq_type", "eq_objtype", "eq_obj1id", "eq_obj2id", "eq_active0", "eq_solref", "eq_solimp", "eq_data"):
    setattr(s, name, np.asarray(getattr(mjm, name))[keep])
  if hasattr(s, "eq_names"):
    s.eq_names = [mjm.eq_names[i] for i in keep]
  s.neq = len(keep)
  return s


def integrate_pos(mjm, qpos, dv):
  """qpos moved by the tangent vector dv (one entry per dof): slide / hinge and the translation of a free joint add, the quaternion of a
  ball / free joint is multiplied on the right by the rotation vector's quaternion (body frame)."""
  q = np.array(qpos, dtype=np.float64)
  for j in range(mjm.njnt):
    qa, da, t = int(mjm.jnt_qposadr[j]), int(mjm.jnt_dofadr[j]), int(mjm.jnt_type[j])
    if t in (JNT_FREE, JNT_BALL):
      if t == JNT_FREE:
        q[qa:qa + 3] += dv[da:da + 3]
        qa, da = qa + 3, da + 3
      w = np.asarray(dv[da:da + 3], dtype=np.float64)
      angle = np.linalg.norm(w)
      rot = nm.axis_angle_to_quat(w / angle, angle) if angle > 0 else np.array([1.0, 0.0, 0.0, 0.0])
      q[qa:qa + 4] = nm.quat_normalize(nm.quat_mul(nm.quat_normalize(q[qa:qa + 4]), rot))
    else:
      q[qa] += dv[da]
  return q


def efc_row(timestep, refsafe, pos_aref, pos_imp, invweight, solref, solimp, vel):
  """(D, aref) of constraint._efc_row (reference constraint.py:84-153) in float64, margin 0."""
  timeconst, dampratio = float(solref[0]), float(solref[1])
  dmin, dmax, width, mid, power = (float(x) for x in solimp)
  if refsafe:
    timeconst = max(timeconst, 2.0 * timestep)
  dmin, dmax, mid = (min(max(x, 1e-4), 0.9999) for x in (dmin, dmax, mid))
  width, power = max(1e-15, width), max(1.0, power)
  k = 1.0 / (dmax * dmax * timeconst * timeconst * dampratio * dampratio)
  b = 2.0 / (dmax * timeconst)
  if solref[0] <= 0:
    k = -solref[0] / (dmax * dmax)
  if solref[1] <= 0:
    b = -solref[1] / dmax
  x = abs(pos_imp) / width
  if x < mid:
    y = x ** power / mid ** (power - 1.0)
  else:
    y = 1.0 - (1.0 - x) ** power / (1.0 - mid) ** (power - 1.0) if x < 1.0 else 1.0
  imp = min(max(dmin + y * (dmax - dmin), dmin), dmax)
  if x > 1.0:
    imp = dmax
  return 1.0 / max(invweight * (1.0 - imp) / imp, 1e-15), -k * imp * pos_aref - b * vel


class Truth:
  """The float64 truth of one host model with connects, at states given one at a time."""

  def __init__(self, mjm, njmax=64):
    self.mjm = mjm
    self.stripped = strip_connects(mjm)
    self.sim = ref.RefSim(self.stripped, nconmax=8, njmax=njmax, tolerance=1e-12, iterations=200)
    self.connects = [int(e) for e in np.flatnonzero(np.asarray(mjm.eq_type) == EQ_CONNECT)]

  # ---- kinematics through the oracle -------------------------------------------------------------------------------------------------
  def _pose(self, qpos, mocap=None):
    s = self.sim
    s.qpos[:] = qpos
    if mocap is not None:
      s.mocap_pos[:], s.mocap_quat[:] = mocap
    s.stage("kinematics")
    return s.xpos.copy(), s.xmat.reshape(-1, 3, 3).copy()

  def gap(self, qpos, e, eq_data=None, mocap=None):
    """p1 - p2 of connect e at qpos."""
    m = self.mjm
    xpos, xmat = self._pose(qpos, mocap)
    data = np.asarray(m.eq_data if eq_data is None else eq_data, dtype=np.float64).reshape(-1, 11)[e]
    p = []
    for side, obj in enumerate((int(m.eq_obj1id[e]), int(m.eq_obj2id[e]))):
      if int(m.eq_objtype[e]) == OBJ_SITE:
        b, local = int(m.site_bodyid[obj]), np.asarray(m.site_pos[obj], dtype=np.float64)
      else:
        b, local = obj, data[3 * side:3 * side + 3]
      p.append(xpos[b] + xmat[b] @ local)
    return p[0] - p[1]

  def jac(self, qpos, e, h=H_J, **kw):
    """[3, nv] central differences of the gap along every dof."""
    nv = self.mjm.nv
    J = np.zeros((3, nv))
    for i in range(nv):
      dv = np.zeros(nv)
      dv[i] = h
      J[:, i] = (self.gap(integrate_pos(self.mjm, qpos, dv), e, **kw) - self.gap(integrate_pos(self.mjm, qpos, -dv), e, **kw)) / (2.0 * h)
    return J

  def jac_dot_vel(self, qpos, qvel, e, h=H_FLOW, h_j=H_J, **kw):
    """[3] Jdot qvel: central difference of J along the flow of qvel, times qvel."""
    qvel = np.asarray(qvel, dtype=np.float64)
    Jp = self.jac(integrate_pos(self.mjm, qpos, h * qvel), e, h_j, **kw)
    Jm = self.jac(integrate_pos(self.mjm, qpos, -h * qvel), e, h_j, **kw)
    return (Jp - Jm) @ qvel / (2.0 * h)

  # ---- rows -----------------------------------------------------------------------------------------------------------------------
  def _joint_row(self, qpos, qvel, e):
    """The row of joint coupling e (constraint.py:500-640), for models that interleave the two kinds."""
    m = self.mjm
    j1, j2, data = int(m.eq_obj1id[e]), int(m.eq_obj2id[e]), np.asarray(m.eq_data[e], dtype=np.float64)
    d1, q1 = int(m.jnt_dofadr[j1]), int(m.jnt_qposadr[j1])
    J = np.zeros(m.nv)
    J[d1] = 1.0
    if j2 >= 0:
      d2, q2 = int(m.jnt_dofadr[j2]), int(m.jnt_qposadr[j2])
      dif = qpos[q2] - m.qpos0[q2]
      pos = qpos[q1] - m.qpos0[q1] - np.polyval(data[4::-1], dif)
      J[d2] = -np.polyval(np.polyder(data[4::-1]), dif)
      invweight = m.dof_invweight0[d1] + m.dof_invweight0[d2]
    else:
      pos, invweight = qpos[q1] - m.qpos0[q1] - data[0], m.dof_invweight0[d1]
    return J, pos, float(invweight)

  def rows(self, qpos, qvel, eq_active=None, eq_data=None, eq_solref=None, eq_solimp=None, mocap=None):
    """dict of the equality rows in equality-id order: J [ne, nv], pos, vel, D, aref, id (float64)."""
    m = self.mjm
    qpos, qvel = np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64)
    active = np.asarray(m.eq_active0 if eq_active is None else eq_active)
    solref = np.asarray(m.eq_solref if eq_solref is None else eq_solref, dtype=np.float64).reshape(-1, 2)
    solimp = np.asarray(m.eq_solimp if eq_solimp is None else eq_solimp, dtype=np.float64).reshape(-1, 5)
    refsafe = not (int(m.opt.disableflags) & (1 << 12))
    out = {k: [] for k in ("J", "pos", "vel", "D", "aref", "id")}
    kw = dict(eq_data=eq_data, mocap=mocap)
    for e in range(m.neq):
      if not active[e]:
        continue
      if int(m.eq_type[e]) == EQ_CONNECT:
        J, pos = self.jac(qpos, e, **kw), self.gap(qpos, e, **kw)
        jdv = self.jac_dot_vel(qpos, qvel, e, **kw)
        b = [int(m.site_bodyid[o]) if int(m.eq_objtype[e]) == OBJ_SITE else int(o) for o in (m.eq_obj1id[e], m.eq_obj2id[e])]
        invweight = float(m.body_invweight0[b[0], 0] + m.body_invweight0[b[1], 0])
        for k in range(3):
          vel = float(J[k] @ qvel)
          D, aref = efc_row(float(m.opt.timestep), refsafe, pos[k], np.linalg.norm(pos), invweight, solref[e], solimp[e], vel)
          for key, val in (("J", J[k]), ("pos", pos[k]), ("vel", vel), ("D", D), ("aref", aref - jdv[k]), ("id", e)):
            out[key].append(val)
      else:
        J, pos, invweight = self._joint_row(qpos, qvel, e)
        vel = float(J @ qvel)
        D, aref = efc_row(float(m.opt.timestep), refsafe, pos, pos, invweight, solref[e], solimp[e], vel)
        for key, val in (("J", J), ("pos", pos), ("vel", vel), ("D", D), ("aref", aref), ("id", e)):
          out[key].append(val)
    ne = len(out["id"])
    return {"J": np.array(out["J"]).reshape(ne, m.nv), "id": np.array(out["id"], dtype=np.int32),
            **{k: np.array(out[k], dtype=np.float64) for k in ("pos", "vel", "D", "aref")}}

  # ---- the constrained acceleration -------------------------------------------------------------------------------------------------
  def smooth(self, qpos, qvel, mocap=None):
    """(dense M, qacc_smooth, subtree_com, xipos) of the stripped model at the state: one oracle forward."""
    s = self.sim
    s.qpos[:], s.qvel[:] = qpos, qvel
    if mocap is not None:
      s.mocap_pos[:], s.mocap_quat[:] = mocap
    s.forward()
    return s.dense_M(), s.qacc_smooth.copy(), s.subtree_com.copy(), s.xipos.copy()

  def qacc(self, qpos, qvel, rows=None, **kw):
    """Closed form for a scene whose only rows are equality rows: (M + J' D J) qacc = M qacc_smooth + J' D aref."""
    r = self.rows(qpos, qvel, **kw) if rows is None else rows
    M, qacc_smooth = self.smooth(qpos, qvel, kw.get("mocap"))[:2]
    JD = r["J"].T * r["D"]
    return np.linalg.solve(M + JD @ r["J"], M @ qacc_smooth + JD @ r["aref"])


def fd_plateau(f, hs):
  """[len(hs)] max |f(h) - f(h_ref)| with h_ref the step where consecutive estimates agree best: the measured error floor of a finite difference."""
  vals = [np.asarray(f(h)) for h in hs]
  step = [np.abs(vals[i + 1] - vals[i]).max() for i in range(len(hs) - 1)]
  best = int(np.argmin(step))
  return np.array([np.abs(v - vals[best]).max() for v in vals]), hs[best]
