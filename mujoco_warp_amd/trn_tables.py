"""Host side of the general actuator transmissions (reference smooth.py _transmission; device: csrc/transmission.hpp).

The sparse structure of Data.actuator_moment depends on the model only: `moment_structure` compiles it once -- rows in actuator order,
columns ascending within a row (MuJoCo C's layout; the reference assigns rowadr with an atomic, so its row order may differ) -- together
with the dof-major transpose the velocity stage gathers qfrc_actuator over.  `host_moment` is the float64 length and dense moment at one
configuration, used for actuator_acc0.  Both take a compiled host model (mujoco.MjModel or the numpy stand-in of mjcf.py).
"""

import numpy as np

from . import _npmath as nm

TRN_JOINT, TRN_JOINTINPARENT, TRN_SLIDERCRANK, TRN_TENDON, TRN_SITE, TRN_BODY = range(6)
JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = range(4)
_NOT_BUILT = {TRN_SLIDERCRANK: "slider-crank", TRN_TENDON: "tendon", TRN_BODY: "body (adhesion)"}


def _quat_to_vel(q):
  """Rotation vector of a unit quaternion, angle in (-pi, pi] (reference math.py quat_to_vel)."""
  axis = np.asarray(q[1:], dtype=np.float64)
  sin_a_2 = float(np.linalg.norm(axis))
  if sin_a_2 == 0.0:
    return np.zeros(3)
  speed = 2.0 * np.arctan2(sin_a_2, q[0])
  if speed > np.pi:
    speed -= 2.0 * np.pi
  return axis * (speed / sin_a_2)


def check_types(trntype):
  for t in np.asarray(trntype).reshape(-1):
    if int(t) in _NOT_BUILT:
      raise NotImplementedError(f"{_NOT_BUILT[int(t)]} transmissions are not built (joint, jointinparent and site transmissions are)")
    if int(t) not in (TRN_JOINT, TRN_JOINTINPARENT, TRN_SITE):
      raise NotImplementedError(f"unknown transmission type {int(t)}")


def _chain(mjm, siteid):
  """Dofs that move the site, ascending: the ancestor chain of the last dof of body_weldid[site_bodyid] (empty for a site welded to the world)."""
  parent = np.asarray(mjm.dof_parentid)
  b = int(np.asarray(mjm.body_weldid)[int(np.asarray(mjm.site_bodyid)[siteid])])
  out = []
  if b > 0:
    d = int(np.asarray(mjm.body_dofadr)[b]) + int(np.asarray(mjm.body_dofnum)[b]) - 1
    while d >= 0:
      out.append(d)
      d = int(parent[d])
  return out[::-1]


def moment_structure(mjm):
  """dict of int32 arrays: moment_rownnz / moment_rowadr [nu], moment_colind / moment_side / moment_rowid [nJmom], momentT_adr [nv + 1],
  momentT_act / momentT_ind [nJmom], plus `scalar` [nu] (bool: the row is the gear[0] of a hinge / slide joint) and nJmom."""
  nu, nv = int(mjm.nu), int(mjm.nv)
  trntype = np.asarray(mjm.actuator_trntype).reshape(-1)
  trnid = np.asarray(mjm.actuator_trnid).reshape(-1, 2)
  jnt_type, jnt_dofadr = np.asarray(mjm.jnt_type), np.asarray(mjm.jnt_dofadr)
  rows, sides, scalar = [], [], np.zeros(nu, dtype=bool)
  for u in range(nu):
    t = int(trntype[u])
    if t in (TRN_JOINT, TRN_JOINTINPARENT):
      j = int(trnid[u, 0])
      n = {JNT_FREE: 6, JNT_BALL: 3}.get(int(jnt_type[j]), 1)
      scalar[u] = n == 1
      cols, side = list(range(int(jnt_dofadr[j]), int(jnt_dofadr[j]) + n)), [0] * n
    else:
      c1 = _chain(mjm, int(trnid[u, 0]))
      c2 = _chain(mjm, int(trnid[u, 1])) if trnid[u, 1] >= 0 else []
      # the reference's merge walk (smooth.py:2661-2727): leaf to root over both chains, stopping at the first dof they share -- that dof
      # and everything above it moves both sites alike
      cols, side = [], []
      a, b = len(c1) - 1, len(c2) - 1
      while a >= 0 or b >= 0:
        da, db = (c1[a] if a >= 0 else -1), (c2[b] if b >= 0 else -1)
        if da == db:
          break
        cols.append(max(da, db))
        side.append(1 if da > db else 2)
        if da > db:
          a -= 1
        else:
          b -= 1
      cols, side = cols[::-1], side[::-1]
    rows.append(cols)
    sides.append(side)
  rownnz = np.array([len(r) for r in rows], dtype=np.int32).reshape(nu)
  rowadr = (np.cumsum(rownnz) - rownnz).astype(np.int32)
  flat = lambda ll: np.array([x for l in ll for x in l], dtype=np.int32)
  colind, side = flat(rows), flat(sides)
  rowid = np.repeat(np.arange(nu, dtype=np.int32), rownnz)
  # dof-major transpose; a stable sort keeps the actuators of a dof in ascending order
  order = np.argsort(colind, kind="stable").astype(np.int32)
  t_adr = np.zeros(nv + 1, dtype=np.int32)
  np.cumsum(np.bincount(colind, minlength=nv)[:nv], out=t_adr[1:])
  return dict(moment_rownnz=rownnz, moment_rowadr=rowadr, moment_colind=colind, moment_side=side, moment_rowid=rowid, momentT_adr=t_adr,
              momentT_act=rowid[order].astype(np.int32), momentT_ind=order, scalar=scalar, nJmom=int(rownnz.sum()))


def host_moment(mjm, qpos, h, st=None):
  """(length [nu], dense moment [nu, nv]) in float64 at `qpos`; h: mjcf.host_mass_matrix(mjm, qpos) (xpos, xquat, xmat, subtree_com, cdof)."""
  nu, nv = int(mjm.nu), int(mjm.nv)
  st = st or moment_structure(mjm)
  qpos = np.asarray(qpos, dtype=np.float64)
  gear = np.asarray(mjm.actuator_gear, dtype=np.float64).reshape(nu, 6)
  trntype, trnid = np.asarray(mjm.actuator_trntype).reshape(-1), np.asarray(mjm.actuator_trnid).reshape(-1, 2)
  site_body = np.asarray(mjm.site_bodyid).reshape(-1)
  site_pos, site_quat = np.asarray(mjm.site_pos, dtype=np.float64).reshape(-1, 3), np.asarray(mjm.site_quat, dtype=np.float64).reshape(-1, 4)
  sxpos = lambda s: h["xpos"][site_body[s]] + h["xmat"][site_body[s]] @ site_pos[s]
  sxmat = lambda s: nm.quat_to_mat(nm.quat_mul(h["xquat"][site_body[s]], site_quat[s]))
  conj = lambda q: q * np.array([1.0, -1.0, -1.0, -1.0])
  length, moment = np.zeros(nu), np.zeros((nu, nv))
  for u in range(nu):
    adr, n = int(st["moment_rowadr"][u]), int(st["moment_rownnz"][u])
    cols, t, g = st["moment_colind"][adr : adr + n], int(trntype[u]), gear[u]
    if t in (TRN_JOINT, TRN_JOINTINPARENT):
      j = int(trnid[u, 0])
      jt, qa = int(mjm.jnt_type[j]), int(mjm.jnt_qposadr[j])
      if jt == JNT_FREE:
        row = g.copy()
        if t == TRN_JOINTINPARENT:
          row[3:] = nm.rot_vec_quat(g[3:], conj(nm.quat_normalize(qpos[qa + 3 : qa + 7])))
      elif jt == JNT_BALL:
        q = nm.quat_normalize(qpos[qa : qa + 4])
        row = nm.rot_vec_quat(g[:3], conj(q)) if t == TRN_JOINTINPARENT else g[:3].copy()
        length[u] = float(np.dot(_quat_to_vel(q), row))
      else:
        row = g[:1]
        length[u] = qpos[qa] * g[0]
      moment[u, cols] = row
      continue
    s, r = int(trnid[u, 0]), int(trnid[u, 1])
    frame = sxmat(s if r < 0 else r)
    wt, wr = frame @ g[:3], frame @ g[3:]
    if r >= 0:
      if g[:3].any():
        length[u] += float(np.dot(frame.T @ (sxpos(s) - sxpos(r)), g[:3]))
      if g[3:].any():  # (site_quat o xquat: the reference's order, smooth.py:2642)
        qs, qr = nm.quat_mul(site_quat[s], h["xquat"][site_body[s]]), nm.quat_mul(site_quat[r], h["xquat"][site_body[r]])
        length[u] += float(np.dot(_quat_to_vel(nm.quat_mul(conj(qr), qs)), g[3:]))
    for k in range(n):
      i, side = int(cols[k]), int(st["moment_side"][adr + k])
      ang, lin = h["cdof"][i, :3], h["cdof"][i, 3:]
      off = sxpos(r if side == 2 else s) - h["subtree_com"][int(mjm.body_rootid[int(mjm.dof_bodyid[i])])]
      v = float(np.dot(lin + np.cross(ang, off), wt) + np.dot(ang, wr))
      moment[u, i] = -v if side == 2 else v
  return length, moment
