"""Float64 numpy truth for the general actuator transmissions (joint / jointinparent on every joint type, site, site + refsite).

Restated from the algorithm of record (the reference's smooth.py `_transmission` and support.py `jac_dof`), independently of
mujoco_warp_amd/trn_tables.py: columns are found from body ancestry here, not from dof-chain merge walks.

  truth(mjm, qpos, site_xpos, site_xmat, xquat, subtree_com, cdof) -> length [nu], dense moment [nu, nv]
      takes one world's position-stage fields (a device read-back goes through float32 exactly, so both sides start from the same numbers)
  truth_host(mjm, qpos) -> the same two outputs from qpos alone, through mjcf's float64 host kinematics (no device)
  body_jacobian(mjm, qpos, point, body) -> jacp, jacr [3, nv] written from joint anchors and axes, not from cdof (the self-check's witness)
"""

import numpy as np

from mujoco_warp_amd import mjcf

JOINT, JOINTINPARENT, SITE = 0, 1, 4
FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3


def qmul(u, v):
  return np.array([u[0] * v[0] - u[1] * v[1] - u[2] * v[2] - u[3] * v[3], u[0] * v[1] + u[1] * v[0] + u[2] * v[3] - u[3] * v[2],
                   u[0] * v[2] - u[1] * v[3] + u[2] * v[0] + u[3] * v[1], u[0] * v[3] + u[1] * v[2] - u[2] * v[1] + u[3] * v[0]])


def qconj(q):
  return np.array([q[0], -q[1], -q[2], -q[3]])


def qrot(v, q):
  return qmul(qmul(q, np.array([0.0, *v])), qconj(q))[1:]


def qnorm(q):
  q = np.asarray(q, dtype=np.float64)
  return q / np.linalg.norm(q)


def qmat(q):
  return np.stack([qrot(e, q) for e in np.eye(3)], axis=1)


def qvel(q):
  """rotation vector of a unit quaternion, angle in (-pi, pi]"""
  s = np.linalg.norm(q[1:])
  if s == 0.0:
    return np.zeros(3)
  a = 2.0 * np.arctan2(s, q[0])
  if a > np.pi:
    a -= 2.0 * np.pi
  return q[1:] * (a / s)


def _ancestors(mjm, body):
  out = set()
  while body > 0:
    out.add(int(body))
    body = int(mjm.body_parentid[body])
  return out


def _moving(mjm, body):
  """dofs that move `body`: those of the body and of its ancestors"""
  anc = _ancestors(mjm, body)
  return [i for i in range(int(mjm.nv)) if int(mjm.dof_bodyid[i]) in anc]


def _jac(mjm, point, body, subtree_com, cdof):
  jacp, jacr = np.zeros((3, int(mjm.nv))), np.zeros((3, int(mjm.nv)))
  off = point - subtree_com[int(mjm.body_rootid[body])]
  for i in _moving(mjm, body):
    ang, lin = cdof[i, :3], cdof[i, 3:]
    jacp[:, i], jacr[:, i] = lin + np.cross(ang, off), ang
  return jacp, jacr


def truth(mjm, qpos, site_xpos, site_xmat, xquat, subtree_com, cdof):
  f64 = lambda a, *shape: np.asarray(a, dtype=np.float64).reshape(*shape)
  nu, nv = int(mjm.nu), int(mjm.nv)
  qpos, site_xpos, site_xmat = f64(qpos, -1), f64(site_xpos, -1, 3), f64(site_xmat, -1, 3, 3)
  xquat, subtree_com, cdof = f64(xquat, -1, 4), f64(subtree_com, -1, 3), f64(cdof, -1, 6)
  gear, site_quat = f64(mjm.actuator_gear, nu, 6), f64(mjm.site_quat, -1, 4)
  length, moment = np.zeros(nu), np.zeros((nu, nv))
  for u in range(nu):
    t, (id0, id1), g = int(mjm.actuator_trntype[u]), (int(x) for x in np.asarray(mjm.actuator_trnid).reshape(-1, 2)[u]), gear[u]
    if t in (JOINT, JOINTINPARENT):
      jt, qa, da = int(mjm.jnt_type[id0]), int(mjm.jnt_qposadr[id0]), int(mjm.jnt_dofadr[id0])
      if jt == FREE:
        moment[u, da : da + 6] = g
        if t == JOINTINPARENT:
          moment[u, da + 3 : da + 6] = qrot(g[3:], qconj(qnorm(qpos[qa + 3 : qa + 7])))
      elif jt == BALL:
        q = qnorm(qpos[qa : qa + 4])
        axis = qrot(g[:3], qconj(q)) if t == JOINTINPARENT else g[:3]
        length[u] = qvel(q) @ axis
        moment[u, da : da + 3] = axis
      else:
        length[u] = qpos[qa] * g[0]
        moment[u, da] = g[0]
      continue
    assert t == SITE
    b0 = int(mjm.site_bodyid[id0])
    jp, jr = _jac(mjm, site_xpos[id0], b0, subtree_com, cdof)
    if id1 < 0:
      moment[u] = jp.T @ (site_xmat[id0] @ g[:3]) + jr.T @ (site_xmat[id0] @ g[3:])
      continue
    b1 = int(mjm.site_bodyid[id1])
    rp, rr = _jac(mjm, site_xpos[id1], b1, subtree_com, cdof)
    R = site_xmat[id1]
    if g[:3].any():
      length[u] += (R.T @ (site_xpos[id0] - site_xpos[id1])) @ g[:3]
    if g[3:].any():  # site_quat o xquat, the reference's order
      qs, qr = qmul(site_quat[id0], xquat[b0]), qmul(site_quat[id1], xquat[b1])
      length[u] += qvel(qmul(qconj(qr), qs)) @ g[3:]
    row = (jp - rp).T @ (R @ g[:3]) + (jr - rr).T @ (R @ g[3:])
    both = set(_moving(mjm, b0)) & set(_moving(mjm, b1))  # dofs that move both sites alike are not columns of the row
    row[sorted(both)] = 0.0
    moment[u] = row
  return length, moment


def host_fields(mjm, qpos):
  h = mjcf.host_mass_matrix(mjm, np.asarray(qpos, dtype=np.float64))
  sb = np.asarray(mjm.site_bodyid).reshape(-1)
  site_pos, site_quat = np.asarray(mjm.site_pos, dtype=np.float64).reshape(-1, 3), np.asarray(mjm.site_quat, dtype=np.float64).reshape(-1, 4)
  site_xpos = np.array([h["xpos"][sb[s]] + h["xmat"][sb[s]] @ site_pos[s] for s in range(len(sb))]).reshape(-1, 3)
  site_xmat = np.array([qmat(qnorm(qmul(h["xquat"][sb[s]], site_quat[s]))) for s in range(len(sb))]).reshape(-1, 3, 3)
  return dict(h, site_xpos=site_xpos, site_xmat=site_xmat)


def truth_host(mjm, qpos):
  h = host_fields(mjm, qpos)
  return truth(mjm, qpos, h["site_xpos"], h["site_xmat"], h["xquat"], h["subtree_com"], h["cdof"])


def body_jacobian(mjm, qpos, point, body):
  """Geometric Jacobian of `point` fixed to `body`, from joint anchors and axes (no cdof, no subtree COM)."""
  xpos, xquat, xanchor, xaxis = mjcf._host_kinematics(mjm, np.asarray(qpos, dtype=np.float64))
  nv = int(mjm.nv)
  jacp, jacr = np.zeros((3, nv)), np.zeros((3, nv))
  anc = _ancestors(mjm, body)
  for j in range(int(mjm.njnt)):
    b = int(mjm.jnt_bodyid[j])
    if b not in anc:
      continue
    t, d = int(mjm.jnt_type[j]), int(mjm.jnt_dofadr[j])
    if t == FREE:
      jacp[:, d : d + 3] = np.eye(3)
      R = qmat(xquat[b])
      for k in range(3):
        jacr[:, d + 3 + k] = R[:, k]
        jacp[:, d + 3 + k] = np.cross(R[:, k], point - xpos[b])
    elif t == BALL:
      R = qmat(xquat[b])
      for k in range(3):
        jacr[:, d + k] = R[:, k]
        jacp[:, d + k] = np.cross(R[:, k], point - xanchor[j])
    elif t == SLIDE:
      jacp[:, d] = xaxis[j]
    else:
      jacr[:, d] = xaxis[j]
      jacp[:, d] = np.cross(xaxis[j], point - xanchor[j])
  return jacp, jacr


def advance(mjm, qpos, dof, h):
  """qpos moved by h along the tangent direction of one dof (quaternions: right-multiplied by the rotation about the body axis)."""
  q = np.array(qpos, dtype=np.float64)
  j = int(mjm.dof_jntid[dof])
  t, qa, k = int(mjm.jnt_type[j]), int(mjm.jnt_qposadr[j]), dof - int(mjm.jnt_dofadr[j])
  if t in (SLIDE, HINGE) or (t == FREE and k < 3):
    q[qa + k] += h
    return q
  qa, k = (qa + 3, k - 3) if t == FREE else (qa, k)
  e = np.zeros(3)
  e[k] = 1.0
  q[qa : qa + 4] = qnorm(qmul(qnorm(q[qa : qa + 4]), np.array([np.cos(h / 2), *(np.sin(h / 2) * e)])))
  return q
