"""What reset_data / reset_data_keyframe leave in Data: a numpy restatement of the list of fields a reset writes, computed from the host model
and a snapshot of Data taken before the reset.  A reset only copies and fills, so every comparison against this truth is bitwise.

  expected(mjm, snap, mask=..., key=..., keys=..., batched=...) -> {field: array}: the whole snapshot after the reset.

World w is reset when mask[w] is nonzero (mask None: every world) and, in the per-world key form, when keys[w] is in [0, nkey).  A reset world gets
  qpos                    qpos0[w % nb], or key_qpos[key]
  qvel, act, ctrl         0, or the keyframe's
  qacc_warmstart, qacc, qfrc_applied, xfrc_applied      0
  time                    0, or key_time[key]
  mocap_pos, mocap_quat   the (batched) body_pos / body_quat of the mocap bodies, in mocap-id order; then the keyframe's mpos / mquat
  the ten sleep tables    every tree awake (what make_data writes)
  eq_active               eq_active0
  nefc, ne, nf, nl, solver_niter, overflow, ws_ncon, ws_ncollision      0
  history                 every buffer [user 0, cursor n - 1, times time - (n - k) timestep, values 0] (history_truth.Buffer.initial)
and, only in the call without mask and without per-world keys, nacon, ncollision and ws_conadr become 0.  Every other entry of the snapshot --
the other worlds, and every field not named here -- stays as it was.

`batched`: {name: array with a leading batch dimension} for the Model fields made per-world (qpos0, body_pos, body_quat, timestep); a field not
given is the host model's own, shared by every world.  Values are float32, as the device holds them.
"""

import numpy as np

import history_truth as ht

MINAWAKE = 10  # mjMINAWAKE
AWAKE, STATIC = 1, -1
STATE_ZERO = ("qacc_warmstart", "qacc", "qfrc_applied", "xfrc_applied")
COUNTERS = ("nefc", "ne", "nf", "nl", "solver_niter", "overflow", "ws_ncon", "ws_ncollision")
GLOBAL_COUNTERS = ("nacon", "ncollision", "ws_conadr")
SLEEP_TABLES = ("tree_asleep", "tree_awake", "body_awake", "body_awake_ind", "dof_awake_ind", "ntree_awake", "nbody_awake", "nv_awake", "tree_island", "nisland")
WRITTEN = ("qpos", "qvel", "act", "ctrl", "time", "mocap_pos", "mocap_quat", "eq_active", "history") + STATE_ZERO + COUNTERS + GLOBAL_COUNTERS + SLEEP_TABLES


def _f32(a):
  return np.asarray(a, dtype=np.float32)


def mocap_bodies(mjm):
  """The body of mocap id 0, 1, ..."""
  mid = np.asarray(mjm.body_mocapid)
  return [int(np.flatnonzero(mid == k)[0]) for k in range(int(mjm.nmocap))]


def sleep_rows(mjm):
  """One world's rows of the ten sleep tables with every tree awake."""
  nt, nb, nv = int(mjm.ntree), int(mjm.nbody), int(mjm.nv)
  treeid, rootid, mocapid = np.asarray(mjm.body_treeid), np.asarray(mjm.body_rootid), np.asarray(mjm.body_mocapid)
  body_awake = [AWAKE if treeid[b] >= 0 or mocapid[rootid[b]] >= 0 else STATIC for b in range(nb)]
  return dict(tree_asleep=np.full(nt, -(1 + MINAWAKE)), tree_awake=np.ones(nt), body_awake=np.array(body_awake), body_awake_ind=np.arange(nb),
              dof_awake_ind=np.arange(nv), ntree_awake=nt, nbody_awake=nb, nv_awake=nv, tree_island=np.full(nt, -1), nisland=0)


def history_row(mjm, time, timestep):
  """One world's row of Data.history in its initial state at `time` (float32 values in, float64 arithmetic, float32 out)."""
  row = np.zeros(int(mjm.nhistory), dtype=np.float32)
  tables = ((mjm.actuator_history, mjm.actuator_historyadr, np.ones(int(mjm.nu), dtype=int)), (mjm.sensor_history, mjm.sensor_historyadr, mjm.sensor_dim))
  for hist, adr, dim in tables:
    hist = np.asarray(hist).reshape(-1, 2)
    for i in range(len(hist)):
      n = int(hist[i, 0])
      if n > 0:
        flat = ht.Buffer.initial(n, int(dim[i]), float(np.float32(time)), float(np.float32(timestep))).flat()
        row[int(adr[i]) : int(adr[i]) + len(flat)] = flat.astype(np.float32)
  return row


def expected(mjm, snap, mask=None, key=-1, keys=None, batched=None):
  batched = batched or {}
  out = {k: np.array(v, copy=True) for k, v in snap.items()}
  W = out["qpos"].shape[0]
  nkey, nmocap = int(mjm.nkey), int(mjm.nmocap)
  row = lambda name, host, w: _f32(batched[name])[w % len(batched[name])] if name in batched else _f32(host)
  bodies = mocap_bodies(mjm)
  sleep = sleep_rows(mjm)
  for w in range(W):
    if mask is not None and not mask[w]:
      continue
    k = int(key if keys is None else keys[w])
    if keys is not None and not 0 <= k < nkey:
      continue
    out["qpos"][w] = _f32(mjm.key_qpos)[k] if k >= 0 else row("qpos0", mjm.qpos0, w)
    for name, table in (("qvel", mjm.key_qvel), ("act", mjm.key_act), ("ctrl", mjm.key_ctrl)):
      out[name][w] = _f32(table)[k] if k >= 0 else 0.0
    for name in STATE_ZERO:
      out[name][w] = 0.0
    time = np.float32(mjm.key_time[k]) if k >= 0 else np.float32(0.0)
    out["time"][w] = time
    if nmocap:
      out["mocap_pos"][w] = row("body_pos", mjm.body_pos, w).reshape(-1, 3)[bodies]
      out["mocap_quat"][w] = row("body_quat", mjm.body_quat, w).reshape(-1, 4)[bodies]
      if k >= 0:
        out["mocap_pos"][w] = _f32(mjm.key_mpos)[k].reshape(nmocap, 3)
        out["mocap_quat"][w] = _f32(mjm.key_mquat)[k].reshape(nmocap, 4)
    for name, val in sleep.items():
      if name in out and out[name].size:
        out[name][w] = val
    if int(mjm.neq):
      out["eq_active"][w] = np.asarray(mjm.eq_active0)
    for name in COUNTERS:
      out[name][w] = 0
    if int(mjm.nhistory):
      out["history"][w] = history_row(mjm, time, np.ravel(row("timestep", mjm.opt.timestep, w))[0])
  if mask is None and keys is None:
    for name in GLOBAL_COUNTERS:
      out[name][...] = 0
  return out
