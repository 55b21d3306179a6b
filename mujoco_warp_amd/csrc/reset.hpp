// reset_data / reset_data_keyframe on the device (reference io.py reset_data, reset_data_keyframe): one launch rewrites the state of the worlds
// a per-world mask (and, optionally, a per-world keyframe index) selects, so that an RL loop resets finished episodes without a host trip and
// inside a captured graph.
//
// One wavefront per world.  The wavefront leaves at once when the world's mask entry is zero or -- in the per-world key form -- when its key is
// outside [0, nkey) (the reference's rule: such a world is not reset).  Otherwise its 64 lanes stride over each field, so that a field's stores
// are consecutive addresses of the world's row.  A reset only copies and fills: no LDS, no atomics, no barriers; every address is written by
// exactly one lane of the launch, and nothing outside the rows of the selected worlds is written (nacon / ncollision / ws_conadr belong to a
// reset of every world and are written only by the call without mask and keys).
//
// The history buffers' sample times are time - (n - k) timestep evaluated in double WITHOUT contraction (a product, then a difference: two roundings,
// then the cast to float): bit for bit what the host's initial state of Data.history is (mjcf.history_row).
#pragma once
#include "dev_common.hpp"

// the values of csrc/sleep.hpp (SLEEP_AWAKE_VAL = -(1 + mjMINAWAKE), SLEEP_AWAKE, SLEEP_STATIC), restated: that header brings k_sleep with it, and
// this unit is to hold k_reset alone
static constexpr int kResetTreeAsleep = -(1 + 10), kResetBodyAwake = 1, kResetBodyStatic = -1;

// the time of the sample `age` = n - k steps in the past
DEV float reset_history_time(float time, int age, float timestep) {
#pragma clang fp contract(off)  // a product and a difference, each rounded: the compiler's default would fuse them into one fma
  const double back = (double)age * (double)timestep;
  return (float)((double)time - back);
}
// one buffer of a world's row of Data.history in its initial state at `time`: [user 0, cursor n - 1, times[n], values[n * dim] 0]
DEV void reset_history_buffer(float* buf, int n, int dim, float time, float timestep, int lane) {
  const int size = 2 + n * (1 + dim);
  for (int j = lane; j < size; j += 64) {
    float v = 0.0f;
    if (j == 1) v = (float)(n - 1);
    else if (j >= 2 && j < 2 + n) v = reset_history_time(time, n - (j - 2), timestep);
    buf[j] = v;
  }
}

__global__ void __launch_bounds__(256) k_reset(MjhModel m, MjhData d, MjhReset r) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= d.nworld) return;
  if (r.mask_u8 && !r.mask_u8[w]) return;
  if (r.mask_i32 && !r.mask_i32[w]) return;
  int key = r.key;
  if (r.keys) {
    key = r.keys[w];
    if (key < 0 || key >= r.nkey) return;
  }
  const bool all = !r.mask_u8 && !r.mask_i32 && !r.keys;  // a reset of every world
  const size_t sw = (size_t)w;

  // ---- the state ----
  {
    const float* src = key >= 0 ? r.key_qpos + (size_t)key * m.nq : BF(m, qpos0, w);
    for (int i = lane; i < m.nq; i += 64) d.qpos[sw * m.nq + i] = src[i];
  }
  for (int i = lane; i < m.nv; i += 64) {
    d.qvel[sw * m.nv + i] = key >= 0 ? r.key_qvel[(size_t)key * m.nv + i] : 0.0f;
    d.qacc_warmstart[sw * m.nv + i] = 0.0f;
    d.qacc[sw * m.nv + i] = 0.0f;
    d.qfrc_applied[sw * m.nv + i] = 0.0f;
  }
  for (int i = lane; i < m.na; i += 64) d.act[sw * m.na + i] = key >= 0 ? r.key_act[(size_t)key * m.na + i] : 0.0f;
  for (int i = lane; i < m.nu; i += 64) d.ctrl[sw * m.nu + i] = key >= 0 ? r.key_ctrl[(size_t)key * m.nu + i] : 0.0f;
  for (int i = lane; i < 6 * m.nbody; i += 64) d.xfrc_applied[sw * 6 * m.nbody + i] = 0.0f;
  const float time = key >= 0 ? r.key_time[key] : 0.0f;
  if (lane == 0) d.time[w] = time;

  // ---- mocap poses: the model's, then the keyframe's ----
  if (m.nmocap > 0) {
    const bool from_key = key >= 0 && key < r.nkey_mocap;
    const float *body_pos = BF(m, body_pos, w), *body_quat = BF(m, body_quat, w);
    for (int i = lane; i < 3 * m.nmocap; i += 64) {
      const int k = i / 3, c = i - 3 * k;
      d.mocap_pos[sw * 3 * m.nmocap + i] = from_key ? r.key_mpos[(size_t)key * 3 * m.nmocap + i]
                                                    : body_pos[r.mocap_bodyid[k] * 3 + c];
    }
    for (int i = lane; i < 4 * m.nmocap; i += 64) {
      const int k = i >> 2, c = i & 3;
      d.mocap_quat[sw * 4 * m.nmocap + i] = from_key ? r.key_mquat[(size_t)key * 4 * m.nmocap + i]
                                                     : body_quat[r.mocap_bodyid[k] * 4 + c];
    }
  }

  // ---- sleeping: every tree fully awake (the tables a Data was made with) ----
  for (int t = lane; t < m.ntree; t += 64) {
    if (d.tree_asleep) d.tree_asleep[sw * m.ntree + t] = kResetTreeAsleep;
    if (d.tree_awake) d.tree_awake[sw * m.ntree + t] = 1;
    if (d.tree_island) d.tree_island[sw * m.ntree + t] = -1;
  }
  for (int b = lane; b < m.nbody; b += 64) {
    if (d.body_awake) d.body_awake[sw * m.nbody + b] = m.body_treeid[b] >= 0 || m.body_mocapid[m.body_rootid[b]] >= 0 ? kResetBodyAwake : kResetBodyStatic;
    if (d.body_awake_ind) d.body_awake_ind[sw * m.nbody + b] = b;
  }
  if (d.dof_awake_ind)
    for (int i = lane; i < m.nv; i += 64) d.dof_awake_ind[sw * m.nv + i] = i;

  for (int i = lane; i < m.neq; i += 64) d.eq_active[sw * m.neq + i] = r.eq_active0[i];

  // ---- per-world counters ----
  if (lane == 0) {
    if (d.ntree_awake) d.ntree_awake[w] = m.ntree;
    if (d.nbody_awake) d.nbody_awake[w] = m.nbody;
    if (d.nv_awake) d.nv_awake[w] = m.nv;
    if (d.nisland) d.nisland[w] = 0;
    d.nefc[w] = 0;
    d.ne[w] = 0;
    d.nf[w] = 0;
    d.nl[w] = 0;
    d.solver_niter[w] = 0;
    d.overflow[w] = 0;
    d.ws_ncon[w] = 0;
    d.ws_ncollision[w] = 0;
    if (all) {
      d.ws_conadr[w] = 0;
      if (w == 0) {
        d.nacon[0] = 0;
        d.ncollision[0] = 0;
      }
    }
  }

  // ---- the delay buffers in their initial state at the new time (actuator buffers, then sensor buffers: history.hpp) ----
  if (m.nhistory > 0) {
    float* row = d.history + sw * m.nhistory;
    const float timestep = BF(m, opt_timestep, w)[0];
    for (int u = 0; u < m.nu; ++u) {
      const int n = m.actuator_history[2 * u];
      if (n > 0) reset_history_buffer(row + m.actuator_historyadr[u], n, 1, time, timestep, lane);
    }
    for (int i = 0; i < m.nsensor; ++i) {
      const int n = m.sensor_history[2 * i];
      if (n > 0) reset_history_buffer(row + m.sensor_historyadr[i], n, m.sensor_dim[i], time, timestep, lane);
    }
  }
}
