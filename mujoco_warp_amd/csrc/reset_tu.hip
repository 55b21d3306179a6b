// reset_tu.hip -- k_reset, its launcher and the entry point mjh_reset (one translation unit of libmjhip.so, see host.hpp): reset_data /
// reset_data_keyframe on the device.  Nothing of the step launches it; mjh_graph_create_reset (mjhip.hip) captures the launcher in front of a step.
#include "host.hpp"

#include "reset.hpp"

int launch_reset(const MjhModel* m, const MjhData* d, const MjhReset* r, hipStream_t s) {
  if (!m || !d || !r || d->nworld <= 0) return fail(MJH_E_ARG, "mjh_reset: null model / data / reset arguments");
  if (r->mask_u8 && r->mask_i32) return fail(MJH_E_ARG, "mjh_reset: two masks given");
  if (r->nkey < 0 || r->nkey_mocap < 0 || r->nkey_mocap > r->nkey) return fail(MJH_E_ARG, "mjh_reset: bad keyframe counts");
  if (!r->keys && (r->key < -1 || r->key >= r->nkey)) return fail(MJH_E_ARG, "mjh_reset: keyframe out of range");
  if (r->keys || r->key >= 0) {  // a keyframe may be read
    if ((m->nq > 0 && !r->key_qpos) || (m->nv > 0 && !r->key_qvel) || (m->na > 0 && !r->key_act) || (m->nu > 0 && !r->key_ctrl) || !r->key_time)
      return fail(MJH_E_ARG, "mjh_reset: a keyframe table (key_qpos / key_qvel / key_act / key_ctrl / key_time) is missing");
    if (r->nkey_mocap > 0 && m->nmocap > 0 && (!r->key_mpos || !r->key_mquat)) return fail(MJH_E_ARG, "mjh_reset: key_mpos / key_mquat missing");
  }
  if (!d->time || (m->nq > 0 && !d->qpos) || (m->nv > 0 && (!d->qvel || !d->qacc_warmstart || !d->qacc || !d->qfrc_applied)) || (m->na > 0 && !d->act) ||
      (m->nu > 0 && !d->ctrl) || (m->nbody > 0 && !d->xfrc_applied))
    return fail(MJH_E_ARG, "mjh_reset: a state array of Data is missing (allocate Data with make_data/put_data)");
  if (!d->nefc || !d->ne || !d->nf || !d->nl || !d->solver_niter || !d->overflow || !d->ws_ncon || !d->ws_ncollision || !d->ws_conadr || !d->nacon || !d->ncollision)
    return fail(MJH_E_ARG, "mjh_reset: a counter of Data is missing (allocate Data with make_data/put_data)");
  if (m->nmocap > 0 && (!d->mocap_pos || !d->mocap_quat || !r->mocap_bodyid || !m->body_pos || !m->body_quat)) return fail(MJH_E_ARG, "mjh_reset: mocap arrays missing");
  if (m->neq > 0 && (!d->eq_active || !r->eq_active0)) return fail(MJH_E_ARG, "mjh_reset: eq_active / eq_active0 missing");
  if (d->body_awake && (!m->body_treeid || !m->body_mocapid || !m->body_rootid)) return fail(MJH_E_ARG, "mjh_reset: Model.body_treeid / body_mocapid / body_rootid missing");
  if (m->qpos0_nb < 1 || m->body_pos_nb < 1 || m->body_quat_nb < 1 || m->opt_timestep_nb < 1 || !m->qpos0 || !m->opt_timestep)
    return fail(MJH_E_ARG, "mjh_reset: Model.qpos0 / opt_timestep or a batch count is missing");
  if (m->nhistory > 0) {
    if (!d->history) return fail(MJH_E_ARG, "mjh_reset: Data.history missing (allocate Data with make_data/put_data)");
    if ((m->nu > 0 && (!m->actuator_history || !m->actuator_historyadr)) || (m->nsensor > 0 && (!m->sensor_history || !m->sensor_historyadr || !m->sensor_dim)))
      return fail(MJH_E_ARG, "mjh_reset: Model.actuator_history / sensor_history tables missing");
  }
  hipLaunchKernelGGL(k_reset, dim3((unsigned)((d->nworld + 3) / 4)), dim3(256), 0, s, *m, *d, *r);
  return MJH_OK;
}

#pragma GCC visibility push(default)
extern "C" int mjh_reset(const MjhModel* m, const MjhData* d, const MjhReset* r, void* stream) {
  if (int rc = launch_reset(m, d, r, (hipStream_t)stream)) return rc;
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
#pragma GCC visibility pop
