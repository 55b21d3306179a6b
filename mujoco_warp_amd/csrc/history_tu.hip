// history_tu.hip -- k_history_ctrl, k_history_sensor, k_history_read, k_history_init, their launchers and the entry points mjh_history_read /
// mjh_history_init (one translation unit of libmjhip.so, see host.hpp): actuator and sensor delays.  mjhip.hip calls the launchers only for
// models with MjhModel.nu_history / nsensor_history_* > 0, so no launch of another model changes.
#include "host.hpp"

#include "history.hpp"

static int history_check(const MjhModel* m, const MjhData* d) {
  if (m->nhistory <= 0 || !d->history) return fail(MJH_E_ARG, "Data.history missing (allocate Data with make_data/put_data; additions within ABI v45)");
  if (m->nu > 0 && (!m->actuator_history || !m->actuator_historyadr || !m->actuator_delay)) return fail(MJH_E_ARG, "Model.actuator_history / actuator_historyadr / actuator_delay missing");
  if (m->nsensor > 0 && (!m->sensor_history || !m->sensor_historyadr || !m->sensor_delay || !m->sensor_dim || !m->sensor_adr)) return fail(MJH_E_ARG, "Model.sensor_history / sensor_historyadr / sensor_delay missing");
  return MJH_OK;
}

int launch_history_ctrl(const MjhModel* m, const MjhData* d, int insert, hipStream_t s) {
  if (int rc = history_check(m, d)) return rc;
  if (!d->ctrl || !d->ws_ctrl_delayed || !d->time) return fail(MJH_E_ARG, "Data.ctrl / ws_ctrl_delayed / time missing (allocate Data with make_data/put_data)");
  const long long n = (long long)d->nworld * m->nu;
  if (n > 0x7fffffffLL) return fail(MJH_E_ARG, "k_history_ctrl: nworld * nu exceeds 2^31 - 1");
  if (n == 0) return MJH_OK;
  hipLaunchKernelGGL(k_history_ctrl, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *m, *d, (const float*)d->ctrl, insert);
  return MJH_OK;
}

int launch_history_sensor(const MjhModel* m, const MjhData* d, int stage, int insert, hipStream_t s) {
  const int nlist = stage == 0 ? m->nsensor_history_posvel : m->nsensor_history_acc;
  const int* list = stage == 0 ? m->sensor_history_posvel : m->sensor_history_acc;
  if (nlist <= 0) return MJH_OK;
  if (int rc = history_check(m, d)) return rc;
  if (!list || nlist > m->nsensor || !d->sensordata || !d->time) return fail(MJH_E_ARG, "Model.sensor_history_posvel / sensor_history_acc or Data.sensordata / time missing");
  const long long n = (long long)d->nworld * nlist;
  if (n > 0x7fffffffLL) return fail(MJH_E_ARG, "k_history_sensor: nworld * sensors exceeds 2^31 - 1");
  hipLaunchKernelGGL(k_history_sensor, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *m, *d, list, nlist, insert);
  return MJH_OK;
}

static int history_id_check(const char* who, const MjhModel* m, const MjhData* d, int is_sensor, int id) {
  if (!m || !d || d->nworld <= 0) return fail(MJH_E_ARG, "%s: null model / data", who);
  if (id < 0 || id >= (is_sensor ? m->nsensor : m->nu)) return fail(MJH_E_ARG, "%s: no such actuator / sensor", who);
  return MJH_OK;
}

#pragma GCC visibility push(default)
extern "C" int mjh_history_read(const MjhModel* m, const MjhData* d, int is_sensor, int id, const float* time, int interp, float* result, int result_stride,
                                void* stream) {
  if (int rc = history_id_check("mjh_history_read", m, d, is_sensor, id)) return rc;
  if (!time || !result || result_stride < 1) return fail(MJH_E_ARG, "mjh_history_read: null time / result");
  if (interp < -1 || interp > 2) return fail(MJH_E_ARG, "mjh_history_read: interp must be -1 (the model's), 0, 1 or 2");
  if (m->nhistory > 0) {
    if (int rc = history_check(m, d)) return rc;
  } else if (is_sensor ? !d->sensordata : !d->ctrl) {
    return fail(MJH_E_ARG, "mjh_history_read: Data.ctrl / sensordata missing");
  }
  hipLaunchKernelGGL(k_history_read, dim3((d->nworld + 255) / 256), dim3(256), 0, (hipStream_t)stream, *m, *d, is_sensor, id, time, interp, result, result_stride);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

extern "C" int mjh_history_init(const MjhModel* m, const MjhData* d, int is_sensor, int id, const float* times, const float* values, int values_stride,
                                const float* phase, void* stream) {
  if (int rc = history_id_check("mjh_history_init", m, d, is_sensor, id)) return rc;
  if (int rc = history_check(m, d)) return rc;
  if (!values || values_stride < 1) return fail(MJH_E_ARG, "mjh_history_init: null values");
  hipLaunchKernelGGL(k_history_init, dim3((d->nworld + 255) / 256), dim3(256), 0, (hipStream_t)stream, *m, *d, is_sensor, id, times, values, values_stride, phase);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
#pragma GCC visibility pop
