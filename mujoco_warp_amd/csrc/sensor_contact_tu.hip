// sensor_contact_tu.hip -- k_sensor_contact and its launcher (one translation unit of libmjhip.so, see host.hpp): the contact sensors run behind
// k_sensor of the acceleration stage (mjhip.hip launch_sensor) and only for models that have one, so no step kernel of another model changes.
#include "host.hpp"

#include "sensor_contact.hpp"

int launch_sensor_contact(const MjhModel* m, const MjhData* d, hipStream_t s) {
  if (!m->sensor_intprm || !m->sensor_contact_adr) return fail(MJH_E_ARG, "contact sensors: Model.sensor_intprm / sensor_contact_adr missing (INTEGRATION.md, additions within ABI v45)");
  if (m->nsensor_contact > m->nsensor) return fail(MJH_E_ARG, "contact sensors: nsensor_contact exceeds nsensor");
  if (m->contact_sensor_maxmatch < 1 || m->contact_sensor_maxmatch > 64)
    return fail(MJH_E_UNSUPPORTED, "contact sensors: contact_sensor_maxmatch must be in 1..64 (one wavefront holds the matches of a world's sensor)");
  if (!d->sensordata) return fail(MJH_E_ARG, "Data.sensordata missing (allocate Data with make_data/put_data)");
  const int wpb = 4;  // wavefronts = worlds per workgroup
  const size_t lds = sizeof(float) * (size_t)cs_lds_words(d->concap) * wpb;
  if (lds > 64 * 1024) return fail(MJH_E_UNSUPPORTED, "k_sensor_contact: the per-world contact capacity does not fit in LDS");
  hipLaunchKernelGGL(k_sensor_contact, dim3((d->nworld + wpb - 1) / wpb), dim3(64 * wpb), lds, s, *m, *d);
  return MJH_OK;
}
