// sensor_collision_tu.hip -- k_sensor_collision and its launcher (one translation unit of libmjhip.so, see host.hpp): the geom distance sensors
// run behind k_sensor of the position stage (mjhip.hip launch_sensor) and only for models that have one, so no step kernel of another model changes.
#include "host.hpp"

#include "sensor_collision.hpp"

int launch_sensor_collision(const MjhModel* m, const MjhData* d, hipStream_t s) {
  if (!m->sensor_collision_adr || !m->body_geomnum || !m->body_geomadr)
    return fail(MJH_E_ARG, "geom distance sensors: Model.sensor_collision_adr / body_geomnum / body_geomadr missing (INTEGRATION.md, additions within ABI v45)");
  if (m->nsensor_collision > m->nsensor) return fail(MJH_E_ARG, "geom distance sensors: nsensor_collision exceeds nsensor");
  if (!d->sensordata) return fail(MJH_E_ARG, "Data.sensordata missing (allocate Data with make_data/put_data)");
  const int wpb = 4;  // wavefronts = (world, sensor) items per workgroup
  const size_t lds = sizeof(float) * (size_t)sc_lds_words(std::max(m->ccd_iterations, m->epa_iterations)) * wpb;
  if (lds > 64 * 1024) return fail(MJH_E_UNSUPPORTED, "k_sensor_collision: the EPA polytopes of a workgroup do not fit in LDS");
  const long long items = (long long)d->nworld * m->nsensor_collision;
  hipLaunchKernelGGL(k_sensor_collision, dim3((unsigned)((items + wpb - 1) / wpb)), dim3(64 * wpb), lds, s, *m, *d);
  return MJH_OK;
}
