// transmission_tu.hip -- k_transmission, k_fwd_vel_trn and their launchers (one translation unit of libmjhip.so, see host.hpp): the general
// actuator transmissions.  mjhip.hip calls them only for models with MjhModel.trn_general, so no kernel of another model changes.
#include "host.hpp"

#include "transmission.hpp"

static int trn_check(const MjhModel* m, const MjhData* d) {
  if (!m->actuator_trntype || !m->actuator_trnobj || !m->moment_rownnz || !m->moment_rowadr || !m->momentT_adr ||
      (m->nJmom > 0 && (!m->moment_colind || !m->moment_rowid || !m->moment_side || !m->momentT_act || !m->momentT_ind)))
    return fail(MJH_E_ARG, "general transmissions: Model.actuator_trntype / actuator_trnobj / moment_* / momentT_* missing (INTEGRATION.md, additions within ABI v45)");
  if (m->nJmom < 0 || m->nu < 1) return fail(MJH_E_ARG, "general transmissions: bad nu / nJmom");
  if (!d->actuator_length || (m->nJmom > 0 && !d->actuator_moment)) return fail(MJH_E_ARG, "Data.actuator_length / actuator_moment missing (allocate Data with make_data/put_data)");
  return MJH_OK;
}

int launch_transmission(const MjhModel* m, const MjhData* d, hipStream_t s) {
  if (int rc = trn_check(m, d)) return rc;
  hipLaunchKernelGGL(k_transmission, dim3((d->nworld + 7) / 8), dim3(256), 0, s, *m, *d);
  return MJH_OK;
}

template <int G>
static int launch_vel_trn_g(const MjhModel* m, const MjhData* d, int first, int last, hipStream_t s) {
  const VelLayout lay = vel_layout(m->nq, m->nv, m->nbody, m->nC, m->nu);
  size_t lds;
  const int threads = pick_block(sizeof(int) * mstruct_ints(m->nv, m->nC), sizeof(float) * lay.total, G, &lds);
  if (!threads) return fail(MJH_E_UNSUPPORTED, "k_fwd_vel_trn: model does not fit in LDS");
  HIPCHK(set_lds(k_fwd_vel_trn<G>, lds));
  const int wpb = threads / G;
  hipLaunchKernelGGL(k_fwd_vel_trn<G>, dim3((d->nworld + wpb - 1) / wpb), dim3(threads), lds, s, *m, *d, first, last);
  return MJH_OK;
}
int launch_vel_trn(const MjhModel* m, const MjhData* d, int first, int last, bool lanes64, hipStream_t s) {
  if (int rc = trn_check(m, d)) return rc;
  return lanes64 ? launch_vel_trn_g<64>(m, d, first, last, s) : launch_vel_trn_g<32>(m, d, first, last, s);
}
