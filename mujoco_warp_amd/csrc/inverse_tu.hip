// inverse_tu.hip -- k_inverse, k_inverse_eulerdamp and their launchers (one translation unit of libmjhip.so, see host.hpp): inverse dynamics.
// Nothing of a step launches them; mjh_inverse / mjh_inv_constraint (mjhip.hip) do.
#include "host.hpp"

#include "contact_rec.hpp"
#include "inverse.hpp"

template <int G, int TT>
static int launch_inverse_t(const MjhModel* m, const MjhData* d, const float* qacc, float* qfrc_inverse, hipStream_t s) {
  size_t lds;
  const int threads = pick_block(sizeof(int) * mstruct_ints(m->nv, m->nC), sizeof(float) * inv_layout(m->nv).total, G, &lds);
  if (!threads) return fail(MJH_E_UNSUPPORTED, "k_inverse: model does not fit in LDS");
  HIPCHK(set_lds((k_inverse<G, TT>), lds));
  const int wpb = threads / G;
  hipLaunchKernelGGL((k_inverse<G, TT>), dim3((d->nworld + wpb - 1) / wpb), dim3(threads), lds, s, *m, *d, qacc, qfrc_inverse);
  return MJH_OK;
}

// G: lanes per world, as the caller chooses them for k_make_constraint / k_mid (16 / 32 / 64)
int launch_inverse(const MjhModel* m, const MjhData* d, const float* qacc, float* qfrc_inverse, int G, hipStream_t s) {
  if (!qacc) return fail(MJH_E_ARG, "k_inverse: null qacc");
  if (m->nv == 0) return MJH_OK;
  if (!d->efc_J || !d->efc_D || !d->efc_aref || !d->efc_frictionloss || !d->efc_force || !d->efc_state || !d->nefc || !d->ne || !d->nf || !d->nl || !d->qfrc_constraint ||
      !d->M || !d->qfrc_bias || !d->qfrc_passive || !d->ws_efc_con || !d->ws_contact)
    return fail(MJH_E_ARG, "k_inverse: a constraint / dynamics array of Data is missing (allocate Data with make_data/put_data)");
  const int nvp = d->nv_pad;
  if (G == 16 && nvp <= 16) return launch_inverse_t<16, 1>(m, d, qacc, qfrc_inverse, s);
  if (G <= 32 && nvp <= 32) return launch_inverse_t<32, 1>(m, d, qacc, qfrc_inverse, s);
  const int trips = (nvp + 63) / 64;  // (64 lanes: the J words of a batch stay in registers, INV_B per trip)
  if (trips <= 1) return launch_inverse_t<64, 1>(m, d, qacc, qfrc_inverse, s);
  if (trips <= 2) return launch_inverse_t<64, 2>(m, d, qacc, qfrc_inverse, s);
  if (trips <= 4) return launch_inverse_t<64, 4>(m, d, qacc, qfrc_inverse, s);
  return fail(MJH_E_UNSUPPORTED, "k_inverse: more than 256 dofs are not supported");
}

int launch_inverse_eulerdamp(const MjhModel* m, const MjhData* d, float* buf, int add, hipStream_t s) {
  const int n = d->nworld * m->nv;
  if (n > 0) hipLaunchKernelGGL(k_inverse_eulerdamp, dim3((n + 255) / 256), dim3(256), 0, s, *m, *d, buf, add);
  return MJH_OK;
}
