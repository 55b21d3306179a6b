// inverse.hpp -- inverse dynamics: the constraint forces at a GIVEN acceleration and the generalized force that produces it.
//
// Reference: inverse.py:129-146 (inv_constraint = solver.init_context without the gradient: Jaref = J qacc - aref, then the force update
// solver.py:1698-1822 and qfrc_constraint = J' force 1912-1947), inverse.py:59-76 (_qfrc_inverse), 79-119 (discrete_acc, Euler branch).
//
// MI355X mapping: one launch, one lane group per world, lane = dof (column of J).  The rows of efc_J are read ONCE, INV_B at a time: every
// lane multiplies the words of its column by qacc[i], the batch's J qacc comes from one csum_n (the dependent DPP chain is paid once per
// batch, not once per row), every lane then evaluates the batch's forces -- the same values in every lane of the group -- and accumulates
// qc_i += J[r][i] f_r from the words it still holds.  No second read of J, no atomics, no vector through global memory between the two
// products.  M qacc comes from the CSR rows of M as in k_solve_m.  Traffic per world: nefc * nv_pad * 4 bytes of J + O(nv + nefc).
#pragma once
#include "dev_common.hpp"  // csum_n
#include "smooth.hpp"      // MStruct, mul_m_ld
#include "solver.hpp"      // row_force, ell_zone

#define INV_B 8  // rows per batch: >= 6, so that the rows of an elliptic contact (condim 3 / 4 / 6) always fit in one

struct InvLayout {
  int vec, res, total;
};
__host__ __device__ inline InvLayout inv_layout(int nv) {
  InvLayout p;
  const int n = ((nv + 3) / 4) * 4;
  p.vec = 0;
  p.res = n;
  p.total = 2 * n;
  return p;
}

// G lanes per world, TT = ceil(nv_pad / G) trips over the columns (1 for G < 64).  qacc: the acceleration to evaluate at [nworld, nv];
// qfrc_inverse: [nworld, nv] or null (inv_constraint alone: no M qacc).  Writes efc_force, efc_state, qfrc_constraint.
template <int G, int TT>
__global__ void __launch_bounds__(256) k_inverse(MjhModel m, MjhData d, const float* qacc, float* qfrc_inverse) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nv = m.nv, nC = m.nC, nvp = d.nv_pad, njmax = d.njmax;
  const bool with_m = qfrc_inverse != nullptr;
  MStruct ms = MStruct{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (with_m) ms = load_mstruct<G>(m, reinterpret_cast<int*>(smem), blockDim.x);  // (whole workgroup; ends with a barrier)
  const int lig = threadIdx.x & (G - 1), gib = threadIdx.x / G;
  const int w = blockIdx.x * (blockDim.x / G) + gib;
  if (w >= d.nworld) return;
  const size_t vo = (size_t)w * nv, eo = (size_t)w * njmax;

  float qa[TT], qc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const int c = t * G + lig;
    qa[t] = c < nv ? qacc[vo + c] : 0.0f;
    qc[t] = 0.0f;
  }
  // ---- M qacc from the CSR rows of M (k_solve_m's product), left in LDS until the end ----------------------------------------------------
  float* res = nullptr;
  if (with_m) {
    const InvLayout lay = inv_layout(nv);
    float* S = smem + mstruct_ints(nv, nC) + (size_t)gib * lay.total;
    float* vec = S + lay.vec;
    res = S + lay.res;
#pragma unroll
    for (int t = 0; t < TT; ++t)
      if (t * G + lig < nv) vec[t * G + lig] = qa[t];
    gsync();
    mul_m_ld<G>(ms, d.M + (size_t)w * nC, vec, res, nv, lig);
    gsync();
  }

  // ---- one pass over efc_J ---------------------------------------------------------------------------------------------------------------
  const int nefc = min(d.nefc[w], njmax);
  const int ne = d.ne[w], nf = d.nf[w], nfric = ne + nf, ncon0 = nfric + d.nl[w];  // (equality | friction loss | limit | contact rows)
  const bool ell = m.cone == CONE_ELLIPTIC && d.nmaxpyramid > 1;
  const bool has_fl = nf > 0;
  const float impr = ell ? BF(m, opt_impratio_invsqrt, w)[0] : 1.0f;
  const float* Jg = d.efc_J + (size_t)w * d.njmax_pad * nvp;
  // the contact of an elliptic row: first row of its contact, rows of the contact that exist (0: not a row of a multi-row elliptic contact)
  auto ell_row = [&](int r, int& r0, int& dim) __attribute__((always_inline)) {
    r0 = r;
    dim = 0;
    if (!ell || r < ncon0 || r >= nefc) return (const float*)nullptr;
    const int cid = d.ws_efc_con[eo + r], c = cid >> 4;
    const float* cr = d.ws_contact + ((size_t)w * d.concap + c) * CON_STRIDE;
    const int* cri = reinterpret_cast<const int*>(cr);
    if (cri[24] <= 1) return (const float*)nullptr;
    r0 = r - (cid & 15);
    dim = min(cri[29], nefc - r0);
    return cr;
  };
  for (int rb = 0; rb < nefc;) {
    int re = min(rb + INV_B, nefc);
    {  // a contact's rows stay together: the batch ends in front of a contact it would cut (dim <= 6 < INV_B: the batch is never empty)
      int r0, dim;
      if (re < nefc && ell_row(re, r0, dim) && r0 > rb) re = min(re, r0);
    }
    float jw[INV_B][TT], ja[INV_B];
#pragma unroll
    for (int b = 0; b < INV_B; ++b) {
      ja[b] = 0.0f;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const int c = t * G + lig;
        jw[b][t] = (rb + b < re && c < nvp) ? Jg[(size_t)(rb + b) * nvp + c] : 0.0f;
        ja[b] += jw[b][t] * qa[t];
      }
    }
    csum_n<G, INV_B>(ja);
    float f[INV_B];
    int st[INV_B];
#pragma unroll
    for (int b = 0; b < INV_B; ++b) {
      const int r = rb + b;
      const bool has = r < re;
      const size_t k = eo + (has ? r : rb);
      const float D = has ? d.efc_D[k] : 0.0f;  // (padding rows, D = 0: no force)
      ja[b] = has ? ja[b] - d.efc_aref[k] : 0.0f;
      const int kind = r < ne ? 0 : (r < nfric ? 1 : 2);
      const float fl = (has_fl && kind == 1 && has) ? d.efc_frictionloss[k] : 0.0f;
      row_force(has ? kind : 3, ja[b], D, has_fl, &fl, f[b], st[b]);  // (3: no row -- no force, whatever the sign of ja)
    }
    if (ell) {
      // the rows of an elliptic contact decide together (zones: solver.hpp ell_zone; middle-zone forces as solver_big.hpp ell_contact)
#pragma unroll
      for (int b = 0; b < INV_B; ++b) {
        int r0, dim;
        const float* cr = ell_row(rb + b, r0, dim);
        if (!cr || r0 != rb + b || rb + b >= re) continue;
        const float mu = cr[14] * impr;
        const float dm = safe_div(d.efc_D[eo + r0], mu * mu * (1.0f + mu * mu));
        float u[6], rs[6];
        float tt = 0.0f;
        // (the batch cut keeps a contact's rows inside one batch, so b + j < INV_B holds for every j < dim at run time; the loops are unrolled
        // over all b and j, though, and the guard and the clamped index keep the register arrays' constant indices in range where b + j >= INV_B)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          rs[j] = j == 0 ? mu : cr[CON_FRICTION_WORD(j - 1)];
          u[j] = (j < dim && b + j < INV_B) ? ja[b + j < INV_B ? b + j : INV_B - 1] * rs[j] : 0.0f;
          if (j > 0) tt += u[j] * u[j];
        }
        const float N = u[0], T = tt <= 0.0f ? 0.0f : sqrtf(tt);
        const int zone = ell_zone(mu, N, T);
        const float fn = -dm * (N - mu * T) * mu;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          if (b + j >= INV_B) break;
          if (j < dim) {
            float fj = 0.0f;
            if (zone == ST_QUADRATIC) fj = -d.efc_D[eo + r0 + j] * ja[b + j];
            else if (zone == ST_CONE) fj = j == 0 ? fn : -safe_div(fn, T) * (u[j] * rs[j]);
            f[b + j] = fj;
            st[b + j] = zone;
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < INV_B; ++b) {
      if (lig == b && rb + b < re) {
        d.efc_force[eo + rb + b] = f[b];
        d.efc_state[eo + rb + b] = st[b];
      }
#pragma unroll
      for (int t = 0; t < TT; ++t) qc[t] += jw[b][t] * f[b];
    }
    rb = re;
  }

  // ---- qfrc_constraint, qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint (inverse.py:59-76) ----------------------------
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const int c = t * G + lig;
    if (c >= nv) continue;
    d.qfrc_constraint[vo + c] = qc[t];
    if (with_m) qfrc_inverse[vo + c] = res[c] + d.qfrc_bias[vo + c] - d.qfrc_passive[vo + c] - qc[t];
  }
}

// invdiscrete, Euler (inverse.py:79-119): qacc_c = M^-1 (M + h diag(dof_damping)) qacc, evaluated as qacc + M^-1 (h dof_damping qacc) -- the
// correction alone goes through the solve, so its rounding error scales with the correction and not with cond(M) |qacc|.
// add == 0: buf = h dof_damping Data.qacc (the right-hand side of the solve); add == 1: buf += Data.qacc (behind the solve)
__global__ void k_inverse_eulerdamp(MjhModel m, MjhData d, float* buf, int add) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, nv = m.nv;
  if (idx >= d.nworld * nv) return;
  const int w = idx / nv, i = idx - w * nv;
  if (add) buf[idx] += d.qacc[idx];
  else buf[idx] = BF(m, opt_timestep, w)[0] * BF(m, dof_damping, w)[i] * d.qacc[idx];
}
