// set_const.hpp -- the constants MuJoCo derives from the (per-world batched) inertial parameters, recomputed on the device:
//   body_subtreemass                                   (mj_setConst "fixed" part, reference set_const.py:35-59)
//   dof_invweight0, body_invweight0, stat.meaninertia  (the qpos0-dependent part, reference set_const.py:170-190, 208-375)
// The float64 host restatement is mjcf.set_const; this is its float32 device twin, one launch for all model-worlds.
//
// MI355X mapping: ONE wavefront per model-world, one world per workgroup; everything between the model tables and the four outputs
// lives in the world's LDS slice (no Data array is read or written, no scratch in global memory).  Kinematics, com_pos and crb at qpos0
// are the stage functions of smooth.hpp, the factor is its sparse L'DL (factor_ld).  The diagonals of M^-1 and of J M^-1 J' are
// r' M^-1 r = |D^-1/2 L^-T r|^2 with ONE right-hand side per lane: nv unit vectors and six Jacobian rows per moving body.  A right-hand
// side is supported on the dof-ancestor chain of one dof (the dof itself / the body's last dof) and L^-T keeps it there, so a lane holds
// its vector in chain coordinates -- at most tree_nvmax words -- and walks the chain leaf to root: row k of L, restricted to the chain, is
// the row's own first entries (the chain of an ancestor is a prefix of the chain).  No atomics, no cross-lane traffic; the lanes loop
// when there are more than 64 right-hand sides.  Means over the translational / rotational triples are taken by a second pass over the
// per-item results.
#pragma once
#include "smooth.hpp"

struct SetConstLayout {
  int pos;      // PosLayout slice (with factor)
  int mass, submass, inertia, ipos, iquat, bpos, bquat, jpos, jaxis, armature;  // the world's row of every batched input field
  int boff;     // [nbody, 3] xipos - subtree_com[root]: the Jacobian's lever arm (xipos itself is overwritten by M)
  int res;      // [nv + 6 nbody] r' M^-1 r per right-hand side
  int x;        // [64, xstride] the lanes' vectors in chain coordinates
  int xstride;  // odd: the lanes' slices start on different banks
  int total;
};
__host__ __device__ inline SetConstLayout set_const_layout(int nq, int nv, int nbody, int njnt, int nC, int tree_nvmax) {
  SetConstLayout p;
  int o = mstruct_ints(nv, nC);
  p.pos = o; o += pos_layout(nq, nv, nbody, njnt, nC, true).total;
  p.mass = o; o += nbody;
  p.submass = o; o += nbody;
  p.inertia = o; o += 3 * nbody;
  p.ipos = o; o += 3 * nbody;
  p.iquat = o; o += 4 * nbody;
  p.bpos = o; o += 3 * nbody;
  p.bquat = o; o += 4 * nbody;
  p.jpos = o; o += 3 * njnt;
  p.jaxis = o; o += 3 * njnt;
  p.armature = o; o += nv;
  p.boff = o; o += 3 * nbody;
  p.res = o; o += nv + 6 * nbody;
  p.xstride = (tree_nvmax > 0 ? tree_nvmax : 1) | 1;
  p.x = o; o += 64 * p.xstride;
  p.total = o;
  return p;
}

// one wavefront, one model-world (blockIdx.x).  Outputs are [nbatch, ...]; a null pointer is not written.
DEV void set_const_body(const MjhModel& m, float* smem, float* out_subtreemass, float* out_dof_invweight0, float* out_body_invweight0, float* out_meaninertia,
                        int what) {
  constexpr int G = 64;
  const int nq = m.nq, nv = m.nv, nbody = m.nbody, njnt = m.njnt, nC = m.nC;
  const int w = blockIdx.x, lig = threadIdx.x;
  const SetConstLayout sl = set_const_layout(nq, nv, nbody, njnt, nC, m.tree_nvmax);
  const PosLayout lay = pos_layout(nq, nv, nbody, njnt, nC, true);
  const bool pos0 = (what & MJH_SET_CONST_0) != 0 && nv > 0;
  MStruct ms = MStruct{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (pos0) ms = load_mstruct<G>(m, reinterpret_cast<int*>(smem), G, false);
  float* S = smem + sl.pos;
  float *mass = smem + sl.mass, *submass = smem + sl.submass, *inertia = smem + sl.inertia, *ipos = smem + sl.ipos, *iquat = smem + sl.iquat,
        *bpos = smem + sl.bpos, *bquat = smem + sl.bquat, *jpos = smem + sl.jpos, *jaxis = smem + sl.jaxis, *armature = smem + sl.armature,
        *boff = smem + sl.boff, *res = smem + sl.res;
  float *qpos = S + lay.qpos, *xpos = S + lay.xpos, *xquat = S + lay.xquat, *xmat = S + lay.xmat, *xipos = S + lay.xipos, *ximat = S + lay.ximat,
        *xanchor = S + lay.xanchor, *xaxis = S + lay.xaxis, *scom = S + lay.scom, *cinert = S + lay.cinert, *cdof = S + lay.cdof,
        *crb = S + lay.crb, *M = S + lay.M, *L = S + lay.L, *dinv = S + lay.dinv;
  // the world's rows of the batched inputs (coalesced), with the M-structure above: one batch of loads
  gcopy<G>(mass, BF(m, body_mass, w), nbody, lig);
  if (pos0) {
    gcopy<G>(qpos, BF(m, qpos0, w), nq, lig);
    gcopy<G>(inertia, BF(m, body_inertia, w), 3 * nbody, lig);
    gcopy<G>(ipos, BF(m, body_ipos, w), 3 * nbody, lig);
    gcopy<G>(iquat, BF(m, body_iquat, w), 4 * nbody, lig);
    gcopy<G>(bpos, BF(m, body_pos, w), 3 * nbody, lig);
    gcopy<G>(bquat, BF(m, body_quat, w), 4 * nbody, lig);
    gcopy<G>(jpos, BF(m, jnt_pos, w), 3 * njnt, lig);
    gcopy<G>(jaxis, BF(m, jnt_axis, w), 3 * njnt, lig);
    gcopy<G>(armature, BF(m, dof_armature, w), nv, lig);
  }
  gsync();

  // ---- body_subtreemass: a subtree is a contiguous id range (depth-first numbering); ascending sum, fixed order ----
  for (int b = lig; b < nbody; b += G) {
    const int end = b + m.body_subtreenum[b];
    float s = 0.0f;
    for (int c = b; c < end; ++c) s += mass[c];
    submass[b] = s;
    if ((what & MJH_SET_CONST_FIXED) && out_subtreemass) out_subtreemass[(size_t)w * nbody + b] = s;
  }
  if (!(what & MJH_SET_CONST_0)) return;
  if (nv == 0) {  // nothing moves: meaninertia 1, every inverse weight 0 (mjcf.set_const)
    if (out_meaninertia && lig == 0) out_meaninertia[w] = 1.0f;
    if (out_body_invweight0)
      for (int i = lig; i < 2 * nbody; i += G) out_body_invweight0[(size_t)w * 2 * nbody + i] = 0.0f;
    return;
  }
  gsync();

  // ---- kinematics, com_pos, crb at qpos0 (smooth.hpp's stages; mocap bodies sit at their model pose like in mjcf.set_const) ----
  kin_levels<G>(m, false, nullptr, nullptr, qpos, qpos, bpos, bquat, jpos, jaxis, xpos, xquat, xanchor, xaxis, lig);
  body_frames<G>(nbody, ipos, iquat, xpos, xquat, xmat, xipos, ximat, lig);
  gsync();
  com_cinert_cdof<G>(nbody, njnt, mass, submass, inertia, m.body_subtreenum, m.body_rootid, m.jnt_bodyid, m.jnt_dofadr, m.jnt_type, xmat, xipos, ximat,
                     xanchor, xaxis, scom, cinert, cdof, lig);
  for (int b = lig; b < nbody; b += G) st3(boff + 3 * b, ld3(xipos + 3 * b) - ld3(scom + 3 * m.body_rootid[b]));
  gsync();
  crb_mass_matrix<G>(ms, nbody, nv, armature, m.body_subtreenum, m.dof_bodyid, m.dof_parentid, cinert, cdof, crb, M, lig);

  // ---- meaninertia = mean(diag M): ascending sum by one lane ----
  if (out_meaninertia && lig == 0) {
    float s = 0.0f;
    for (int i = 0; i < nv; ++i) s += M[ms.rowadr[i] + ms.rownnz[i] - 1];
    out_meaninertia[w] = s / (float)nv;
  }

  // ---- M = L' D L ----
  gcopy<G>(L, M, nC, lig);
  gsync();
  factor_ld<G>(ms, L, dinv, nv, lig, &m);

  // ---- r' M^-1 r, one right-hand side per lane ----
  float* x = smem + sl.x + lig * sl.xstride;
  const int nitem = nv + 6 * nbody;
  for (int it = lig; it < nitem; it += G) {
    int dof, row = -1, body = 0;
    if (it < nv) {
      dof = it;
    } else {
      body = (it - nv) / 6;
      row = (it - nv) - 6 * body;
      dof = m.body_weldid[body] == 0 ? -1 : m.body_lastdof[body];  // welded to the world / no dof up to the world: the row stays 0
    }
    float acc = 0.0f;
    if (dof >= 0) {
      const int start = ms.rowadr[dof], n = ms.rownnz[dof];
      if (row < 0) {
        for (int p = 0; p < n; ++p) x[p] = p == n - 1 ? 1.0f : 0.0f;
      } else {  // row of the body's 6 x nv Jacobian at xipos: translational rows 0..2, rotational rows 3..5 (mjcf.set_const)
        const V3 off = ld3(boff + 3 * body);
        for (int p = 0; p < n; ++p) {
          const float* c = cdof + 6 * ms.colind[start + p];
          const V3 ang = ld3(c), lin = ld3(c + 3);
          const V3 v = row < 3 ? lin + cross(ang, off) : ang;
          const int k = row < 3 ? row : row - 3;
          x[p] = k == 0 ? v.x : k == 1 ? v.y : v.z;
        }
      }
      for (int p = n - 1; p >= 0; --p) {  // x <- L^-T x along the chain, |.|^2 weighted by D^-1 on the way
        const int k = ms.colind[start + p];
        const float xk = x[p];
        acc += xk * xk * dinv[k];
        const float* Lk = L + ms.rowadr[k];
        for (int a = 0; a < p; ++a) x[a] -= Lk[a] * xk;
      }
    }
    res[it] = acc;
  }
  gsync();

  // ---- the means: a free joint's translational and rotational triples, a ball joint's triple, a body's two triples ----
  if (out_dof_invweight0) {
    float* out = out_dof_invweight0 + (size_t)w * nv;
    for (int j = lig; j < njnt; j += G) {
      const int d = m.jnt_dofadr[j], t = m.jnt_type[j];
      if (t == JNT_FREE || t == JNT_BALL) {
        const int ntriple = t == JNT_FREE ? 2 : 1;
        for (int g = 0; g < ntriple; ++g) {
          const float mean = (res[d + 3 * g] + res[d + 3 * g + 1] + res[d + 3 * g + 2]) / 3.0f;
          for (int k = 0; k < 3; ++k) out[d + 3 * g + k] = mean;
        }
      } else {
        out[d] = res[d];
      }
    }
  }
  if (out_body_invweight0) {
    float* out = out_body_invweight0 + (size_t)w * 2 * nbody;
    for (int b = lig; b < nbody; b += G) {
      const float* r = res + nv + 6 * b;
      float tr = (r[0] + r[1] + r[2]) / 3.0f, ro = (r[3] + r[4] + r[5]) / 3.0f;
      if (tr < MJ_MINVAL && ro > MJ_MINVAL) tr = ro;  // (a body that only slides / only turns: the other weight stands in)
      else if (ro < MJ_MINVAL && tr > MJ_MINVAL) ro = tr;
      out[2 * b] = tr;
      out[2 * b + 1] = ro;
    }
  }
}

// grid: one 64-thread workgroup per model-world
__global__ __launch_bounds__(64) void k_set_const(MjhModel m, float* out_subtreemass, float* out_dof_invweight0, float* out_body_invweight0,
                                                  float* out_meaninertia, int what) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  set_const_body(m, smem, out_subtreemass, out_dof_invweight0, out_body_invweight0, out_meaninertia, what);
}
