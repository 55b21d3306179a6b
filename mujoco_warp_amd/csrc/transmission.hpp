// transmission.hpp -- general actuator transmissions (reference smooth.py _transmission, support.py jac_dof): joint targets of every
// joint type, jointinparent, site and site + refsite.  Launched only for models with MjhModel.trn_general (some moment row is not the
// scalar gear[0] of a hinge / slide joint); every other model keeps length and velocity inside fwd_vel_body and launches nothing here.
//
//   k_transmission   behind the position stage: Data.actuator_length [nworld, nu] and Data.actuator_moment [nworld, nJmom].  The sparse
//                    structure (rownnz / rowadr / colind, rows in actuator order, columns ascending: MuJoCo C's layout) depends on the model
//                    only and is compiled on the host (trn_tables.py moment_structure); the reference assigns rowadr with an atomic instead.
//   k_fwd_vel_trn    the velocity stage's TRN instantiation (smooth.hpp fwd_vel_body<G, true>): actuator_velocity = moment . qvel over the
//                    row, qfrc_actuator gathered per dof over the transpose lists -- fixed order, no atomics, independent of nworld.
//
// Mapping of k_transmission: one 32-lane group per world, eight worlds per 256-thread workgroup; lane l takes actuators l, l + 32, ... for the
// length and sparse entries l, l + 32, ... for the moment (an entry knows its actuator, its dof and which of the two sites the dof moves).
// Inputs are the position stage's outputs in global memory (site_xpos, site_xmat, xquat, subtree_com, cdof: a few hundred words per
// world, read once, L2 resident behind k_fwd_pos); nothing is shared between lanes, so there is no LDS and no barrier.
#pragma once
#include "smooth.hpp"

enum { TRN_JOINT = 0, TRN_JOINTINPARENT = 1, TRN_SITE = 4 };

// gear axis of a ball joint / rotational gear of a free joint: as given (joint) or rotated by the inverse joint quaternion (jointinparent)
DEV V3 trn_gear_axis(V3 axis, const float* quat, bool inparent) {
  if (!inparent) return axis;
  const Q4 q = quat_normalize(ld4(quat));
  return rot_vec_quat(axis, Q4{q.w, -q.x, -q.y, -q.z});
}

DEV float trn_length(const MjhModel& m, const MjhData& d, int w, int u) {
  const float* gear = BF(m, actuator_gear, w) + 6 * u;
  const int type = m.actuator_trntype[u], id0 = m.actuator_trnobj[2 * u], id1 = m.actuator_trnobj[2 * u + 1];
  if (type == TRN_JOINT || type == TRN_JOINTINPARENT) {
    const float* q = d.qpos + (size_t)w * m.nq + m.jnt_qposadr[id0];
    const int jt = m.jnt_type[id0];
    if (jt == JNT_FREE) return 0.0f;
    if (jt == JNT_BALL) return dot(quat_to_vel(quat_normalize(ld4(q))), trn_gear_axis(ld3(gear), q, type == TRN_JOINTINPARENT));
    return q[0] * gear[0];
  }
  if (id1 < 0) return 0.0f;  // site without refsite
  const float* sx = d.site_xpos + (size_t)w * m.nsite * 3;
  const float* rmat = d.site_xmat + ((size_t)w * m.nsite + id1) * 9;
  const V3 gt = ld3(gear), gr = ld3(gear + 3);
  float length = 0.0f;
  if (gt.x != 0.0f || gt.y != 0.0f || gt.z != 0.0f) length += dot(matT_mul(rmat, ld3(sx + 3 * id0) - ld3(sx + 3 * id1)), gt);
  if (gr.x != 0.0f || gr.y != 0.0f || gr.z != 0.0f) {
    // the two site quaternions from their bodies' (site_quat o xquat, the reference's order: smooth.py:2642)
    const float* sq = BF(m, site_quat, w);
    const float* xq = d.xquat + (size_t)w * m.nbody * 4;
    const Q4 quat = mul_quat(ld4(sq + 4 * id0), ld4(xq + 4 * m.site_bodyid[id0]));
    const Q4 refquat = mul_quat(ld4(sq + 4 * id1), ld4(xq + 4 * m.site_bodyid[id1]));
    length += dot(quat_sub(quat, refquat), gr);
  }
  return length;
}

DEV float trn_moment(const MjhModel& m, const MjhData& d, int w, int k) {
  const int u = m.moment_rowid[k], i = m.moment_colind[k];
  const float* gear = BF(m, actuator_gear, w) + 6 * u;
  const int type = m.actuator_trntype[u], id0 = m.actuator_trnobj[2 * u], id1 = m.actuator_trnobj[2 * u + 1];
  if (type == TRN_JOINT || type == TRN_JOINTINPARENT) {
    const int jt = m.jnt_type[id0], c = i - m.jnt_dofadr[id0];
    const float* q = d.qpos + (size_t)w * m.nq + m.jnt_qposadr[id0];
    if (jt == JNT_FREE) {
      if (c < 3 || type == TRN_JOINT) return gear[c];
      const V3 a = trn_gear_axis(ld3(gear + 3), q + 3, true);
      return c == 3 ? a.x : c == 4 ? a.y : a.z;
    }
    if (jt == JNT_BALL) {
      const V3 a = trn_gear_axis(ld3(gear), q, type == TRN_JOINTINPARENT);
      return c == 0 ? a.x : c == 1 ? a.y : a.z;
    }
    return gear[0];
  }
  // site: the wrench in the world frame through the refsite's frame (the site's own without one) ...
  const float* fmat = d.site_xmat + ((size_t)w * m.nsite + (id1 < 0 ? id0 : id1)) * 9;
  const V3 wt = mat_mul(fmat, ld3(gear)), wr = mat_mul(fmat, ld3(gear + 3));
  // ... against the dof's Jacobian column at the site it moves (jac_dof: cdof is taken about the subtree COM of the dof's tree root)
  const int side = m.moment_side[k];
  const V3 point = ld3(d.site_xpos + ((size_t)w * m.nsite + (side == 2 ? id1 : id0)) * 3);
  const V3 off = point - ld3(d.subtree_com + ((size_t)w * m.nbody + m.body_rootid[m.dof_bodyid[i]]) * 3);
  const float v = jac_dot(m, d.cdof + ((size_t)w * m.nv + i) * 6, off, wt, wr);
  return side == 2 ? -v : v;
}

__global__ void __launch_bounds__(256) k_transmission(MjhModel m, MjhData d) {
  constexpr int G = 32;
  const int lig = threadIdx.x & (G - 1), w = blockIdx.x * (256 / G) + threadIdx.x / G;
  if (w >= d.nworld) return;
  for (int u = lig; u < m.nu; u += G) d.actuator_length[(size_t)w * m.nu + u] = trn_length(m, d, w, u);
  for (int k = lig; k < m.nJmom; k += G) d.actuator_moment[(size_t)w * m.nJmom + k] = trn_moment(m, d, w, k);
}

template <int G>
__global__ void __launch_bounds__(256) k_fwd_vel_trn(MjhModel m, MjhData d, int first, int last) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  fwd_vel_body<G, true>(m, d, first, last, smem, blk_of_launch<G>());
}
