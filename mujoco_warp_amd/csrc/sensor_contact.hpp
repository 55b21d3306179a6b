// Contact sensors (reference sensor.py:1810-2009 the slots and netforce, 2315-2471 matching / direction / criteria, 2475-2508 the sort):
// "which contacts involve this geom / body / subtree / site volume", answered with found / force / torque / dist / pos / normal / tangent of
// the first, nearest or strongest `num` matches, or with their net wrench.
//
// One wavefront per world (four worlds per 256-thread workgroup); the wavefront loops over the model's contact sensors.  Wave64 and the cap
// of 64 kept matches per (world, sensor) fit each other: after matching, lane k owns match k.
//   1. the six-component contact-frame force of every record of the world is decoded ONCE into LDS (same decoding as k_rne_postconstraint /
//      k_contact_force; skipped when no contact sensor of the model reads a force);
//   2. per sensor the records are walked in chunks of 64, one record per lane; a chunk's matches are numbered with a ballot and the popcount
//      of the lower lanes, so the numbering is the world's contact order (= the order of the public contact arrays) without any atomic --
//      the reference numbers them by atomic arrival;
//   3. mindist / maxforce: every lane counts, over at most 64 broadcast LDS reads, the kept matches that precede its own under (criterion,
//      match index): that count is its position in a STABLE sort;
//   4. lanes whose position is below `num` write their slot, the remaining slots of the sensor are zeroed; netforce sums by a fixed-order
//      butterfly (gsum<64>) and fills one slot.
// Inputs: the contact records d.ws_contact (the public contact.* arrays are published off the critical path and may not be there yet),
// efc_force, geom_bodyid, body_parentid, site pose / type / size.  The only global atomic is the atomicOr of OVF_CONTACT_MATCH.
// LDS per wavefront: cs_lds_words(concap) floats = 7 concap (forces, odd stride: conflict-free lane-per-record access) + 64 (match list) + 64
// (criteria); 7.5 KB per world at concap = 256.
// Not built: contact_sensor_maxmatch > 64, sensor noise, cutoff (the reference applies none to contact sensors).
#pragma once
#include "dev_common.hpp"
#include "site_inside.hpp"

#define OVF_CONTACT_MATCH (1 << 6) /* OverflowType.CONTACT_MATCH (types.py) */
#define CS_FSTRIDE 7
enum { CS_OBJ_UNKNOWN = 0, CS_OBJ_BODY = 1, CS_OBJ_XBODY = 2, CS_OBJ_GEOM = 5, CS_OBJ_SITE = 6 };
enum { CS_FOUND = 1, CS_FORCE = 2, CS_TORQUE = 4, CS_DIST = 8, CS_POS = 16, CS_NORMAL = 32, CS_TANGENT = 64 };
enum { CS_REDUCE_NONE = 0, CS_REDUCE_MINDIST = 1, CS_REDUCE_MAXFORCE = 2, CS_REDUCE_NETFORCE = 3 };

// floats of LDS per wavefront (a multiple of 4: every wavefront's base stays 16-byte aligned)
__host__ __device__ static inline int cs_lds_words(int concap) { return (CS_FSTRIDE * concap + 128 + 3) & ~3; }

// floats of one slot
DEV int cs_slot_size(int spec) {
  return ((spec & CS_FOUND) ? 1 : 0) + ((spec & CS_FORCE) ? 3 : 0) + ((spec & CS_TORQUE) ? 3 : 0) + ((spec & CS_DIST) ? 1 : 0) + ((spec & CS_POS) ? 3 : 0) + ((spec & CS_NORMAL) ? 3 : 0) +
         ((spec & CS_TANGENT) ? 3 : 0);
}

// sensor.py:2315-2330 _check_match: is (body, geom), one side of a contact, the sensor's object
DEV bool cs_check(const int* body_parentid, int body, int geom, int objtype, int objid) {
  if (objtype == CS_OBJ_UNKNOWN || objtype == CS_OBJ_SITE) return true;  // (a site has passed its volume test)
  if (objtype == CS_OBJ_GEOM) return objid == geom;
  if (objtype == CS_OBJ_BODY) return objid == body;
  if (objtype == CS_OBJ_XBODY) {  // subtree: bodies are numbered depth first, so walking up ends at or below objid
    while (body > objid) body = body_parentid[body];
    return body == objid;
  }
  return false;
}

// support.py:445 contact_force in the contact frame, from the record (a contact that got no rows reads zero)
DEV void cs_decode(const MjhModel& m, const MjhData& d, const float* rec, const float* efc_force, float* f) {
  const int* reci = reinterpret_cast<const int*>(rec);
  const int condim = reci[24], adr0 = reci[28];
#pragma unroll
  for (int k = 0; k < 6; ++k) f[k] = 0.0f;
  if (adr0 < 0) return;
  if (m.cone == CONE_PYRAMIDAL) {
    if (condim == 1) f[0] = adr0 < d.njmax ? efc_force[adr0] : 0.0f;
    else {
#pragma unroll
      for (int i = 0; i < 5; ++i)
        if (i < condim - 1) {
          const int a = adr0 + 2 * i;
          const float d1 = a < d.njmax ? efc_force[a] : 0.0f, d2 = a + 1 < d.njmax ? efc_force[a + 1] : 0.0f;
          f[0] += d1 + d2;
          f[i + 1] = (d1 - d2) * rec[CON_FRICTION_WORD(i)];
        }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i)
      if (i < condim && adr0 + i < d.njmax) f[i] = efc_force[adr0 + i];
  }
}

__global__ void __launch_bounds__(256) k_sensor_contact(MjhModel m, MjhData d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int w = blockIdx.x * (blockDim.x >> 6) + wib;
  if (w >= d.nworld) return;  // (whole wavefronts leave: nothing below synchronises the workgroup)
  float* frc = smem + (size_t)wib * cs_lds_words(d.concap);
  int* mrec = reinterpret_cast<int*>(frc + CS_FSTRIDE * d.concap);
  float* crit = frc + CS_FSTRIDE * d.concap + 64;
  const int ncon = (d.ws_ncon && d.ws_contact) ? min(d.ws_ncon[w], d.concap) : 0;
  const float* recs = d.ws_contact + (size_t)w * d.concap * CON_STRIDE;
  const float* efc_force = d.efc_force + (size_t)w * d.njmax;
  const int maxmatch = min(max(m.contact_sensor_maxmatch, 1), 64), ncs = m.nsensor_contact;

  bool need_force = false;  // (uniform: model tables only)
  for (int k = 0; k < ncs; ++k) {
    const int i = m.sensor_contact_adr[k];
    need_force = need_force || (m.sensor_intprm[3 * i] & (CS_FORCE | CS_TORQUE)) || m.sensor_intprm[3 * i + 1] >= CS_REDUCE_MAXFORCE;
  }
  if (need_force)
    for (int c = lane; c < ncon; c += 64) {
      float f[6];
      cs_decode(m, d, recs + c * CON_STRIDE, efc_force, f);
#pragma unroll
      for (int k = 0; k < 6; ++k) frc[CS_FSTRIDE * c + k] = f[k];
    }
  gsync();

  for (int k = 0; k < ncs; ++k) {
    const int i = m.sensor_contact_adr[k];
    const int objtype = m.sensor_objtype[i], objid = m.sensor_objid[i], reftype = m.sensor_reftype[i], refid = m.sensor_refid[i];
    const int spec = m.sensor_intprm[3 * i], reduce = m.sensor_intprm[3 * i + 1], num = m.sensor_intprm[3 * i + 2], size = cs_slot_size(spec);
    float* out = d.sensordata + (size_t)w * m.nsensordata + m.sensor_adr[i];
    V3 spos = V3{0, 0, 0}, ssize = V3{0, 0, 0};
    const float* smat = nullptr;
    int stype = -1;
    if (objtype == CS_OBJ_SITE) {
      spos = ld3(d.site_xpos + ((size_t)w * m.nsite + objid) * 3);
      smat = d.site_xmat + ((size_t)w * m.nsite + objid) * 9;
      ssize = ld3(m.site_size + 3 * objid);
      stype = m.site_type[objid];
    }

    // ---- match: contact order, the first maxmatch kept (sensor.py:2391-2446)
    int found = 0;
    for (int c0 = 0; c0 < ncon; c0 += 64) {
      const int c = c0 + lane;
      bool match = false, neg = false;
      if (c < ncon) {
        const float* rec = recs + c * CON_STRIDE;
        const int* reci = reinterpret_cast<const int*>(rec);
        match = objtype != CS_OBJ_SITE || cs_inside(stype, ssize, spos, smat, ld3(rec + 1));
        if (match && (objtype != CS_OBJ_UNKNOWN || reftype != CS_OBJ_UNKNOWN)) {
          const int g1 = reci[25], g2 = reci[26], b1 = m.geom_bodyid[g1], b2 = m.geom_bodyid[g2];
          const bool m11 = cs_check(m.body_parentid, b1, g1, objtype, objid), m12 = cs_check(m.body_parentid, b2, g2, objtype, objid);
          const bool m21 = cs_check(m.body_parentid, b1, g1, reftype, refid), m22 = cs_check(m.body_parentid, b2, g2, reftype, refid);
          match = (m11 || m12) && (m21 || m22);
          if (objtype != CS_OBJ_UNKNOWN && reftype != CS_OBJ_UNKNOWN) {
            const bool regular = m11 && m22, reverse = m12 && m21;
            match = match && (regular || reverse);
            neg = reverse && !regular;
          } else if (objtype != CS_OBJ_UNKNOWN) neg = !m11;
          else neg = !m22;
        }
      }
      int total;
      const int pos = found + grank<64>(match, lane, total);
      if (match && pos < maxmatch) mrec[pos] = c | (neg ? 0x40000000 : 0);
      found += total;
    }
    const int nmatch = min(found, maxmatch);
    if (found > maxmatch && lane == 0) atomicOr(d.overflow + w, OVF_CONTACT_MATCH);
    gsync();

    // ---- lane k owns match k
    const bool own = lane < nmatch;
    const int e = own ? mrec[lane] : 0, c = e & 0xffff;
    const float dir = (e & 0x40000000) ? -1.0f : 1.0f;
    const float* rec = recs + c * CON_STRIDE;
    float f[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (own && need_force) {
#pragma unroll
      for (int q = 0; q < 6; ++q) f[q] = frc[CS_FSTRIDE * c + q];
    }
    const float fsq = f[0] * f[0] + f[1] * f[1] + f[2] * f[2];

    if (reduce == CS_REDUCE_NETFORCE) {  // sensor.py:1857-1945
      V3 p = V3{0, 0, 0}, fg = V3{0, 0, 0}, tg = V3{0, 0, 0};
      float wgt = 0.0f;
      if (own) {
        const float* R = rec + 4;  // frame rows: normal, tangent 1, tangent 2
        wgt = sqrtf(fsq);
        p = ld3(rec + 1);
        fg = V3{f[0] * R[0] + f[1] * R[3] + f[2] * R[6], f[0] * R[1] + f[1] * R[4] + f[2] * R[7], f[0] * R[2] + f[1] * R[5] + f[2] * R[8]} * dir;
        tg = V3{f[3] * R[0] + f[4] * R[3] + f[5] * R[6], f[3] * R[1] + f[4] * R[4] + f[5] * R[7], f[3] * R[2] + f[4] * R[5] + f[5] * R[8]} * dir + cross(p, fg);
      }
      const float sw = gsum<64>(wgt);
      V3 np = V3{gsum<64>(wgt * p.x), gsum<64>(wgt * p.y), gsum<64>(wgt * p.z)};
      const V3 nf = V3{gsum<64>(fg.x), gsum<64>(fg.y), gsum<64>(fg.z)};
      V3 nt = V3{gsum<64>(tg.x), gsum<64>(tg.y), gsum<64>(tg.z)};
      np = np * (1.0f / fmaxf(sw, MJ_MINVAL));
      nt = nt - cross(np, nf);  // about the centroid instead of the origin
      if (lane == 0) {
        float* o = out;
        if (spec & CS_FOUND) *o++ = (float)nmatch;
        if (spec & CS_FORCE) { st3(o, nf); o += 3; }
        if (spec & CS_TORQUE) { st3(o, nt); o += 3; }
        if (spec & CS_DIST) *o++ = 0.0f;
        if (spec & CS_POS) { st3(o, np); o += 3; }
        if (spec & CS_NORMAL) { st3(o, V3{1.0f, 0.0f, 0.0f}); o += 3; }
        if (spec & CS_TANGENT) st3(o, V3{0.0f, 1.0f, 0.0f});
      }
      for (int idx = size + lane; idx < num * size; idx += 64) out[idx] = 0.0f;  // (slots the reference leaves untouched)
      gsync();  // (the next sensor overwrites mrec)
      continue;
    }

    // ---- position of the lane's match in a stable sort by the criterion (sensor.py:2448-2468, 2475-2508)
    int rank = lane;
    if (reduce == CS_REDUCE_MINDIST || reduce == CS_REDUCE_MAXFORCE) {
      const float cr = own ? (reduce == CS_REDUCE_MINDIST ? rec[0] : -fsq) : 0.0f;
      crit[lane] = cr;
      gsync();
      rank = 0;
      for (int j = 0; j < nmatch; ++j) {
        const float cj = crit[j];
        rank += (cj < cr || (cj == cr && j < lane)) ? 1 : 0;
      }
      gsync();  // (the next sensor overwrites crit)
    }
    // ---- slots (sensor.py:1947-2009)
    if (own && rank < num) {
      float* o = out + rank * size;
      if (spec & CS_FOUND) *o++ = (float)nmatch;
      if (spec & CS_FORCE) { st3(o, V3{f[0], f[1], dir * f[2]}); o += 3; }
      if (spec & CS_TORQUE) { st3(o, V3{f[3], f[4], dir * f[5]}); o += 3; }
      if (spec & CS_DIST) *o++ = rec[0];
      if (spec & CS_POS) { st3(o, ld3(rec + 1)); o += 3; }
      if (spec & CS_NORMAL) { st3(o, ld3(rec + 4) * dir); o += 3; }
      if (spec & CS_TANGENT) st3(o, ld3(rec + 7) * dir);
    }
    for (int idx = min(nmatch, num) * size + lane; idx < num * size; idx += 64) out[idx] = 0.0f;
    gsync();  // (the next sensor overwrites mrec)
  }
}
