// Geom distance sensors (reference sensor.py:642-718 <distance> / <normal> / <fromto>, mjSENS_GEOMDIST / GEOMNORMAL / GEOMFROMTO; the
// collision-sensor branch of collision_convex.py:814-861): the smallest signed surface-to-surface distance over the geom pairs (g1 of side 1,
// g2 of side 2) of a sensor -- a side is one geom or the geoms of one body --, negative when the geoms penetrate, with the witness points
// `from` on the side-1 geom and `to` on the side-2 geom of the minimising pair.  Geom margins play no part.
//
// One wavefront per (world, sensor), four of them in a 256-thread workgroup; nothing synchronises the workgroup.
//   1. the lanes stride over the n1 x n2 pairs, 64 per trip.  A lane orders its pair as the colliders do (lower geom type first, then lower
//      id), so that (A, B) and (B, A) run the same arithmetic, and runs ccd_gjk_phase in registers with the sensor's cutoff (spheres and
//      capsules shrink to their point / segment there), in its GUARD instantiation: a reading is used as a number, so the float32 failures
//      of the sub-distance solve on curved rims, which a contact survives, are caught (convex.hpp ccd_gjk).  A plane never goes through GJK: with n the plane's normal and s the geom's support
//      point along -n, d = n . (s - plane point), witnesses s - d n on the plane and s on the geom.
//   2. lanes whose pair penetrates are served one after the other by the WHOLE wavefront through ccd_epa_phase<64> (a loop over the ballot:
//      uniform control flow): the pair index, the simplex and the mesh vertex caches are broadcast from the owning lane, every lane rebuilds
//      the two geoms from the pair index, the polytope lives in the wavefront's LDS (ccd_poly_words floats, stride 1: 8.8 KB at the cap of 64
//      iterations).  An EPA that gives up leaves the pair out; what it reports (OverflowType.EPA_HORIZON) goes to the world's overflow word.
//   3. every lane keeps the best (distance, pair index) of its trips; one butterfly of __shfl_xor finds the minimum and, among equals, the
//      lowest pair index -- independent of how pairs fell on lanes.  No LDS round trip.
//   4. the winning lane un-swaps its witnesses and stores 1 / 3 / 6 floats: distance = min(d, cutoff) clamped to [-cutoff, cutoff] for a
//      positive cutoff, min(d, 0) for cutoff 0; normal = normalize(to - from) and fromto = (from, to), zeros when no pair is below the
//      cutoff, never clamped.
// Inputs: Data.geom_xpos / geom_xmat, the world's row of Model.geom_size and opt.ccd_tolerance, the mesh tables.  The only global atomic is
// the atomicOr of an EPA overflow.
#pragma once
#include "convex.hpp"

enum { SC_GEOMDIST = 39, SC_GEOMNORMAL = 40, SC_GEOMFROMTO = 41, SC_OBJ_BODY = 1 };

// floats of LDS per wavefront (a multiple of 4: every wavefront's base stays 16-byte aligned)
__host__ __device__ static inline int sc_lds_words(int iterations) { return (ccd_poly_words(iterations) + 3) & ~3; }

// pair `p` of a sensor whose sides start at geoms id1 / id2 with n2 geoms on side 2: the two geoms in collider order
DEV void sc_pair(const MjhModel& m, int id1, int id2, int n2, int p, int& g1, int& g2, bool& swapped) {
  const int i1 = p / n2;
  g1 = id1 + i1;
  g2 = id2 + (p - i1 * n2);
  const int t1 = m.geom_type[g1], t2 = m.geom_type[g2];
  swapped = t1 > t2 || (t1 == t2 && g1 > g2);
  if (swapped) {
    const int x = g1;
    g1 = g2;
    g2 = x;
  }
}
// margin-0 CcdGeom of geom g in world w; `index`: the mesh vertex cache to start from (-1: none)
DEV CcdGeom sc_geom(const MjhModel& m, const MjhData& d, int w, int g, int index) {
  const int type = m.geom_type[g];
  const float* vert = nullptr;
  const int* graph = nullptr;
  int nvert = 0, meshid = -1;
  if (type == G_MESH) {
    meshid = m.geom_dataid[g];
    vert = m.mesh_vert + 3 * m.mesh_vertadr[meshid];
    nvert = m.mesh_vertnum[meshid];
    if (m.mesh_graphadr[meshid] >= 0) graph = m.mesh_graph + m.mesh_graphadr[meshid];
  }
  return CcdGeom{type, ld3(d.geom_xpos + ((size_t)w * m.ngeom + g) * 3), d.geom_xmat + ((size_t)w * m.ngeom + g) * 9, ld3(BF(m, geom_size, w) + 3 * g),
                 0.0f, vert, nvert, index, meshid, graph, index, nullptr};
}
DEV V3 sc_bcast(V3 a, int src) { return V3{__shfl(a.x, src, 64), __shfl(a.y, src, 64), __shfl(a.z, src, 64)}; }

#ifndef MJH_SC_WAVES  // wavefronts per SIMD the register allocation aims at (developer knob)
#define MJH_SC_WAVES 2
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MJH_SC_WAVES, 8))) k_sensor_collision(MjhModel m, MjhData d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, ncs = m.nsensor_collision;
  const int item = blockIdx.x * (blockDim.x >> 6) + wib;
  if (item >= d.nworld * ncs) return;  // (whole wavefronts leave: nothing below synchronises the workgroup)
  const int w = item / ncs, i = m.sensor_collision_adr[item - w * ncs];
  const int iters = max(m.ccd_iterations, m.epa_iterations);
  float* poly = smem + (size_t)wib * sc_lds_words(iters);

  const int type = m.sensor_type[i], objtype = m.sensor_objtype[i], objid = m.sensor_objid[i], reftype = m.sensor_reftype[i], refid = m.sensor_refid[i];
  const float cutoff = m.sensor_cutoff[i], tol = BF(m, opt_ccd_tolerance, w)[0];
  const int n1 = objtype == SC_OBJ_BODY ? m.body_geomnum[objid] : 1, id1 = objtype == SC_OBJ_BODY ? m.body_geomadr[objid] : objid;
  const int n2 = reftype == SC_OBJ_BODY ? m.body_geomnum[refid] : 1, id2 = reftype == SC_OBJ_BODY ? m.body_geomadr[refid] : refid;
  const int npair = n1 * n2, gjk_it = min(m.ccd_iterations, CCD_MAX_ITER), epa_it = min(m.epa_iterations, CCD_MAX_ITER);

  // the lane's best pair so far: distance, pair index, witnesses on the side-1 / side-2 geom
  float bd = CCD_FLOAT_MAX;
  int bp = 0x7fffffff, ovf = 0;
  V3 bfrom = V3{0.0f, 0.0f, 0.0f}, bto = V3{0.0f, 0.0f, 0.0f};

  for (int p0 = 0; p0 < npair; p0 += 64) {  // (uniform)
    const int p = p0 + lane;
    int st = 0, idx1 = -1, idx2 = -1;
    bool swapped = false;
    float dist = CCD_FLOAT_MAX;
    V3 x1 = V3{0.0f, 0.0f, 0.0f}, x2 = V3{0.0f, 0.0f, 0.0f};
    GjkOut res = {};  // (lanes without a GJK run still take part in the broadcasts below)
    if (p < npair) {
      int g1, g2;
      sc_pair(m, id1, id2, n2, p, g1, g2, swapped);
      CcdGeom a = sc_geom(m, d, w, g1, -1), b = sc_geom(m, d, w, g2, -1);
      if (a.type == G_PLANE) {
        const V3 n = V3{a.rot[2], a.rot[5], a.rot[8]};
        int vid;
        x2 = ccd_support(b, -n, vid);
        dist = dot(n, x2 - a.pos);
        x1 = x2 - dist * n;
      } else {
        st = ccd_gjk_phase<0, true>(tol, cutoff, gjk_it, a, b, dist, x1, x2, res);  // (GUARD: see ccd_gjk)
        idx1 = a.index;
        idx2 = b.index;
      }
    }
    // penetrating pairs: EPA by the whole wavefront, one pair after the other
    unsigned long long em = __ballot(st == 2);
    while (em) {  // (uniform: the ballot is the same in every lane)
      const int src = __ffsll((long long)em) - 1;
      em &= em - 1;
      GjkOut r;
      r.dim = __shfl(res.dim, src, 64);
      r.separated = __shfl((int)res.separated, src, 64) != 0;
      r.dist = __shfl(res.dist, src, 64);
      r.x1 = sc_bcast(res.x1, src);
      r.x2 = sc_bcast(res.x2, src);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r.s[k] = sc_bcast(res.s[k], src);
        r.s1[k] = sc_bcast(res.s1[k], src);
        r.s2[k] = sc_bcast(res.s2[k], src);
        r.i1[k] = __shfl(res.i1[k], src, 64);
        r.i2[k] = __shfl(res.i2[k], src, 64);
      }
      int g1, g2;
      bool sw;
      sc_pair(m, id1, id2, n2, p0 + src, g1, g2, sw);
      const CcdGeom a = sc_geom(m, d, w, g1, __shfl(idx1, src, 64)), b = sc_geom(m, d, w, g2, __shfl(idx2, src, 64));
      float ed = r.dist;
      V3 y1 = r.x1, y2 = r.x2;
      int face, eovf = 0;
      Poly pt;
      const int n = ccd_epa_phase<64>(tol, epa_it, a, b, r, poly, ed, y1, y2, eovf, face, pt, lane, 1);
      ovf |= eovf;
      if (lane == src) {
        dist = n ? ed : CCD_FLOAT_MAX;  // (an EPA that gave up: the pair is left out)
        x1 = y1;
        x2 = y2;
      }
      gsync();  // (the next pair overwrites the polytope)
    }
    if (p < npair && dist < cutoff && dist < bd) {  // (p grows from trip to trip: the earlier pair keeps a tie)
      bd = dist;
      bp = p;
      bfrom = swapped ? x2 : x1;
      bto = swapped ? x1 : x2;
    }
  }
  if (ovf && lane == 0) atomicOr(d.overflow + w, ovf);

  // the minimum over the wavefront; among equal distances the lowest pair index
  const float low = gminf<64>(bd);
  const int win = gmini<64>((bd == low) ? bp : 0x7fffffff);
  const bool found = low < cutoff && win != 0x7fffffff;
  if (found ? bp != win : lane != 0) return;
  float* out = d.sensordata + (size_t)w * m.nsensordata + m.sensor_adr[i];
  if (type == SC_GEOMDIST) {
    float v = found ? low : cutoff;
    if (cutoff > 0.0f) v = fminf(fmaxf(v, -cutoff), cutoff);
    out[0] = v;
  } else if (type == SC_GEOMNORMAL) {
    st3(out, found ? normalize(bto - bfrom) : V3{0.0f, 0.0f, 0.0f});
  } else {
    st3(out, found ? bfrom : V3{0.0f, 0.0f, 0.0f});
    st3(out + 3, found ? bto : V3{0.0f, 0.0f, 0.0f});
  }
}
