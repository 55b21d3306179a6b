// linesearch.hpp -- the exact one-dimensional search every CG / Newton kernel runs along its search direction
// (reference solver.py:835-1347 _linesearch_iterative_kernel), and nothing else: the ray evaluators (pyramidal rows, friction-loss
// rows, elliptic contacts), the bracket-end update, ONE driver for everything behind the sums at alpha = 0 (ls_bracket) and
// line_search_rows, the search over rows held in registers.  The kernels keep what is theirs -- where the rows live, how a contact's
// rows meet, how a sum is reduced -- and hand the driver a callable.
//
// The part above the __HIPCC__ guard (P3, bracket_update) is plain C++: tests/ls_bracket_host.cpp compiles it with the host compiler
// and compares bracket_update with the reference's chained update over a grid of derivatives.
#pragma once
#ifdef __HIPCC__
#include "dev_common.hpp"
#define LS_FN DEV
#else
#include <math.h>
#define LS_FN inline
#endif

// (cost - cost(0), grad, hess) of ONE constraint row -- or of a whole ray point once summed -- at step alpha
struct P3 {
  float c, g, h;
};

// Bracket-end update (solver.py:1222-1290).  The reference takes a candidate when its derivative lies strictly between the bracket
// end's derivative and zero -- (x.g < y.g && y.g < 0) || (x.g > y.g && y.g > 0) for end x, candidate y --, for three candidates in turn,
// each test on the end the previous one may have replaced.  The end therefore finishes on the candidate whose derivative is closest
// to zero among those strictly between the ORIGINAL end and zero (the earliest on ties), which needs no chain: three keys, one
// minimum, one select.  Returns whether the end moved (the reference's s1 || s2 || s3).
// Equivalence with the chain (selected candidate and flag), by brute force over 17^4 derivative quadruples with both zeros, denormals,
// +-inf, NaN and magnitudes around 3e38: the two differ ONLY when a candidate's derivative is finite with |g| >= 3.0e38, the key's
// sentinel (794 of the 83521 cases, every one with such a candidate).  tests/test_host.py pins this on a grid below that bound.
// No device intrinsic in here (the sign-bit test is a bit cast): the host compiler compiles it too.
LS_FN float bracket_key(float g, float g0) {  // |g| when g lies strictly between g0 and zero, the sentinel otherwise
  const float mg = fabsf(g);
  const bool same = (__builtin_bit_cast(int, g) ^ __builtin_bit_cast(int, g0)) >= 0;  // equal sign bits
  return (same && mg > 0.0f && mg < fabsf(g0)) ? mg : 3.0e38f;
}
LS_FN bool bracket_update(P3& end, float& end_a, const P3& y1, float a1, const P3& y2, float a2, const P3& y3, float a3) {
  const float k1 = bracket_key(y1.g, end.g), k2 = bracket_key(y2.g, end.g), k3 = bracket_key(y3.g, end.g);
  const float kb = fminf(k1, fminf(k2, k3));
  const bool any = kb < 3.0e38f;
  const bool u1 = k1 == kb, u2 = k2 == kb;
  const float sc = u1 ? y1.c : (u2 ? y2.c : y3.c), sg = u1 ? y1.g : (u2 ? y2.g : y3.g), sh = u1 ? y1.h : (u2 ? y2.h : y3.h);
  const float sa = u1 ? a1 : (u2 ? a2 : a3);
  end.c = any ? sc : end.c;
  end.g = any ? sg : end.g;
  end.h = any ? sh : end.h;
  end_a = any ? sa : end_a;
  return any;
}

#ifdef __HIPCC__
// group sums (solver.hpp): RED selects the broadcast
template <int G, int N, int RED>
DEV void gsum_sel(float (&v)[N]);

// division for step-size candidates and ratios that only steer the search (v_rcp_f32, 1 ulp; an IEEE divide is ~10 ops)
DEV float fast_div(float x, float y) { return x * __builtin_amdgcn_rcpf(y != 0.0f ? y : MJ_MINVAL); }

// ---- one row on the ray (solver.py:518-556 _compute_efc_eval_pt_pyramidal; alpha = 0 variant 620-647) ------------------------------
DEV P3 eval_row(float ja, float jv, float D, float f, int kind, float a) {
  const float jvD = jv * D, hess = jv * jvD, grad0 = jvD * ja;
  const float x = ja + a * jv;
  P3 r = P3{0.0f, 0.0f, 0.0f};
  if (kind == 2) {  // limit / contact: active only when x < 0
    const float quad0 = 0.5f * D * ja * ja;
    const float cost0 = ja < 0.0f ? quad0 : 0.0f;
    if (x < 0.0f) {
      r.c = a * (grad0 + 0.5f * a * hess) + (quad0 - cost0);
      r.g = grad0 + a * hess;
      r.h = hess;
    } else {
      r.c = -cost0;
    }
  } else if (kind == 1) {  // friction loss
    const float rf = safe_div(f, D);
    const float cost0 = (-rf < ja && ja < rf) ? 0.5f * D * ja * ja : (ja <= -rf ? f * (-0.5f * rf - ja) : f * (-0.5f * rf + ja));
    if (-rf < x && x < rf) {
      r.c = 0.5f * D * x * x - cost0;
      r.g = jvD * x;
      r.h = hess;
    } else if (x <= -rf) {
      r.c = f * (-0.5f * rf - x) - cost0;
      r.g = -f * jv;
    } else {
      r.c = f * (-0.5f * rf + x) - cost0;
      r.g = f * jv;
    }
  } else if (kind == 0) {  // equality
    r.c = a * (grad0 + 0.5f * a * hess);
    r.g = grad0 + a * hess;
    r.h = hess;
  }
  return r;
}

// ---- a lane's NR rows on the ray: cost(a) - cost(0) = a (grad0 + a hess / 2) + cact when the row is active at a, cin otherwise;
// equality rows are always active, padding rows have D = jv = 0 ---------------------------------------------------------------------
template <int NR>
struct RowRay {
  float hess[NR], grad0[NR], cact[NR], cin[NR];
};
template <int NR>
DEV void row_ray(RowRay<NR>& e, const float (&rja)[NR], const float (&rjv)[NR], const float (&rD)[NR], const int (&rkind)[NR]) {
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const float jvD = rjv[k] * rD[k], quad0 = 0.5f * rD[k] * rja[k] * rja[k];
    const float cost0 = (rkind[k] == 0 || rja[k] < 0.0f) ? quad0 : 0.0f;
    e.hess[k] = rjv[k] * jvD;
    e.grad0[k] = jvD * rja[k];
    e.cact[k] = quad0 - cost0;
    e.cin[k] = -cost0;
  }
}
// the lane's sum at step a, added to s.  Equality / limit / contact rows only: branch-free
template <int NR>
DEV void row_ray_eval(P3& s, const RowRay<NR>& e, const float (&rja)[NR], const float (&rjv)[NR], const int (&rkind)[NR], float a) {
  const float ha = 0.5f * a;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const bool act = rkind[k] == 0 || (rja[k] + a * rjv[k] < 0.0f);
    s.c += act ? a * (e.grad0[k] + ha * e.hess[k]) + e.cact[k] : e.cin[k];
    s.g += act ? e.grad0[k] + a * e.hess[k] : 0.0f;
    s.h += act ? e.hess[k] : 0.0f;
  }
}
// the same with friction-loss rows present (three-zone cost, rare); floss_lane[G * k]: frictionloss of the lane's row k
template <int NR, int G>
DEV void row_ray_eval_fl(P3& s, const float (&rja)[NR], const float (&rjv)[NR], const float (&rD)[NR], const int (&rkind)[NR], const float* floss_lane,
                         float a) {
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const P3 t = eval_row(rja[k], rjv[k], rD[k], rkind[k] == 1 ? floss_lane[G * k] : 0.0f, rkind[k], a);
    s.c += t.c;
    s.g += t.g;
    s.h += t.h;
  }
}

// ---- elliptic friction cones (solver.py:272-421) -------------------------------------------------------------
// One contact = `dim` consecutive rows (normal, then friction directions).  In the reference's scaled coordinates
// N = mu * Jaref_0 and T = |(fri_j * Jaref_j)_j>=1| the contact is SATISFIED for N >= mu T (top zone), QUADRATIC for
// mu N + T <= 0 (bottom zone, every row an independent quadratic) and in the CONE (middle) zone otherwise, where its cost is
// dm/2 (N - mu T)^2, dm = D_0 / (mu^2 (1 + mu^2)), mu = friction_0 / sqrt(impratio).
DEV int ell_zone(float mu, float N, float T) {
  if (N >= mu * T || (T <= 0.0f && N >= 0.0f)) return ST_SATISFIED;
  if (mu * N + T <= 0.0f || (T <= 0.0f && N < 0.0f)) return ST_QUADRATIC;
  return ST_CONE;
}
// constants of one contact on the search ray, held by the lane that owns the contact's first row
struct EllRay {
  float mu, dm, q0, q1, q2, u0, v0, uu, uv, vv;  // q = sum_j (D ja^2 / 2, D jv ja, D jv^2 / 2); u = scaled Jaref, v = scaled jv
  float cost0, T0, r0;                            // the reference point alpha = 0 (_eval_elliptic_reference solver.py:275-298)
  int state0;
};
DEV void ell_ray_reference(EllRay& e) {
  e.T0 = 0.0f;
  e.r0 = 0.0f;
  if (e.uu <= 0.0f) {
    e.state0 = e.u0 < 0.0f ? ST_QUADRATIC : ST_SATISFIED;
    e.cost0 = e.u0 < 0.0f ? e.q0 : 0.0f;
    return;
  }
  e.T0 = sqrtf(e.uu);
  if (e.u0 >= e.mu * e.T0) {
    e.state0 = ST_SATISFIED;
    e.cost0 = 0.0f;
  } else if (e.mu * e.u0 + e.T0 <= 0.0f) {
    e.state0 = ST_QUADRATIC;
    e.cost0 = e.q0;
  } else {
    e.r0 = e.u0 - e.mu * e.T0;
    e.state0 = ST_CONE;
    e.cost0 = 0.5f * e.dm * e.r0 * e.r0;
  }
}
// (cost(alpha) - cost(0), d/dalpha, d2/dalpha2) of one elliptic contact: the shifted forms of the reference
// (_eval_elliptic_shifted solver.py:343-403), which difference against the reference point analytically -- in float32
// the plain difference of two costs loses the line search's whole signal near convergence
DEV P3 ell_eval(const EllRay& e, float a) {
  const float N = e.u0 + a * e.v0;
  const float Td = a * (2.0f * e.uv + a * e.vv), Tsqr = e.uu + Td;
  const float aq2 = a * e.q2;
  bool quadz = false, conez = false;
  float T = 0.0f;
  if (Tsqr <= 0.0f) {
    quadz = N < 0.0f;
  } else {
    T = sqrtf(Tsqr);
    if (N >= e.mu * T) {
    } else if (e.mu * N + T <= 0.0f) quadz = true;
    else conez = true;
  }
  if (quadz) {  // _eval_elliptic_quadratic_shifted solver.py:318-340
    float cost = a * (aq2 + e.q1);
    if (e.state0 == ST_CONE) {
      const float b0 = e.mu * e.u0 + e.T0;
      cost += 0.5f * e.dm * b0 * b0;
    } else if (e.state0 == ST_SATISFIED) {
      cost = 0.5f * e.dm * (1.0f + e.mu * e.mu) * (N * N + fmaxf(Tsqr, 0.0f));
    }
    return P3{cost, 2.0f * aq2 + e.q1, 2.0f * e.q2};
  }
  if (conez) {
    const float Tinv = 1.0f / T;
    const float T1 = (e.uv + a * e.vv) * Tinv, T2 = (e.vv - T1 * T1) * Tinv;
    const float r = N - e.mu * T, r1 = e.v0 - e.mu * T1;
    float cost;
    if (e.state0 == ST_CONE) {  // rationalised T - T0
      const float Tdelta = Td / (T + e.T0), rdelta = a * e.v0 - e.mu * Tdelta;
      cost = 0.5f * e.dm * rdelta * (2.0f * e.r0 + rdelta);
    } else if (e.state0 == ST_QUADRATIC) {
      const float b = e.mu * N + T;
      cost = a * (aq2 + e.q1) - 0.5f * e.dm * b * b;
    } else {
      cost = 0.5f * e.dm * r * r;
    }
    return P3{cost, e.dm * r * r1, e.dm * (r1 * r1 - e.mu * r * T2)};
  }
  return P3{-e.cost0, 0.0f, 0.0f};
}

// ---- the driver: everything behind the sums at alpha = 0 (solver.py:1100-1347) -----------------------------------------------------
// p0: the total at alpha = 0 (c = 0).  totals(a, t): t[i] = the finished total at step a[i] for i < N, N = 1 or 3 (a, t: arrays of N) --
// summed over the lane group, the Gauss (smooth) quadratic added.  Newton point, early exit, bracket [lo, hi] around the zero of the
// derivative, then per round the Newton steps from both ends and the midpoint, bracket_update on each end, until an end's derivative
// is inside gtol or no end moved; alpha = 0 when nothing improved the cost.
//
// The callers differ on purpose in two places, and aligning them would change results:
//   * the float32 noise floor on gtol (MJH_LS_NOISE_ULPS) is applied by line_search_rows only; the elliptic branch of solve_body
//     (solver.hpp) and solve_big_body (solver_big.hpp) pass the reference's gtol as it is;
//   * friction-loss rows (has_fl) select the three-zone evaluator at compile time in line_search_rows (HAS_FL) and at run time in
//     those two.
struct LsStep {
  float alpha, improvement;
  bool converged;
};
template <class Totals>
DEV LsStep ls_bracket(const P3& p0, float gtol, int ls_iterations, Totals&& totals, int* iters_out = nullptr) {
  const float a1[1] = {-fast_div(p0.g, p0.h)};
  P3 t1[1];
  totals(a1, t1);
  const float lo_alpha_in = a1[0];
  const P3 lo_in = t1[0];
  float alpha = 0.0f, improvement = 0.0f;
  bool ls_converged = fabsf(lo_in.g) < gtol && lo_in.c < 0.0f;
  if (ls_converged) {
    alpha = lo_alpha_in;
    improvement = -lo_in.c;
  } else {
    const bool lo_less = lo_in.g < p0.g;
    P3 lo = lo_less ? lo_in : p0, hi = lo_less ? p0 : lo_in;
    float lo_alpha = lo_less ? lo_alpha_in : 0.0f, hi_alpha = lo_less ? 0.0f : lo_alpha_in;
    for (int it = 0; it < ls_iterations; ++it) {
      if (iters_out) ++*iters_out;
      const float a_lo = lo_alpha - fast_div(lo.g, lo.h), a_hi = hi_alpha - fast_div(hi.g, hi.h);
      const float a_mid = 0.5f * (lo_alpha + hi_alpha);
      const float a3[3] = {a_lo, a_hi, a_mid};
      P3 t3[3];
      totals(a3, t3);
      const P3 lo_next = t3[0], hi_next = t3[1], mid = t3[2];
      // (selects, not branches: the updates are wave-divergent between the two worlds of a wavefront)
      const bool swap_lo = bracket_update(lo, lo_alpha, lo_next, a_lo, mid, a_mid, hi_next, a_hi);
      const bool swap_hi = bracket_update(hi, hi_alpha, hi_next, a_hi, mid, a_mid, lo_next, a_lo);
      const bool ls_done = (!swap_lo && !swap_hi) || (lo.c < 0.0f && lo.g < 0.0f && lo.g > -gtol) || (hi.c < 0.0f && hi.g > 0.0f && hi.g < gtol);
      const bool improved = lo.c < 0.0f || hi.c < 0.0f;
      const bool lo_better = lo.c < hi.c;
      alpha = improved ? (lo_better ? lo_alpha : hi_alpha) : alpha;
      improvement = improved ? -(lo_better ? lo.c : hi.c) : improvement;
      if (ls_done) {
        ls_converged = true;
        break;
      }
    }
  }
  return LsStep{alpha, improvement, ls_converged};
}

#ifndef MJH_LS_NOISE_ULPS
#define MJH_LS_NOISE_ULPS 4
#endif
// ---- the line search over rows held in registers; every sum of an evaluation round is reduced together (gsum_sel<G, 3 or 9, RED>)
// HAS_FL: friction-loss rows present (three-zone cost, rare): a compile-time switch, the common instantiation is branch-free
template <int NR, int G, bool HAS_FL, int RED = 0>
DEV void line_search_rows(const float (&rja)[NR], const float (&rjv)[NR], const float (&rD)[NR], const int (&rkind)[NR],
                          const float* floss_lane, float gauss1_lane, float gauss2_lane, float gauss1_abs_lane, float gtol_in, int ls_iterations,
                          float& alpha_out, float& improvement_out, bool& converged_out, int* iters_out = nullptr) {
  // (the constants and the evaluator of RowRay / row_ray_eval, spelled out on plain arrays: routed through those functions the compiler
  // contracts a (grad0 + a hess / 2) + cact differently in the pyramidal kernels and their results move in the last bits -- measured on
  // cgw, pair, cg64, newton64 and the MFMA Newton kernel --, and a refactor may not move them)
  float ehess[NR], egrad0[NR], ecact[NR], ecin[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const float jvD = rjv[k] * rD[k], quad0 = 0.5f * rD[k] * rja[k] * rja[k];
    const float cost0 = (rkind[k] == 0 || rja[k] < 0.0f) ? quad0 : 0.0f;
    ehess[k] = rjv[k] * jvD;
    egrad0[k] = jvD * rja[k];
    ecact[k] = quad0 - cost0;
    ecin[k] = -cost0;
  }
  auto eval = [&](float a) __attribute__((always_inline)) {
    P3 s = P3{0.0f, 0.0f, 0.0f};
    if (!HAS_FL) {
      const float ha = 0.5f * a;
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        const bool act = rkind[k] == 0 || (rja[k] + a * rjv[k] < 0.0f);
        s.c += act ? a * (egrad0[k] + ha * ehess[k]) + ecact[k] : ecin[k];
        s.g += act ? egrad0[k] + a * ehess[k] : 0.0f;
        s.h += act ? ehess[k] : 0.0f;
      }
    } else {
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        const P3 t = eval_row(rja[k], rjv[k], rD[k], rkind[k] == 1 ? floss_lane[G * k] : 0.0f, rkind[k], a);
        s.c += t.c;
        s.g += t.g;
        s.h += t.h;
      }
    }
    return s;
  };
  const P3 e = eval(0.0f);
#if MJH_LS_NOISE_ULPS > 0
  // float32: the ray derivative is a sum of ~nefc + nv terms that mostly cancel at the minimum, so it carries rounding noise of
  // about eps * sum |term|.  A derivative inside that noise is zero as far as float32 can tell: bracketing on (the reference's
  // tolerance floor of 1e-6 is an absolute number chosen for float64) only chases noise -- measured 2.5 bracketing iterations
  // per call against 0.75 for the float64 oracle, with no effect on the iterates.
  // (round 3: the three sums of the Gauss quadratic -- search . (Ma - qfrc_smooth), search . M search / 2 and the absolute terms of the
  // first -- ride in the same reduction: one dependent DPP chain per solver iteration less)
  float eabs = 0.0f;
#pragma unroll
  for (int k = 0; k < NR; ++k) eabs += fabsf(egrad0[k]);
  float r2[6] = {e.g, e.h, eabs, gauss1_lane, gauss2_lane, gauss1_abs_lane};
  gsum_sel<G, 6, RED>(r2);
  const float gauss1 = r2[3], gauss2 = r2[4];
  const float gtol = fmaxf(gtol_in, (MJH_LS_NOISE_ULPS * 5.96e-8f) * (r2[5] + r2[2]));
#else
  float r2[4] = {e.g, e.h, gauss1_lane, gauss2_lane};
  gsum_sel<G, 4, RED>(r2);
  const float gauss1 = r2[2], gauss2 = r2[3];
  const float gtol = gtol_in;
#endif
  const P3 p0 = P3{0.0f, gauss1 + r2[0], 2.0f * gauss2 + r2[1]};
  // group sums + the Gauss (smooth) quadratic; the sums of the one or three points of a round are reduced together
  auto finish = [&](float c, float g, float h, float a) __attribute__((always_inline)) {
    return P3{a * a * gauss2 + a * gauss1 + c, 2.0f * a * gauss2 + gauss1 + g, 2.0f * gauss2 + h};
  };
  auto totals = [&](const auto& a, auto& t) __attribute__((always_inline)) {
    if constexpr (sizeof(a) == sizeof(float)) {
      const P3 el = eval(a[0]);
      float r3[3] = {el.c, el.g, el.h};
      gsum_sel<G, 3, RED>(r3);
      t[0] = finish(r3[0], r3[1], r3[2], a[0]);
    } else {
      const P3 e1 = eval(a[0]), e2 = eval(a[1]), e3 = eval(a[2]);
      float r9[9] = {e1.c, e1.g, e1.h, e2.c, e2.g, e2.h, e3.c, e3.g, e3.h};
      gsum_sel<G, 9, RED>(r9);
      t[0] = finish(r9[0], r9[1], r9[2], a[0]);
      t[1] = finish(r9[3], r9[4], r9[5], a[1]);
      t[2] = finish(r9[6], r9[7], r9[8], a[2]);
    }
  };
  const LsStep s = ls_bracket(p0, gtol, ls_iterations, totals, iters_out);
  alpha_out = s.alpha;
  improvement_out = s.improvement;
  converged_out = s.converged;
}
#endif  // __HIPCC__
