// host.hpp -- host-side helpers shared by the translation units of libmjhip.so.
//
// The library is built from several translation units compiled in parallel (the solver kernels are ~70 template
// instantiations and dominate the build time; _abi.UNITS and unity.hip list them):
//   mjhip.hip                          entry points, the step plan, launch sequencing, every non-solver kernel
//   solve_cg32 / solve_cg64 / solve_newton32 / solve_newton64 .hip, their elliptic-cone twins solve_ell_*.hip and the
//   one-row-per-lane solve_ell_newton32_r1.hip       k_solve_plus instantiations (solve_newton32.hip also k_solve_newton, MFMA)
//   solve_cgp.hip / solve_cgw.hip      k_solve_cgp_plus (pooled contact-basis CG) / k_solve_cgw_plus (one world per wavefront)
//   solve_tree_cg / solve_tree_newton / solve_tree_ell_cg / solve_tree_ell_newton .hip   k_solve_tree (per-island solves, nv > 64)
//   pgs_tu.hip (k_solve_pgs, k_solve_pgs_big), solve_big.hip (k_solve_big), render_tu.hip (k_render, k_camera_rays: the cameras),
//   set_const_tu.hip (k_set_const and its entry point mjh_set_const: the derived model constants),
//   sensor_contact_tu.hip (k_sensor_contact: the contact sensors behind the acceleration-stage sensor launch),
//   sensor_collision_tu.hip (k_sensor_collision: the geom distance sensors behind the position-stage sensor launch),
//   transmission_tu.hip (k_transmission, k_fwd_vel_trn: general actuator transmissions, only for models with MjhModel.trn_general),
//   history_tu.hip (k_history_ctrl, k_history_sensor, k_history_read, k_history_init and the entry points mjh_history_read / mjh_history_init:
//   actuator and sensor delays, only for models with MjhModel.nhistory > 0),
//   reset_tu.hip (k_reset and its entry point mjh_reset: reset_data / reset_data_keyframe on the device; never launched by a step),
//   inverse_tu.hip (k_inverse: inverse dynamics, the launch of mjh_inverse / mjh_inv_constraint; never launched by a step),
//   build_id.hip (the source hash, no kernels)
// Device code is header-only and fully inlined per kernel, so no relocatable device code is needed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/mjhip.h"
#include "dev_common.hpp"

int mjh_fail(int code, const char* fmt, const char* a = "");  // records the message for mjh_last_error (mjhip.hip)
#define fail mjh_fail
#define HIPCHK(expr)                                                      \
  do {                                                                    \
    hipError_t e_ = (expr);                                               \
    if (e_ != hipSuccess) return fail(MJH_E_LAUNCH, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

static const int kLdsPerCU = 160 * 1024;

// Developer knobs (tuning / A-B switches; none changes results beyond what the parity tests bound; DESIGN.md lists every one).  The MJH_*
// environment variables are read ONCE, when the library is loaded, into a table (mjhip.hip); nothing on the launch path calls getenv.
// mjh_dev_knob (include/mjhip.h) -- the one documented test hook -- overrides an entry of the table afterwards.  mjh_knob returns nullptr
// when the knob is unset (lock-free while the table is empty); the string it returns is interned and stays valid for the process.
// Two kinds of reader, told apart at the call site:
//   knob_str / knob_flag / knob_int     LIVE: looked up on every call, so mjh_dev_knob takes effect at the next launch
//   KNOB_ONCE_INT / KNOB_ONCE_FLAG      LATCHED: read at first use (one static per call site) and registered, so that a later mjh_dev_knob
//                                       on that name fails with MJH_E_ARG instead of silently doing nothing
const char* mjh_knob(const char* name);
void mjh_knob_latch(const char* name);
static inline const char* knob_str(const char* name) { return mjh_knob(name); }
static inline bool knob_flag(const char* name) { return mjh_knob(name) != nullptr; }
static inline int knob_int(const char* name, int dflt) {
  const char* v = mjh_knob(name);
  return v ? atoi(v) : dflt;
}
#define KNOB_ONCE_INT(name, dflt) ([] { static const int v_ = (mjh_knob_latch(name), knob_int(name, dflt)); return v_; }())
#define KNOB_ONCE_FLAG(name) ([] { static const bool v_ = (mjh_knob_latch(name), knob_flag(name)); return v_; }())

// friction cones are elliptic AND some contact has more than one row (condim 1 everywhere: the cone type is moot)
static inline bool elliptic(const MjhModel* m, const MjhData* d) { return m->cone == CONE_ELLIPTIC && d->nmaxpyramid > 1; }

// ceil(nv / 4) as a compile-time constant: kernels are specialised on it (no padded matrix columns).  f is a generic lambda called with a
// std::integral_constant, e.g. dispatch_nv4_32(nv4, [&](auto NV4) { return launch_cgp_t<NV4()>(m, d, ...); }).  Two ladders, so that a
// launcher instantiates the sizes of its own lane count only: 32 lanes per world (nv <= 32: 1 .. 8) ...
template <typename F>
static inline int dispatch_nv4_32(int nv4, F&& f) {
  switch (nv4) {
    case 0:
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}
// ... and 64 lanes per world (32 < nv <= 64), rounded up to an instantiated size (lanes past nv hold identity rows)
template <typename F>
static inline int dispatch_nv4_64(int nv4, F&& f) {
  if (nv4 <= 9) return f(std::integral_constant<int, 9>{});
  if (nv4 <= 10) return f(std::integral_constant<int, 10>{});
  if (nv4 <= 12) return f(std::integral_constant<int, 12>{});
  if (nv4 <= 14) return f(std::integral_constant<int, 14>{});
  return f(std::integral_constant<int, 16>{});
}

// Profiling builds only (hipcc -DMJH_PHASE_CLOCK; tools/build_variant_fast.py, tools/phase_clock.py --lib ...): read (and optionally reset)
// the per-kernel, per-phase tick sums.  Every unit that marks phases has its own copy of g_phase_ticks (dev_common.hpp) and therefore
// exports its own copy of this reader: MJH_DEFINE_PHASE_TICKS at the end of the unit.
#ifdef MJH_PHASE_CLOCK
#define MJH_DEFINE_PHASE_TICKS                                                                                                      \
  extern "C" __attribute__((visibility("default"))) int mjh_debug_phase_ticks(unsigned long long* out, int reset) {               \
    if (out) HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_ticks), sizeof(unsigned long long) * 64 * 8 * 16));                 \
    if (reset) {                                                                                                                    \
      static unsigned long long zeros[64 * 8 * 16] = {0};                                                                           \
      HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_ticks), zeros, sizeof(zeros)));                                                   \
    }                                                                                                                               \
    return MJH_OK;                                                                                                                  \
  }
#else
#define MJH_DEFINE_PHASE_TICKS
#endif

// pick threads per block in {256,128,64} maximising resident worlds per CU for the given LDS needs (mjhip.hip)
int pick_block(size_t shared_bytes, size_t per_world_bytes, int G, size_t* lds_out, bool prefer_small_arg = false);

// raise the dynamic-LDS cap of a kernel once (never during stream capture: mjh_graph_create warms up first)
template <typename K>
static hipError_t set_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  static std::mutex mu;
  static std::vector<std::pair<const void*, size_t>> done;
  const void* f = reinterpret_cast<const void*>(kernel);
  std::lock_guard<std::mutex> lock(mu);
  for (auto& p : done)
    if (p.first == f && p.second >= bytes) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) done.emplace_back(f, bytes);
  return e;
}

// developer knob MJH_DEBUG_OCC: print the resident workgroups per CU the runtime computes for a launch and the rounds its grid needs
template <typename K>
static void debug_occupancy(const char* name, K kernel, int grid, int threads, size_t lds) {
  if (!KNOB_ONCE_FLAG("MJH_DEBUG_OCC")) return;
  int nb = -1;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, lds);
  fprintf(stderr, "%-22s grid %5d x %3d threads, LDS %6zu B: %2d workgroups per CU = %4.1f wavefronts per SIMD, %.2f rounds on 256 CUs\n", name, grid,
          threads, lds, nb, nb * (threads / 64) / 4.0, nb > 0 ? grid / (256.0 * nb) : 0.0);
}

// solver launches, one translation unit each (nr = rows per lane: 2 / 6 with 32 lanes per world, 1 / 2 / 3 with 64;
// (lo, hi] = row-count range of the worlds this launch solves; fuse_euler: explicit Euler step in the solver epilogue)
int launch_solve_32_cg(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
// one row per lane (worlds of at most 32 rows): solve_ell_newton32_r1.hip
int launch_solve_32_newton_ell_r1(const MjhModel* m, const MjhData* d, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
// CG with one world per wavefront (solver_cgw.hpp): nv <= 32, worlds of at most 64 rows, pyramidal cones
int launch_solve_cgw(const MjhModel* m, const MjhData* d, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
// CG with contact-basis rows in one row pool per workgroup (solver_cgp.hpp): nv <= 32, njmax <= 64, MjhModel.cg_basis; worlds it cannot take
// are flagged solver_niter = -1 for the fallback launch (launch_solve_32_cg_deferred, solve_cg32.hip)
int launch_solve_32_cg_deferred(const MjhModel* m, const MjhData* d, int fuse_euler, hipStream_t s);
int launch_solve_cgp(const MjhModel* m, const MjhData* d, bool with_factor, int fuse_euler, hipStream_t s);
// Newton, nv <= 32, pyramidal cones: the register-resident VALU solver (k_solve_plus) and the MFMA kernel (solver_newton.hpp: njmax <= 64, every
// world of the batch, 32-bit byte offsets; with_factor: the riders as its trailing workgroups).  plan_step (mjhip.hip) decides which one runs.
int launch_solve_32_newton(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
int launch_solve_newton_mfma(const MjhModel* m, const MjhData* d, bool with_factor, int fuse_euler, hipStream_t s);
int launch_solve_64_cg(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
int launch_solve_64_newton(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
// the same with elliptic friction cones (solve_ell_*.hip)
int launch_solve_32_cg_ell(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
int launch_solve_32_newton_ell(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
int launch_solve_64_cg_ell(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
int launch_solve_64_newton_ell(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi);
// per-(world, island) solves for nv > 64 (solve_tree_*.hip)
// (s: the common island class; sr, sr2, sr3: the rare classes -- 8..16 dofs, 16..32 dofs, many rows / 33..64 dofs -- which touch disjoint islands)
int launch_solve_tree_cg(const MjhModel* m, const MjhData* d, hipStream_t s, hipStream_t sr, hipStream_t sr2, hipStream_t sr3);
int launch_solve_tree_newton(const MjhModel* m, const MjhData* d, hipStream_t s, hipStream_t sr, hipStream_t sr2, hipStream_t sr3);
int launch_solve_tree_cg_ell(const MjhModel* m, const MjhData* d, hipStream_t s, hipStream_t sr, hipStream_t sr2, hipStream_t sr3);      // (elliptic cones: solve_tree_ell_*.hip)
int launch_solve_tree_newton_ell(const MjhModel* m, const MjhData* d, hipStream_t s, hipStream_t sr, hipStream_t sr2, hipStream_t sr3);
// PGS: the register / LDS resident sweeps (pgs.hpp: nv <= 64, pyramidal cones) and the generic kernel (pgs_big.hpp: nv > 64 or elliptic cones)
int launch_pgs(const MjhModel* m, const MjhData* d, hipStream_t s);
int launch_pgs_big(const MjhModel* m, const MjhData* d, hipStream_t s);
// generic LDS solver (solver_big.hpp): nv > 64, and the worlds of a small model with more than nefc_lo = 192 rows
int launch_solve_big(const MjhModel* m, const MjhData* d, hipStream_t s, int nefc_lo = -1);
// cameras (render.hpp, render_tu.hip): camera frames + the tile kernel / the pixel rays in the world frame; mjhip.hip checks the arguments
int launch_render(const MjhModel* m, const MjhData* d, const MjhRender* rc, hipStream_t s);
int launch_camera_rays(const MjhModel* m, const MjhData* d, const MjhRender* rc, float* pnt, float* vec, hipStream_t s);
// contact sensors (sensor_contact.hpp, sensor_contact_tu.hip): one wavefront per world, after k_sensor of the acceleration stage
int launch_sensor_contact(const MjhModel* m, const MjhData* d, hipStream_t s);
// geom distance sensors (sensor_collision.hpp, sensor_collision_tu.hip): one wavefront per (world, sensor), after k_sensor of the position stage
int launch_sensor_collision(const MjhModel* m, const MjhData* d, hipStream_t s);
// general actuator transmissions (transmission.hpp, transmission_tu.hip; MjhModel.trn_general): actuator_length / actuator_moment behind the position
// stage, and the velocity stage's instantiation that reads the sparse moment rows (lanes64: the caller's lane choice for the model)
int launch_transmission(const MjhModel* m, const MjhData* d, hipStream_t s);
int launch_vel_trn(const MjhModel* m, const MjhData* d, int first, int last, bool lanes64, hipStream_t s);
// actuator / sensor delays (history.hpp, history_tu.hip; MjhModel.nu_history / nsensor_history_*): Data.ws_ctrl_delayed from the actuators' buffers at
// Data.time (insert: and ctrl into them), and behind the sensor launch of `stage` the delayed read / insert of that stage's sensors with a buffer
int launch_history_ctrl(const MjhModel* m, const MjhData* d, int insert, hipStream_t s);
int launch_history_sensor(const MjhModel* m, const MjhData* d, int stage, int insert, hipStream_t s);
// reset of the worlds `r` selects (reset.hpp, reset_tu.hip): mjh_reset, and the first node of the graph of mjh_graph_create_reset
int launch_reset(const MjhModel* m, const MjhData* d, const MjhReset* r, hipStream_t s);
// inverse dynamics (inverse.hpp, inverse_tu.hip): efc_force / efc_state / qfrc_constraint at the acceleration `qacc` [nworld, nv] and, unless
// qfrc_inverse is null, qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint; G: the caller's lane choice for the model
// (16 / 32 / 64).  launch_inverse_eulerdamp (invdiscrete, Euler): buf = h dof_damping Data.qacc (add == 0), buf += Data.qacc (add == 1)
int launch_inverse(const MjhModel* m, const MjhData* d, const float* qacc, float* qfrc_inverse, int G, hipStream_t s);
int launch_inverse_eulerdamp(const MjhModel* m, const MjhData* d, float* buf, int add, hipStream_t s);
