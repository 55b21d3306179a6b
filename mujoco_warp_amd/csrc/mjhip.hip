// mjhip.hip -- extern "C" entry points of libmjhip.so (see include/mjhip.h) and launch sequencing.
//
// One `step` = 3-4 composite launches on the caller's stream (reference: ~90 fixed launches + ~12 per solver
// iteration, forward.py:1341-1380):
//   k_fwd_pos_plus (kinematics+com_pos+crb, solver schedule) -> k_mid ({collision -> make_constraint} and fwd_vel
//   workgroups) -> k_solve_plus / k_solve_pgs (the whole solve, riders) -> k_integrate_plus (integrator, riders);
// the stage API launches the same bodies as plain kernels.  See "composite launches" below and DESIGN.md section 3.
// Nothing here allocates or synchronises (hipGraph-capturable); workspace lives in MjhData.
#include "host.hpp"

#include "contact_rec.hpp"
// developer knobs of the k_mid occupancy experiment (round 5, LAB_NOTES.md R5): contacts per staging window, wavefronts per SIMD of the light k_mid
#ifdef MJH_CON_WINDOW
#undef CON_WINDOW
#define CON_WINDOW MJH_CON_WINDOW
#endif
#ifndef MJH_MID_WAVES
#define MJH_MID_WAVES 4
#endif

#include "collide.hpp"
#include "constraint.hpp"
#include "dev_common.hpp"
#include "integrate.hpp"
#include "implicit.hpp"
#include "sensor.hpp"
#include "sleep.hpp"
#include "smooth.hpp"
#include "support.hpp"

static thread_local char g_err[512] = "";
int mjh_fail(int code, const char* fmt, const char* a) {
  snprintf(g_err, sizeof(g_err), fmt, a);
  return code;
}

// ---- developer knobs: a table filled ONCE from the environment when the library is loaded; mjh_dev_knob overrides entries (host.hpp) ----
#include <atomic>
#include <map>
#include <set>
#include <string>
extern char** environ;
namespace {
struct KnobTable {
  std::mutex mu;
  std::set<std::string> pool;                    // every value ever set, interned: what mjh_knob hands out is never freed
  std::map<std::string, const std::string*> kv;  // name -> its value in `pool`
  std::set<std::string> latched;                 // names a KNOB_ONCE_* reader has consumed (mjh_dev_knob refuses them)
  std::atomic<int> n{0};
  void set(const std::string& name, const char* value) { kv[name] = &*pool.insert(value).first; }
  KnobTable() {
    for (char** e = environ; e && *e; ++e) {
      if (strncmp(*e, "MJH_", 4) != 0 || strncmp(*e, "MJH_LIB=", 8) == 0) continue;  // (MJH_LIB: the Python loader's variable, not a knob)
      const char* eq = strchr(*e, '=');
      if (eq) set(std::string(*e, eq - *e), eq + 1);
    }
    n.store((int)kv.size());
  }
};
KnobTable& knobs() {
  static KnobTable t;  // (constructed at first use or by the initialiser below, whichever comes first: before any launch)
  return t;
}
struct KnobInit {
  KnobInit() { knobs(); }
} g_knob_init;  // library load
}  // namespace
const char* mjh_knob(const char* name) {
  KnobTable& t = knobs();
  if (t.n.load(std::memory_order_acquire) == 0) return nullptr;  // the product path: no knob set, no lock, no lookup
  std::lock_guard<std::mutex> lock(t.mu);
  auto it = t.kv.find(name);
  return it == t.kv.end() ? nullptr : it->second->c_str();
}
void mjh_knob_latch(const char* name) {
  KnobTable& t = knobs();
  std::lock_guard<std::mutex> lock(t.mu);
  t.latched.insert(name);
}
#define TRY(x)               \
  do {                       \
    int rc_ = (x);           \
    if (rc_ != MJH_OK) return rc_; \
  } while (0)

// ---- the call context: what one entry-point call hands down to every launch it makes ---------------------------------------------------
// optional per-kernel event instrumentation used by mjh_timed_steps
struct Instr {
  std::vector<hipEvent_t> ev;  // pairs
  std::vector<int> cls;
  bool plain = false;  // one plain kernel per stage instead of the fused launches
  hipError_t err = hipSuccess;  // first failing hipEvent* call of a Scope (reported by mjh_timed_steps)
};
// An entry point (mjh_stage, mjh_graph_create, mjh_timed_steps, mjh_ctrl_noise) makes one on its stack and passes it down by reference; nothing
// per-call lives in a global.  Launchers that need only a stream take run.s.
struct Run {
  hipStream_t s;
  // the sensors and actuators with a history buffer (csrc/history.hpp) store their fresh values -- every evaluation but the RK4 sub-evaluations
  bool hist_insert = true;
  Instr* instr = nullptr;  // per-kernel event pairs are on: one stream, no side launches, every Scope records
  // The benchmark loop's control noise (mjh_timed_steps), pending until something applies it.  ONE rule: the fused position launch carries it
  // (launch_pos_plus_g); where there is none, the driver launches it (apply_noise) in front of the first launch that reads ctrl.
  NoiseArgs noise = {0, 0, 0.0f, 0.0f, nullptr, 0};
  explicit Run(void* stream) : s((hipStream_t)stream) {}
};
struct Scope {
  Instr* in;
  hipStream_t s;
  int cls;
  hipEvent_t a, b;
  void note(hipError_t e) {
    if (e != hipSuccess && in->err == hipSuccess) in->err = e;
  }
  Scope(const Run& run, int c) : in(run.instr), s(run.s), cls(c), a(nullptr), b(nullptr) {
    if (in) {
      note(hipEventCreate(&a));
      note(hipEventCreate(&b));
      if (a && b) note(hipEventRecord(a, s));
    }
  }
  ~Scope() {
    if (in && a && b) {
      note(hipEventRecord(b, s));
      in->ev.push_back(a);
      in->ev.push_back(b);
      in->cls.push_back(cls);
    } else {
      if (a) hipEventDestroy(a);
      if (b) hipEventDestroy(b);
    }
  }
};
enum { K_NOISE = 0, K_POS = 1, K_COLLISION = 2, K_CONSTRAINT = 3, K_VEL = 4, K_SOLVE = 5, K_INTEGRATE = 6, K_OTHER = 7, K_MID = 8 };

// pick threads per block in {256,128,64} maximising resident worlds per CU for the given LDS needs
int pick_block(size_t shared_bytes, size_t per_world_bytes, int G, size_t* lds_out, bool prefer_small_arg) {
  const int small_env = KNOB_ONCE_INT("MJH_SMALL_BLOCKS", -1);  // developer knob
  const bool prefer_small = small_env >= 0 ? (small_env != 0) : prefer_small_arg;
  int best = 0, best_worlds = -1;
  // ties go to the first candidate: large blocks amortise the block-shared tables, small blocks retire as soon as
  // their own worlds converge (k_solve: per-world work varies by an order of magnitude)
  const int order_big[3] = {256, 128, 64}, order_small[3] = {64, 128, 256};
  for (int oi = 0; oi < 3; ++oi) {
    const int threads = prefer_small ? order_small[oi] : order_big[oi];
    const int wpb = threads / G;
    if (wpb < 1) continue;
    const size_t lds = shared_bytes + per_world_bytes * wpb;
    if (lds > (size_t)kLdsPerCU) continue;
    int blocks = (int)(kLdsPerCU / lds);
    const int wave_cap = 32 / (threads / 64);
    if (blocks > wave_cap) blocks = wave_cap;
    const int worlds = blocks * wpb;
    if (worlds > best_worlds) {
      best_worlds = worlds;
      best = threads;
    }
  }
  if (best) *lds_out = shared_bytes + per_world_bytes * (best / G);
  return best;
}
// The launch of a plain "one lane group per world" kernel: the workgroup pick_block chooses for its LDS needs (shared_bytes per workgroup +
// per_world_bytes per world), threads / G worlds per workgroup.  unfit: the message when not even the smallest workgroup fits in LDS.
template <typename K, typename... Args>
static int launch_per_world(K kernel, const char* unfit, int G, size_t shared_bytes, size_t per_world_bytes, int nworld, hipStream_t s, const Args&... args) {
  size_t lds;
  const int threads = pick_block(shared_bytes, per_world_bytes, G, &lds);
  if (!threads) return fail(MJH_E_UNSUPPORTED, unfit);
  HIPCHK(set_lds(kernel, lds));
  const int wpb = threads / G;
  hipLaunchKernelGGL(kernel, dim3((nworld + wpb - 1) / wpb), dim3(threads), lds, s, args...);
  return MJH_OK;
}

// Lanes per world of every kernel but the solvers (which choose their own): 32 -- two worlds per wavefront -- for models of at most 32 dofs
// and bodies, 64 beyond (round 3): these kernels are chains of dependent steps whose loops stride over dofs / bodies / geoms by the
// group size, so a model that needs two trips with 32 lanes needs one with 64 (three humanoids, nv 81: k_mid 690 -> 518 us, step + 22 %).
static inline bool lanes64(const MjhModel* m) {
  const int force = KNOB_ONCE_INT("MJH_LANES", 0);  // developer knob: 32 / 64
  if (force) return force == 64;
  // (models with GJK / EPA pairs stay at 32: Data.ws_ccd holds one polytope workspace per lane of a 32-lane group)
  return (m->nv > 32 || m->nbody > 32) && !m->heavy_colliders;
}
// 16 lanes per world -- four worlds per wavefront -- in k_mid for small models (at most 16 dofs and bodies, light colliders; round 3): half the
// wavefronts for the same worlds and still one trip per loop.  Same-box A/B: Panda 8192 worlds k_mid 62.0 -> 49.5 us, step 180 -> 164.6 us
// (- 8.7 %).  Not for larger models (forced on the humanoid, 27 dofs on 17 bodies: k_mid 84 -> 101 us -- every loop needs two trips) and not
// for k_fwd_pos (Panda 48.0 vs 49.1 us: its chain is the tree depth whatever the lane count): both experiments lost, their knobs are retired.
static inline bool lanes16(const MjhModel* m) {
  const int force = KNOB_ONCE_INT("MJH_LANES", 0);  // developer knob: 32 / 64 forbid it; 16 is the default's choice, never beyond 16 dofs / bodies
  if (force && force != 16) return false;
  return m->nv <= 16 && m->nbody <= 16 && !m->heavy_colliders;
}
// (k_fwd_pos: its loops run over bodies -- the G1, 35 dofs on 30 bodies, is 4 us slower with 64 lanes; three humanoids, 52 bodies, 25 us faster)

template <int G>
static int launch_pos_g(const MjhModel* m, const MjhData* d, int first, int last, hipStream_t s) {
  const PosLayout lay = pos_layout(m->nq, m->nv, m->nbody, m->njnt, m->nC, last >= POS_FACTOR);
  return launch_per_world(k_fwd_pos<G>, "k_fwd_pos: model does not fit in LDS", G, sizeof(int) * pos_shared_words(m->nv, m->nC, m->nbody, m->njnt, m->nbodylevel, m->ngeom, m->nsite),
                          sizeof(float) * lay.total, d->nworld, s, *m, *d, first, last);
}
static int launch_pos(const MjhModel* m, const MjhData* d, int first, int last, hipStream_t s) { return lanes64(m) && m->nbody > 32 ? launch_pos_g<64>(m, d, first, last, s) : launch_pos_g<32>(m, d, first, last, s); }
template <int G>
static int launch_vel_g(const MjhModel* m, const MjhData* d, int first, int last, hipStream_t s) {
  const VelLayout lay = vel_layout(m->nq, m->nv, m->nbody, m->nC, m->nu);
  return launch_per_world(k_fwd_vel<G>, "k_fwd_vel: model does not fit in LDS", G, sizeof(int) * mstruct_ints(m->nv, m->nC), sizeof(float) * lay.total, d->nworld, s, *m, *d, first, last);
}
// (general transmissions, MjhModel.trn_general: the velocity stage's TRN instantiation and k_transmission behind the position stage, both in
// transmission_tu.hip -- every other model launches what it launched before)
static int launch_vel(const MjhModel* m, const MjhData* d, int first, int last, hipStream_t s) {
  if (m->trn_general) return launch_vel_trn(m, d, first, last, lanes64(m), s);
  return lanes64(m) ? launch_vel_g<64>(m, d, first, last, s) : launch_vel_g<32>(m, d, first, last, s);
}
static int launch_trn(const MjhModel* m, const MjhData* d, hipStream_t s) { return m->trn_general ? launch_transmission(m, d, s) : MJH_OK; }
// public L'DL factor (qLD, qLDiagInv) and, on request, qacc_smooth: outputs nobody inside the step waits for
// (32 lanes per world here and in the other kernels that chain over the sparse factor -- k_integrate, k_integrate_plus, k_solve_m, and
// k_publish_contacts with them: more lanes per world only halve the worlds per wavefront)
static int launch_factor_smooth(const MjhModel* m, const MjhData* d, int write_qacc, hipStream_t s) {
  const FacLayout lay = fac_layout(m->nv, m->nC);
  return launch_per_world(k_factor_smooth<32>, "k_factor_smooth: model does not fit in LDS", 32, sizeof(int) * mstruct_ints(m->nv, m->nC), sizeof(float) * lay.total, d->nworld, s, *m, *d, write_qacc);
}
// the three launches of the convex narrowphase in front of a contact kernel (models with GJK pairs; csrc/convex.hpp header)
template <int G>
static int launch_ccd_pre(const MjhModel* m, const MjhData* d, hipStream_t s) {
  const int it = std::max(m->ccd_iterations, m->epa_iterations);
  const CcdLayout CL = ccd_layout(d->nworld, it, m->nhfield, m->npolygonmax, m->nmeshdegmax, collide_ccap(m->npair, d->concap), d->nccdhand, m->npair);
  hipLaunchKernelGGL(k_ccd_reset, dim3(std::max((m->npair + 63) / 64, 1)), dim3(64), 0, s, *m, *d);  // counters, convex-pair mask (a kernel, not a memset node: replayed inside hipGraphs)
  if (m->broadphase == 0 && m->npair > 0) {  // NXN: the broadphase filters of every world as their own launch (a workgroup per world), results as bit masks
    const size_t lds_mask = sizeof(float) * (size_t)bmask_layout(m->ngeom, m->npair, m->broadphase_filter, m->ncullgeom, m->ncullgroup, m->ncullpair).total;
    if (lds_mask > 160 * 1024 || m->ngeom > 65535) return fail(MJH_E_UNSUPPORTED, "k_broad_mask: the geom tables do not fit in LDS");
    if (m->ncullpair <= 0 || !m->cull_pair || !m->cull_list) return fail(MJH_E_ARG, "k_broad_mask: Model.cull_pair / cull_list missing (io.py cull_tables; a binding must build them, INTEGRATION.md ABI v42)");
    HIPCHK(set_lds(k_broad_mask, lds_mask));
    hipLaunchKernelGGL(k_broad_mask, dim3((unsigned)std::min(d->nworld, 8192)), dim3(256), lds_mask, s, *m, *d);
  }
  if (m->broadphase != 0 || m->npair == 0) {  // sweep-and-prune: the broadphase of a world by its lane group (k_broad_mask publishes the NXN list itself)
    TRY(launch_per_world(k_ccd_broad<G>, "k_ccd_broad: pair list does not fit in LDS", G, sizeof(float) * 9 * m->ngeom,  // (the staged model tables)
                         sizeof(float) * broad_lds_words(m->ngeom, m->npair, d->concap, m->broadphase), d->nworld, s, *m, *d));
  }
  // (grids sized for the device -- 256 CUs x 8 workgroups --, not for the lists' capacities: the kernels walk their lists with the grid's stride)
  {
    // lanes per pair by the length of the list (read on the device): one lane per pair needs >= 2 wavefronts per SIMD to hide its chains of
    // dependent table loads; shorter lists give a pair 8 or 32 lanes (MJH_GJK_LANES: developer knob, forces one instantiation)
    const int force = KNOB_ONCE_INT("MJH_GJK_LANES", 0);
    const int t8_env = KNOB_ONCE_INT("MJH_GJK_T8", 16384), t1_env = KNOB_ONCE_INT("MJH_GJK_T1", 131072);  // developer knobs
    const int all = 0x7fffffff, t8 = force ? (force == 32 ? all : 0) : t8_env, t1 = force ? (force == 1 ? 0 : all) : std::max(t1_env, t8_env);
    const long long cap = (long long)d->nworld * CL.ccap;  // work items at most
    const int grid1 = (int)std::min<long long>((cap + 255) / 256, 2048);
    hipLaunchKernelGGL(k_ccd_gjk<32>, dim3((unsigned)std::min<long long>((cap + 7) / 8, 4096)), dim3(256), 0, s, *m, *d, 0, t8);
    hipLaunchKernelGGL(k_ccd_gjk<8>, dim3((unsigned)std::min<long long>((cap + 31) / 32, 4096)), dim3(256), 0, s, *m, *d, t8, t1);
    hipLaunchKernelGGL(k_ccd_gjk<1>, dim3(grid1), dim3(256), 0, s, *m, *d, t1, all);
  }
  // lane groups per workgroup: a group's LDS (polytope + the multi-contact polygon buffers: 11.7 KB on the ALOHA scene) decides how many are
  // resident on a CU -- eight groups in one 256-thread workgroup leave room for ONE workgroup there; smaller workgroups pack the LDS
  const int epa_threads = KNOB_ONCE_INT("MJH_EPA_THREADS", 256);  // developer knob
  const size_t group_bytes = sizeof(float) * (size_t)ccd_coop_words(it, m->npolygonmax, m->nmeshdegmax);
  int gpb = std::max(epa_threads / G, 1);
  while (gpb > 1 && group_bytes * gpb > (size_t)kLdsPerCU) gpb >>= 1;  // (a mesh vertex of very high degree: long feature lists per group)
  if (group_bytes > (size_t)kLdsPerCU) return fail(MJH_E_UNSUPPORTED, "k_ccd_epa: a lane group's polytope and multi-contact lists do not fit in LDS (mesh vertex degree / polygon size too large)");
  const size_t lds_epa = group_bytes * gpb;
  HIPCHK(set_lds((k_ccd_epa<G>), lds_epa));
  hipLaunchKernelGGL((k_ccd_epa<G>), dim3(std::min((CL.handcap + gpb - 1) / gpb, 16384 / 8)), dim3(G * gpb), lds_epa, s, *m, *d);
  return MJH_OK;
}
template <int G>
static int launch_collision_g(const MjhModel* m, const MjhData* d, hipStream_t s) {
  if (m->heavy_colliders && d->ws_ccd) TRY(launch_ccd_pre<G>(m, d, s));
  const size_t per_world = sizeof(float) * collide_lds_words(m->ngeom, m->npair, d->concap, m->heavy_colliders ? m->broadphase : 0, m->heavy_colliders && d->ws_ccd != nullptr);
  auto go = [&](auto kernel) { return launch_per_world(kernel, "k_collision: pair list does not fit in LDS", G, 0, per_world, d->nworld, s, *m, *d); };
  if (!m->heavy_colliders) return go(k_collision<G, false>);
  return m->nhfield > 0 ? go(k_collision<G, true, true>) : go(k_collision<G, true, false>);  // (without the height-field colliders: the registers of their per-lane GJK / EPA)
}
static int launch_collision(const MjhModel* m, const MjhData* d, hipStream_t s) { return lanes64(m) ? launch_collision_g<64>(m, d, s) : launch_collision_g<32>(m, d, s); }
// compact public contact arrays, contact.efc_address and efc.id of contact rows from the per-world records
static int launch_publish(const MjhModel* m, const MjhData* d, hipStream_t s) {
  hipLaunchKernelGGL(k_publish_contacts<32>, dim3((d->nworld + 256 / 32 - 1) / (256 / 32)), dim3(256), 0, s, *d, 1, m->nexplicit ? m->pair_solreffriction : nullptr);
  return MJH_OK;
}
// (a model with connect equalities, MjhModel.has_connect: the instantiation that carries their rows -- no other model launches it, and k_mid never)
template <int G>
static int launch_constraint_g(const MjhModel* m, const MjhData* d, hipStream_t s) {
  const ConLayout lay = con_layout(m->nv, d->njmax, d->concap, m->nbody, m->ngeom);
  if (m->has_connect) {
    if (!m->eq_kind) return fail(MJH_E_ARG, "Model.eq_kind missing (a model with connect equalities; INTEGRATION.md ABI v45)");
    return launch_per_world(k_make_constraint<G, true>, "k_make_constraint: does not fit in LDS", G, 0, sizeof(float) * lay.total, d->nworld, s, *m, *d);
  }
  return launch_per_world(k_make_constraint<G>, "k_make_constraint: does not fit in LDS", G, 0, sizeof(float) * lay.total, d->nworld, s, *m, *d);
}
static int launch_constraint(const MjhModel* m, const MjhData* d, hipStream_t s) { return lanes64(m) ? launch_constraint_g<64>(m, d, s) : launch_constraint_g<32>(m, d, s); }
static int launch_rne_postconstraint(const MjhModel* m, const MjhData* d, hipStream_t s) {
  const int wpb = lds_wpb32((size_t)18 * m->nbody);
  if (!wpb) return fail(MJH_E_UNSUPPORTED, "k_rne_postconstraint: nbody does not fit in LDS");
  const size_t lds = sizeof(float) * 18 * m->nbody * wpb;
  HIPCHK(set_lds(k_rne_postconstraint<32>, lds));
  hipLaunchKernelGGL(k_rne_postconstraint<32>, dim3((d->nworld + wpb - 1) / wpb), dim3(32 * wpb), lds, s, *m, *d);
  return MJH_OK;
}
static int launch_subtree_vel(const MjhModel* m, const MjhData* d, hipStream_t s) {
  const int wpb = subtree_vel_wpb(m->nbody);
  if (!wpb) return fail(MJH_E_UNSUPPORTED, "k_subtree_vel: nbody does not fit in LDS");
  const size_t lds = sizeof(float) * 9 * m->nbody * wpb;
  HIPCHK(set_lds(k_subtree_vel<32>, lds));
  hipLaunchKernelGGL(k_subtree_vel<32>, dim3((d->nworld + wpb - 1) / wpb), dim3(32 * wpb), lds, s, *m, *d);
  return MJH_OK;
}
static int launch_energy(const MjhModel* m, const MjhData* d, hipStream_t s) {
  if (!d->energy) return fail(MJH_E_ARG, "Data.energy missing (allocate Data with make_data/put_data)");
  hipLaunchKernelGGL(k_energy<32>, dim3((d->nworld + 7) / 8), dim3(256), 0, s, *m, *d);
  return MJH_OK;
}
static int launch_sensor(const MjhModel* m, const MjhData* d, int stage, const Run& run) {  // stage 1: acceleration-stage sensors (after the solver)
  const hipStream_t s = run.s;
  if (stage == 0 && ((m->enableflags & ENBL_ENERGY) || m->nsensor_energy > 0)) TRY(launch_energy(m, d, s));  // Data.energy rides with the position / velocity stage sensors (forward.py:1326-1338)
  if (m->nsensor == 0 || (m->disableflags & DSBL_SENSOR) || (stage == 1 && m->nsensor_acc == 0)) return MJH_OK;
  if (stage == 1 && m->nsensor_frc > 0) {
    if (!d->cfrc_ext) return fail(MJH_E_ARG, "Data.cfrc_ext missing");
    TRY(launch_rne_postconstraint(m, d, s));
  }
  if (stage == 0 && m->nsensor_subtree > 0) {
    if (!d->subtree_linvel || !d->subtree_angmom) return fail(MJH_E_ARG, "Data.subtree_linvel / subtree_angmom missing");
    TRY(launch_subtree_vel(m, d, s));
  }
  if (!d->sensordata) return fail(MJH_E_ARG, "Data.sensordata missing (allocate Data with make_data/put_data)");
  if (m->nsensor > m->nsensor_contact + m->nsensor_collision)  // (a model whose sensors are all contact / geom distance sensors has nothing for k_sensor)
    hipLaunchKernelGGL(k_sensor, dim3((d->nworld * m->nsensor + 255) / 256), dim3(256), 0, s, *m, *d, stage);
  if (stage == 0 && m->nsensor_collision > 0) TRY(launch_sensor_collision(m, d, s));  // (k_sensor skips their slots)
  if (stage == 1 && m->nsensor_contact > 0) TRY(launch_sensor_contact(m, d, s));  // (k_sensor skips their slots)
  // delayed sensors of this stage: sensordata = their buffer at time - delay, then the fresh values go into the buffer (no launch without them)
  if ((stage == 0 ? m->nsensor_history_posvel : m->nsensor_history_acc) > 0) TRY(launch_history_sensor(m, d, stage, run.hist_insert ? 1 : 0, s));
  return MJH_OK;
}
// the linear system of the fully implicit integrator (csrc/implicit.hpp): Data.ws_iacc = (M - h dF/dv)^-1 M qacc
static int launch_implicit(const MjhModel* m, const MjhData* d, hipStream_t s) {
  const ImpLayout lay = imp_layout(m->nv, m->nbody, 32);
  int wpb = 2;
  if (sizeof(float) * lay.total * 2 > (size_t)kLdsPerCU) wpb = 1;
  const size_t lds = sizeof(float) * lay.total * wpb;
  if (lds > (size_t)kLdsPerCU) return fail(MJH_E_UNSUPPORTED, "k_implicit_solve: nv / nbody do not fit in LDS");
  HIPCHK(set_lds(k_implicit_solve<32>, lds));
  hipLaunchKernelGGL(k_implicit_solve<32>, dim3((d->nworld + wpb - 1) / wpb), dim3(32 * wpb), lds, s, *m, *d);
  return MJH_OK;
}
static int launch_integrate(const MjhModel* m, const MjhData* d, int mode, hipStream_t s) {
  if (mode == 2) TRY(launch_implicit(m, d, s));
  const IntLayout lay = int_layout(m->nv, m->nC);
  return launch_per_world(k_integrate<32>, "k_integrate: does not fit in LDS", 32, sizeof(int) * mstruct_ints(m->nv, m->nC), sizeof(float) * lay.total, d->nworld, s, *m, *d, mode);
}

// ---- composite launches of the fused step --------------------------------------------------------------------
// Cross-stream fork/join costs 5-15 us per hop on the critical path (event record -> barrier packet -> dispatch),
// while consecutive kernels of one stream start back to back.  The fused step therefore uses ONE stream and gives
// the workgroups of a launch different roles:
//   k_mid           : {collision -> make_constraint} workgroups, then the (shorter) fwd_vel workgroups (both only depend
//                     on k_fwd_pos; both are latency-bound, so they share the CUs)
//   k_solve_plus    : solver workgroups (longest expected solve first), then factor_smooth and publish workgroups: dispatched last,
//                     they fill the CUs that the solver's stragglers leave idle
//   k_fwd_pos_plus  : k_fwd_pos + one workgroup computing the solver schedule from the previous step's solver_niter
//   k_integrate_plus: integrator workgroups, then publish_contacts workgroups
template <int G, bool HEAVY, bool HFT = true>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((!HEAVY && G >= 32) ? MJH_MID_WAVES : 1, 8))) k_mid(MjhModel m, MjhData d, int ncc, int nvb, int nw_cc, int nw_v, int stride_cc, int sched) {  // (the light instantiation: four wavefronts per SIMD = 128 registers, its occupancy since round 3)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  (void)nvb;
  // sched: workgroup 0 sorts the solver schedule here instead of in the k_fwd_pos launch (models whose fwd_pos
  // workgroups are too small to do it quickly)
  // (LAST in the dispatch order, round 5: every launch of the step fills the device's workgroup slots exactly -- LDS-bound, four per CU --, so
  // one more workgroup in front pushes a real one into a second round: + 7 us here, + 8 us in k_fwd_pos_plus, measured.  Behind the
  // velocity-stage workgroups it takes the first slot one of them frees and ends inside the spread of their finish times.)
  if (sched && blockIdx.x == gridDim.x - 1) {
    schedule_body(d, reinterpret_cast<int*>(smem), blockDim.x, sched_cls(m, d));
    return;
  }
  const int bi = (int)blockIdx.x;
  const int cc_before = bi < ncc ? (int)bi : ncc;               // longest jobs first: all CC workgroups, then fwd_vel
  const bool is_cc = bi < ncc;
  if (is_cc) {
    const Blk b{cc_before * nw_cc, nw_cc, nw_cc * G};
    collision_body<G, HEAVY, 0, HFT>(m, d, smem, b, stride_cc);
    __threadfence_block();  // the world's contact records (global) are read back by the same lanes
    make_constraint_body<G>(m, d, smem, b, stride_cc);
  } else {
    const Blk b{((int)bi - cc_before) * nw_v, nw_v, nw_v * G};
    fwd_vel_body<G>(m, d, VEL_COMVEL, VEL_ACCEL, smem, b);
  }
}
template <int G>
__global__ void __launch_bounds__(256) k_integrate_plus(MjhModel m, MjhData d, int mode, int nint, int npub) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wpb = blockDim.x / G, bi = blockIdx.x;
  if (bi < nint) integrate_body<G>(m, d, mode, smem, Blk{bi * wpb, wpb, (int)blockDim.x});
  else if (bi < nint + npub) publish_body<G>(d, 1, reinterpret_cast<int*>(smem), Blk{(bi - nint) * wpb, wpb, (int)blockDim.x}, m.nexplicit ? m.pair_solreffriction : nullptr);
  else factor_smooth_body<G>(m, d, 1, smem, Blk{(bi - nint - npub) * wpb, wpb, (int)blockDim.x});  // Newton only, see k_solve_plus
}
// k_fwd_pos + one workgroup that sorts the worlds by the PREVIOUS step's solver_niter (the solver schedule of this step)
template <int G>
__global__ void __launch_bounds__(256) k_fwd_pos_plus(MjhModel m, MjhData d, int first, int last, int npos, NoiseArgs noise) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  // the schedule workgroup goes FIRST: workgroups are dispatched in index order, so as the last one it would start
  // when the launch is nearly over and add its whole duration (~8 us) to it
  if (blockIdx.x == 0) {
    if (noise.sched) schedule_body(d, reinterpret_cast<int*>(smem), blockDim.x, sched_cls(m, d));
  } else if ((int)blockIdx.x <= npos) {
    const int wpb = blockDim.x / G;
    fwd_pos_body<G>(m, d, first, last, smem, Blk{((int)blockIdx.x - 1) * wpb, wpb, (int)blockDim.x});
  } else {
    // the benchmark loop's control noise rides here (mjh_timed_steps): nothing in this launch reads ctrl, the next launch
    // (fwd_vel's actuation) does; dispatched last, these few trivial workgroups run in the launch's tail
    const int idx = ((int)blockIdx.x - npos - 1) * blockDim.x + threadIdx.x;
    if (idx < noise.n) ctrl_noise_elem(m, d, noise.center, noise.step, noise.noise_std, noise.noise_rate, idx);
  }
}

template <int G>
static int launch_mid_g(const MjhModel* m, const MjhData* d, bool sched, hipStream_t s) {
  if constexpr (G != 16) {  // (16 lanes: light colliders only, see lanes16)
    if (m->heavy_colliders && d->ws_ccd) TRY(launch_ccd_pre<G>(m, d, s));
  }
  const ConLayout cl = con_layout(m->nv, d->njmax, d->concap, m->nbody, m->ngeom);
  const int stride_cc = std::max(cl.total, collide_lds_words(m->ngeom, m->npair, d->concap, m->heavy_colliders ? m->broadphase : 0, m->heavy_colliders && d->ws_ccd != nullptr) | 1);
  const VelLayout vl = vel_layout(m->nq, m->nv, m->nbody, m->nC, m->nu);
  const size_t ms_bytes = sizeof(int) * mstruct_ints(m->nv, m->nC);
  // 8 collision+constraint worlds per workgroup; as many fwd_vel worlds as fit in the same LDS footprint
  int nw_cc = 256 / G;
  while (nw_cc > 1 && sizeof(float) * stride_cc * nw_cc > (size_t)kLdsPerCU / 2) nw_cc >>= 1;
  size_t lds = sizeof(float) * stride_cc * nw_cc;
  int nw_v = (int)((lds > ms_bytes ? lds - ms_bytes : 0) / (sizeof(float) * vl.total));
  if (nw_v < 1) nw_v = 1;
  if (nw_v > 256 / G) nw_v = 256 / G;
  // an odd world count leaves half a wavefront slot empty: round up when the same number of workgroups still fits a CU
  if ((nw_v & 1) && nw_v < 256 / G) {
    const size_t up = ms_bytes + sizeof(float) * vl.total * (nw_v + 1);
    if ((size_t)kLdsPerCU / std::max(up, lds) == (size_t)kLdsPerCU / lds) ++nw_v;
    else --nw_v;
  }
  if (nw_v < 1) nw_v = 1;
  if (const char* e = knob_str("MJH_MID_W")) {  // tuning knob (developer only): worlds per workgroup of both roles
    nw_cc = nw_v = atoi(e);
    lds = sizeof(float) * stride_cc * nw_cc;
  }
  lds = std::max(lds, ms_bytes + sizeof(float) * vl.total * nw_v);
  if (lds > (size_t)kLdsPerCU) return fail(MJH_E_UNSUPPORTED, "k_mid: model does not fit in LDS");
  const int ncc = (d->nworld + nw_cc - 1) / nw_cc, nvb = (d->nworld + nw_v - 1) / nw_v;
  const dim3 grid(ncc + nvb + (sched ? 1 : 0)), block(G * std::max(nw_cc, nw_v));
  auto go = [&](auto kernel, const char* name) {
    HIPCHK(set_lds(kernel, lds));
    debug_occupancy(name, kernel, (int)grid.x, (int)block.x, lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, *m, *d, ncc, nvb, nw_cc, nw_v, stride_cc, sched ? 1 : 0);
    return MJH_OK;
  };
  if constexpr (G != 16) {  // (heavy colliders without height fields: the instantiation without their per-lane GJK / EPA)
    if (m->heavy_colliders) return m->nhfield > 0 ? go(k_mid<G, true, true>, "k_mid<heavy>") : go(k_mid<G, true, false>, "k_mid<heavy>");
  }
  return go(k_mid<G, false>, "k_mid");
}
static int launch_mid(const MjhModel* m, const MjhData* d, bool sched, hipStream_t s) { return lanes16(m) ? launch_mid_g<16>(m, d, sched, s) : lanes64(m) ? launch_mid_g<64>(m, d, sched, s) : launch_mid_g<32>(m, d, sched, s); }
static int solve_supported(const MjhModel* m, const MjhData* d) {
  if (m->cone != CONE_PYRAMIDAL && m->cone != CONE_ELLIPTIC) return fail(MJH_E_UNSUPPORTED, "unknown cone type");
  if (m->solver != SOL_NEWTON && m->solver != SOL_CG && m->solver != SOL_PGS) return fail(MJH_E_UNSUPPORTED, "unknown solver");
  if (m->nv <= 64 && d->njmax > 192 && m->solver == SOL_PGS && m->cone != CONE_ELLIPTIC)
    return fail(MJH_E_UNSUPPORTED, "njmax > 192 with the register / LDS resident PGS kernels is not supported (nv <= 64, pyramidal)");
  return MJH_OK;
}
// The ONE set of side streams per host thread and device, created on first use and released by mjh_release_thread_resources().  Two users,
// never in the same step:
//   the per-island dispatch (nv > 64; launch_solve_any): the rare island classes (one stream each: round 6) and the generic solver touch
//     islands / worlds the common-class launch skips, so they run beside it instead of after it -- all MJH_NAUX streams;
//   the Newton riders (plan_step: RIDE_SIDE): the public-output riders (contact publication, L'DL factor + qacc_smooth) cannot ride with the
//     solver launch (its 256 VGPRs throttle them) and cost 55 us at the end of the integrator launch; they run beside the solver instead --
//     stream 0 and join 0.  Two event hops (fork after k_mid, join after the integrator), neither on the solver's critical path.
// Round 6: the riders' stream IS the first auxiliary stream of the per-island solver.  A stream of its own cost every later model of the
// process its solver concurrency: once it existed -- any Newton model of at most 32 dofs stepped earlier -- the four class launches of
// clutter_synth ran 25 % slower (1.43 -> 1.07 M env-steps/s, tools/interference_probe.py: the runtime multiplexes user streams onto a few
// hardware queues, and streams that share one run in order).  MJH_NO_AUX (developer knob): the set is ONE stream, at the lowest priority, for
// the riders alone.  (Retired experiment, LAB_NOTES.md R3: high / normal priority -- no difference, queue priority does not arbitrate CU
// slots; the riders' workgroups only get slots as the solver's retire.)  Under instrumentation (one stream, one event pair per launch) nothing
// is created or handed out.
#define MJH_NAUX 4
#define MJH_NAUX_EAGER 4  // (see launch_solve_any: eager launches pay for the forks while few islands are awake, and win afterwards)
struct Streams {
  int n;  // streams in the set: MJH_NAUX, or 1 under MJH_NO_AUX
  hipStream_t stream[MJH_NAUX];
  hipEvent_t fork, join[MJH_NAUX];
};
static thread_local Streams* g_streams_per_dev[16] = {nullptr};
static Streams* side_streams(const Run& run) {
  if (run.instr) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  if (!g_streams_per_dev[dev]) {
    Streams* a = new Streams();
    a->n = KNOB_ONCE_FLAG("MJH_NO_AUX") ? 1 : MJH_NAUX;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
    bool ok = hipEventCreateWithFlags(&a->fork, hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < a->n && ok; ++k)
      ok = (a->n == 1 ? hipStreamCreateWithPriority(&a->stream[k], hipStreamNonBlocking, least) : hipStreamCreateWithFlags(&a->stream[k], hipStreamNonBlocking)) == hipSuccess &&
           hipEventCreateWithFlags(&a->join[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      delete a;  // (a partially created set leaks a handle or two: only on an already failing device)
      return nullptr;
    }
    g_streams_per_dev[dev] = a;
  }
  return g_streams_per_dev[dev];
}
// ---- the step plan: every decision of a step that more than one launch depends on, taken ONCE ---------------------------------------
// plan_step is the one place that decides which solver kernel serves (m, d) and where the public-output riders (contact publication, L'DL
// factor + qacc_smooth) go; run_stage passes the plan down, launch_solve_any switches on it, mjh_solver_kernel reports it.  Pure: nothing
// is launched, no stream is touched, nothing allocated.
// Adding a solver kernel touches: one SolverFamily value + its string, one branch in plan_step, one branch in launch_solve_any, one launcher
// declaration in host.hpp, one unit in _abi.UNITS and unity.hip.
enum SolverFamily { FAM_UNSUPPORTED, FAM_PGS, FAM_PGS_BIG, FAM_BIG, FAM_TREE_BIG, FAM_CG64, FAM_CG64_ELL, FAM_NEWTON64, FAM_NEWTON64_ELL,
                    FAM_NEWTON_MFMA, FAM_NEWTON32, FAM_NEWTON32_ELL, FAM_CG32_ELL, FAM_CGW, FAM_CGP, FAM_PAIR };
static const char* const kFamilyName[] = {"unsupported", "pgs", "pgs_big", "big", "tree+big", "cg64", "cg64_ell", "newton64", "newton64_ell",
                                          "newton_mfma", "newton32", "newton32_ell", "cg32_ell", "cgw", "cgp", "pair"};
// who carries the riders: nobody (the stage API: its plain kernels), trailing workgroups of the solver launch (CG; Newton "inline", MFMA kernel
// only), a launch of their own on the side stream beside the solver (Newton), or the integrator launch
enum Riders { RIDE_NONE, RIDE_SOLVER, RIDE_SIDE, RIDE_INTEGRATOR };
struct StepPlan {
  int mode;        // integrator: 0 Euler, 1 implicitfast, 2 implicit (k_integrate's argument)
  int fuse_euler;  // the solver's epilogue integrates: 0 no (the integrator launch does), 1 explicit Euler, 2 implicitfast
  Riders riders;
  SolverFamily family;
  bool newton, ell;  // (ell: elliptic(m, d))
  bool r1;           // Newton, elliptic cones: the one-row-per-lane launch for the worlds of at most 32 rows goes first
};
static inline int integrator_mode(const MjhModel* m) { return m->integrator == INT_IMPLICITFAST ? 1 : (m->integrator == INT_IMPLICIT ? 2 : 0); }  // (k_integrate's argument)
static SolverFamily plan_family(const MjhModel* m, const MjhData* d, bool ell, int fuse_euler) {
  if (solve_supported(m, d)) return FAM_UNSUPPORTED;
  const bool newton = m->solver == SOL_NEWTON;
  if (m->solver == SOL_PGS) return m->nv > 64 || ell ? FAM_PGS_BIG : FAM_PGS;
  if (m->nv > 64) return m->tree_solve ? FAM_TREE_BIG : FAM_BIG;
  // the k_solve_plus instantiations: by lanes per world (32 up to 32 dofs, 64 beyond), solver and cone
  if (m->nv > 32) return newton ? (ell ? FAM_NEWTON64_ELL : FAM_NEWTON64) : (ell ? FAM_CG64_ELL : FAM_CG64);
  if (newton) {
    if (ell) return FAM_NEWTON32_ELL;
    // the MFMA kernel (solver_newton.hpp) takes every world of a batch with njmax <= 64; 32-bit byte offsets inside the kernel: nworld *
    // max(nv, njmax) * 4 must fit.  MJH_OLD_NEWTON (developer knob): A/B against the VALU solver
    const bool mfma = !KNOB_ONCE_FLAG("MJH_OLD_NEWTON") && d->njmax <= 64 && (double)d->nworld * std::max(m->nv, d->njmax) * 4.0 < 4.0e9;
    return mfma ? FAM_NEWTON_MFMA : FAM_NEWTON32;
  }
  if (ell) return FAM_CG32_ELL;
  // Which CG kernel serves the class nv <= 32, pyramidal cones:
//   cgw       one world per wavefront (solver_cgw.hpp): SMALL batches.  A solve is a dependent chain of ~17 k instructions per wavefront of which
//             the line search's per-wavefront bookkeeping is the bulk, so pairing two worlds in a wavefront halves the instruction count per world
//             and wins whenever the SIMDs are issue bound (measured, humanoid: 8192 worlds 194 us one-per-wavefront vs 193 paired, 141 M vs 81 M
//             VALU instructions); with at most ~3 wavefronts per SIMD the chain's latency decides instead and the shorter chain of the unpaired
//             kernel wins (1024 worlds: 88 vs 112 us, 2048: 103 vs 120, 3072: 122 vs 124)
//   cgp       the pooled contact-basis kernel (solver_cgp.hpp): larger batches of models whose contacts are condim 1 / 3 and that have no
//             friction-loss rows (MjhModel.cg_basis), njmax <= 64
//   pair      k_solve<cg> (solver.hpp): everything else
  // MJH_CG_KERNEL = cgp / pair / cgw (developer knob, live; tests set it through mjh_dev_knob) forces one of the three where it applies.
  const bool wide_can = fuse_euler != 2;  // (its half rows of M do not serve the fused implicitfast update)
  const bool wide = m->nv >= KNOB_ONCE_INT("MJH_CGW_MIN_NV", 13) && d->nworld <= KNOB_ONCE_INT("MJH_CGW_MAX_NWORLD", 3072) && wide_can;
  const bool cgp_can = m->cg_basis && d->njmax <= 64 && m->nv >= 1;
  const char* force = knob_str("MJH_CG_KERNEL");
  if (force && !strcmp(force, "cgw")) return wide_can ? FAM_CGW : FAM_PAIR;
  if (force && !strcmp(force, "pair")) return FAM_PAIR;
  if (force && !strcmp(force, "cgp")) return cgp_can ? FAM_CGP : FAM_PAIR;
  return wide ? FAM_CGW : (cgp_can ? FAM_CGP : FAM_PAIR);
}
// stage: MJH_STAGE_STEP / MJH_STAGE_FORWARD plan the fused launches; any other stage plans a bare solve (the stage API, the plain path, the sleep path)
// instrumented: per-kernel event pairs are on (one stream, no side launches).  side_ok = false: the side stream could not be created
static StepPlan plan_step(const MjhModel* m, const MjhData* d, int stage, bool instrumented, bool side_ok = true) {
  StepPlan p;
  p.mode = integrator_mode(m);
  p.newton = m->solver == SOL_NEWTON;
  p.ell = elliptic(m, d);
  p.fuse_euler = 0;
  p.riders = RIDE_NONE;
  if (stage == MJH_STAGE_STEP || stage == MJH_STAGE_FORWARD) {
    const bool step = stage == MJH_STAGE_STEP;
    // The Newton riders as trailing workgroups of the MFMA solver launch (solver_newton.hpp) instead of a side-stream launch, for SMALL models
    // (round 3).  Where the solve is short the side stream's fork / join hops and the riders' late start set the step: Panda (nv 9, njmax 5: solver
    // 22 us) 135.0 -> 117.2 us per step (60.7 -> 69.9 M env-steps/s, two interleaved pairs on one box).  Where the solve is long the riders'
    // workgroups in its tail cost more than the join they save: humanoid (nv 27) 0.2824 / 0.2844 -> 0.2894 / 0.2897 ms, so the side stream stays
    // above 16 dofs.  Only with the MFMA kernel.  MJH_NEWTON_RIDERS=0 / 1 forces it off / on (developer knob).
    const int inl_force = KNOB_ONCE_INT("MJH_NEWTON_RIDERS", -1);
    const bool inl = step && !instrumented && (inl_force >= 0 ? inl_force != 0 : m->nv <= 16) && plan_family(m, d, p.ell, 0) == FAM_NEWTON_MFMA;
    // Newton only: the riders cannot ride with the solver launch of larger models (its 256 VGPRs throttle them) and cost 55 us at the end of the
    // integrator launch; they run on a side stream beside the solver instead (see side_streams)
    // (nv <= 32 only: beside the 64-lane solver of larger models the riders cost more than they save, G1 -3 %)
    const bool side = p.newton && m->nv <= KNOB_ONCE_INT("MJH_SIDE_NV", 32) && !instrumented && !inl && side_ok && !KNOB_ONCE_FLAG("MJH_NO_SIDE");  // developer knobs
    p.riders = inl || (m->solver == SOL_CG && m->nv <= 64) ? RIDE_SOLVER : side ? RIDE_SIDE : RIDE_INTEGRATOR;
    // explicit Euler without activations: the velocity/position update is a few loads and stores per dof, done by the
    // solver's own epilogue (saves a launch); every other case keeps the integrator workgroups
    // (Newton: only when its riders run with the solver or on the side stream -- otherwise the integrator launch exists anyway, for them)
    const bool fusable = step && m->na == 0 && p.riders != RIDE_INTEGRATOR && m->nv <= 64 &&
                         m->nsensor_acc == 0 &&  // (acceleration-stage sensors read qvel / qacc between the solver and the integrator)
                         d->njmax <= 192;        // (beyond: some worlds go to the generic solver, which does not integrate)
    // implicitfast without activations (round 3): the dense system (M + h D - h dA/dv) x = M qacc is solved from the M row the solver holds
    // (MJH_NO_FUSE_IMPLICITFAST: developer knob, A/B)
    p.fuse_euler = !fusable ? 0
                   : (m->integrator == INT_EULER && (m->disableflags & (DSBL_EULERDAMP | DSBL_DAMPER)) != 0) ? 1
                   : (m->integrator == INT_IMPLICITFAST && !KNOB_ONCE_FLAG("MJH_NO_FUSE_IMPLICITFAST") && !m->act_velfeedback) ? 2 : 0;  // (positive velocity feedback: the matrix may be indefinite -- the integrator launch's L'DL handles that, the epilogue's Cholesky does not)
  }
  p.family = plan_family(m, d, p.ell, p.fuse_euler);
  // rows per lane (32 lanes per world): 1 covers 32 rows, 2 covers 64 rows (humanoid, panda), 6 covers 192.  Newton with elliptic cones has
  // a one-row instantiation for the worlds of at most 32 rows (the ALOHA scene: nefc 24 on average, 27 at the 95th percentile): 155 instead
  // of 191 VGPRs and 6.7 instead of 12.2 KB of LDS per world -- 2.9 instead of 1.6 wavefronts per SIMD -- and half the row work per lane:
  // 333 -> 254 us per step there (MJH_SOLVE_R1=0: developer knob, off).  The launches follow one another on the caller's stream: a batch
  // with worlds in both classes pays the latency of one more solve (on a side stream beside the 64-row launch the ALOHA scene LOST 17 %:
  // 4.95 vs 5.97 M env-steps/s, the fork / join hops inside the step's graph).  (The same for CG with pyramidal cones was built and
  // measured on the humanoid -- bit-identical results, but no gain: behind one another 0.471 vs 0.369 ms per step at nefc 46 where a
  // quarter of the worlds are in the small class; side by side 0.370 vs 0.372 ms there and 0.349 vs 0.329 ms at nefc 32.  Not kept.)
  p.r1 = p.family == FAM_NEWTON32_ELL && d->njmax > 32 && KNOB_ONCE_INT("MJH_SOLVE_R1", 1) != 0;
  return p;
}
// the launches of the plan's solver family (fe: the solver's epilogue integrates; with_factor: the riders are its trailing workgroups)
static int launch_solve_any(const MjhModel* m, const MjhData* d, const StepPlan& p, const Run& run) {
  const hipStream_t s = run.s;
  const int fe = p.fuse_euler, all = 0x7fffffff;
  const bool with_factor = p.riders == RIDE_SOLVER;
  // njmax > 192: the register-resident kernels end at 192 rows (6 x 32 / 3 x 64 lanes); the (rare) worlds beyond go to the generic
  // solver, which keeps J in HBM and is generic in njmax
  const int top = d->njmax > 192 ? 192 : all;
  switch (p.family) {
    case FAM_UNSUPPORTED: return solve_supported(m, d);  // (its code and message)
    case FAM_PGS: return launch_pgs(m, d, s);
    case FAM_PGS_BIG: return launch_pgs_big(m, d, s);  // (the generic PGS kernel: csrc/pgs_big.hpp)
    case FAM_BIG: return launch_solve_big(m, d, s);    // (nv > 64: no riders, they go with the integrator launch)
    case FAM_TREE_BIG: {
      // constraint islands (trees joined by coupling rows): worlds whose islands all have at most 64 dofs are solved per island by the
      // register-resident kernels, the others by the generic solver below
      hipLaunchKernelGGL(k_isl_clear, dim3(1), dim3(64), 0, s, *d);
      hipLaunchKernelGGL(k_tree_rows, dim3(d->nworld), dim3(64), sizeof(int) * (size_t)(2 * std::max(d->njmax, 1) + 2 * m->ntree), s, *m, *d);
      Streams* aux = side_streams(run);
      if (aux && aux->n < MJH_NAUX) aux = nullptr;  // (MJH_NO_AUX)
      // One stream per rare island class (round 6).  clutter_synth, 2048 worlds, steps 100-300 (tools/clutter_ab.py, bit-identical states, two
      // interleaved rounds): hipGraph replay -- the reference's own way to run a step, cli.py:262-290 -- none 1.27, one shared side stream 1.29,
      // one each 1.43 M env-steps/s; eager launches 1.28 / 1.28 / 1.40.  (Eager, steps 0-100 -- five trees awake, every class launch nearly
      // empty -- the forks are host API calls on the critical path: 1.74 / 1.48 / 1.51; the graph replay does not pay them: 1.75 / 1.73 / 1.78.)
      int naux = 0;
      if (aux) {
        hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
        naux = (hipStreamIsCapturing(s, &cst) == hipSuccess && cst == hipStreamCaptureStatusActive) ? MJH_NAUX : MJH_NAUX_EAGER;
        const int cap = KNOB_ONCE_INT("MJH_NAUX", -1);  // developer knob (A/B): 2 = one side stream for the rare classes, 4 = one each
        if (cap >= 2 && cap <= MJH_NAUX) naux = cap;
      }
      // stream 0: islands of 8..16 dofs; 1: the generic solver (worlds with an island beyond 64 dofs); 2: 16..32 dofs; 3: many rows / 33..64 dofs.
      // (Retired experiment, LAB_NOTES.md R6.14: the generic solver behind the 16..32-dof class on stream 2, four branches instead of five -- nothing.)
      hipStream_t s1 = aux ? aux->stream[0] : s, s2 = aux ? aux->stream[1] : s, s3 = naux > 2 ? aux->stream[2] : s1, s4 = naux > 3 ? aux->stream[3] : s1;
      if (aux) {
        HIPCHK(hipEventRecord(aux->fork, s));
        for (int k = 0; k < naux; ++k) HIPCHK(hipStreamWaitEvent(aux->stream[k], aux->fork, 0));
      }
      int rc = (p.newton ? (p.ell ? launch_solve_tree_newton_ell : launch_solve_tree_newton) : (p.ell ? launch_solve_tree_cg_ell : launch_solve_tree_cg))(m, d, s, s1, s3, s4);
      if (!rc) rc = launch_solve_big(m, d, s2);
      if (aux) {  // (every fork rejoins the caller's stream, also on the error path: the streams may be under capture)
        for (int k = 0; k < naux; ++k) {
          HIPCHK(hipEventRecord(aux->join[k], aux->stream[k]));
          HIPCHK(hipStreamWaitEvent(s, aux->join[k], 0));
        }
      }
      return rc;
    }
    case FAM_NEWTON_MFMA: return launch_solve_newton_mfma(m, d, with_factor, fe, s);
    case FAM_CGP: {
      // CG, pyramidal, contacts of condim 1 / 3, njmax <= 64 (the headline class): contact-basis rows in one row pool per workgroup, three
      // wavefronts per SIMD (solver_cgp.hpp); the worlds it flags (a contact cut by njmax, a pool overflow) are solved by k_solve<cg> in the
      // launch behind it, which is empty in the common case.
      if (int rc = launch_solve_cgp(m, d, with_factor, fe, s)) return rc;
      return launch_solve_32_cg_deferred(m, d, fe, s);
    }
    case FAM_CGW:
    case FAM_PAIR:
    case FAM_CG32_ELL:
    case FAM_NEWTON32:
    case FAM_NEWTON32_ELL: {
      // 32 lanes per world, 2 rows per lane cover 64 rows, 6 cover 192 (the one-row launch of plan.r1: see plan_step)
      auto s32 = p.ell ? (p.newton ? launch_solve_32_newton_ell : launch_solve_32_cg_ell) : (p.newton ? launch_solve_32_newton : launch_solve_32_cg);
      const bool wide = p.family == FAM_CGW;
      int lo2 = -1;
      if (p.r1) {
        if (int rc = launch_solve_32_newton_ell_r1(m, d, false, fe, s, -1, 32)) return rc;
        lo2 = 32;
      }
      // njmax > 64: two launches over the same world list (see solve_body): a small-row instantiation for the worlds with
      // at most 64 rows, the big one (riders attached) for the rest
      if (d->njmax <= 64) return wide ? launch_solve_cgw(m, d, with_factor, fe, s, -1, all) : s32(m, d, 2, with_factor, fe, s, lo2, all);
      if (int rc = wide ? launch_solve_cgw(m, d, false, fe, s, -1, 64) : s32(m, d, 2, false, fe, s, lo2, 64)) return rc;
      if (int rc = s32(m, d, 6, with_factor, fe, s, 64, top)) return rc;
      return d->njmax > 192 ? launch_solve_big(m, d, s, 192) : MJH_OK;
    }
    case FAM_CG64:
    case FAM_CG64_ELL:
    case FAM_NEWTON64:
    case FAM_NEWTON64_ELL: {
      // 64 lanes per world: 1 / 2 / 3 rows per lane cover 64 / 128 / 192 rows.  The second launch of a pair runs after the first on the same
      // stream, so the split point is chosen to leave it (almost) empty: its real worlds would otherwise be a serial tail on an idle GPU (G1:
      // 6 % of the worlds exceed 64 rows, practically none exceed 128).
      // (Retired experiments, LAB_NOTES.md R6.5: the worlds of at most 64 rows in a one-row launch of their own, in front -- G1 7.84 vs 9.14 M
      // env-steps/s -- or beside the others on an auxiliary stream -- 9.75 -> 9.64 M; the two-row launch bounded at 112 / 96 rows instead of 128 --
      // 9.54 / 9.47 / 9.44 M.)
      auto s64 = p.ell ? (p.newton ? launch_solve_64_newton_ell : launch_solve_64_cg_ell) : (p.newton ? launch_solve_64_newton : launch_solve_64_cg);
      if (d->njmax <= 64) return s64(m, d, 1, with_factor, fe, s, -1, all);
      if (d->njmax <= 128) return s64(m, d, 2, with_factor, fe, s, -1, all);
      if (int rc = s64(m, d, 2, with_factor, fe, s, -1, 128)) return rc;
      if (int rc = s64(m, d, 3, false, fe, s, 128, top)) return rc;
      return d->njmax > 192 ? launch_solve_big(m, d, s, 192) : MJH_OK;
    }
  }
  return fail(MJH_E_ARG, "launch_solve_any: unknown solver family");
}
static int launch_solve(const MjhModel* m, const MjhData* d, const Run& run) { return launch_solve_any(m, d, plan_step(m, d, MJH_STAGE_SOLVE, run.instr != nullptr), run); }  // (the bare solve: no riders, no fused integrator)
// name of the solver family of (m, d) in a fused step -- the plan, nothing launched
static const char* solver_kernel_name(const MjhModel* m, const MjhData* d) { return kFamilyName[plan_step(m, d, MJH_STAGE_STEP, false).family]; }
// integrator workgroups (integrate) and the riders -- contact publication, L'DL factor + qacc_smooth -- (with_factor)
static int launch_integrate_plus(const MjhModel* m, const MjhData* d, int mode, bool integrate, bool with_factor, hipStream_t s) {
  constexpr int G = 32;  // (see launch_factor_smooth)
  const IntLayout lay = int_layout(m->nv, m->nC);
  const FacLayout fl = fac_layout(m->nv, m->nC);
  const size_t ms_bytes = sizeof(int) * mstruct_ints(m->nv, m->nC);
  size_t lds = std::max(ms_bytes + sizeof(float) * std::max(lay.total, fl.total) * (256 / G), (size_t)2048);
  if (lds > (size_t)kLdsPerCU) return fail(MJH_E_UNSUPPORTED, "k_integrate: does not fit in LDS");
  HIPCHK(set_lds(k_integrate_plus<G>, lds));
  const int nb = (d->nworld + 256 / G - 1) / (256 / G);
  // (the riders: here when the plan says RIDE_INTEGRATOR, and on the side stream, as a launch without integrator workgroups)
  const int nint = integrate ? nb : 0, npub = with_factor ? nb : 0, nfac = with_factor ? nb : 0;
  if (nint + npub + nfac == 0) return MJH_OK;
  if (integrate && mode == 2) TRY(launch_implicit(m, d, s));
  debug_occupancy("k_integrate_plus", k_integrate_plus<G>, nint + npub + nfac, 256, lds);
  hipLaunchKernelGGL(k_integrate_plus<G>, dim3(nint + npub + nfac), dim3(256), lds, s, *m, *d, mode, nint, npub);
  return MJH_OK;
}
// the pending control noise (Run::noise) as a launch of its own, under its own class; mjh_ctrl_noise is this launch
static void apply_noise(const MjhModel* m, const MjhData* d, Run& run) {
  const NoiseArgs noise = run.noise;
  run.noise.n = 0;
  if (noise.n == 0) return;
  Scope sc(run, K_NOISE);
  hipLaunchKernelGGL(k_ctrl_noise, dim3((noise.n + 255) / 256), dim3(256), 0, run.s, *m, *d, noise.center, noise.step, noise.noise_std, noise.noise_rate);
}
// *sched_done: whether the launch carried the schedule workgroup (it needs >= 128 threads to be quick; otherwise it
// rides with k_mid, whose workgroups always have 256).  The pending control noise rides with the same launch, or goes in front of the plain one.
template <int G>
static int launch_pos_plus_g(const MjhModel* m, const MjhData* d, int first, int last, bool* sched_done, Run& run) {
  const hipStream_t s = run.s;
  const PosLayout lay = pos_layout(m->nq, m->nv, m->nbody, m->njnt, m->nC, last >= POS_FACTOR);
  size_t lds;
  const int threads = pick_block(sizeof(int) * pos_shared_words(m->nv, m->nC, m->nbody, m->njnt, m->nbodylevel, m->ngeom, m->nsite), sizeof(float) * lay.total, G, &lds);
  if (!threads) return fail(MJH_E_UNSUPPORTED, "k_fwd_pos: model does not fit in LDS");
  // The schedule workgroup is this launch's first workgroup.  Round 5: its sort was a chain of 32 dependent memory round trips (13 us: the tail of
  // whichever launch carried it -- fused k_fwd_pos 48 us against 39 us without it); with its loads in one batch (integrate.hpp schedule_body) it
  // costs this launch 2 us.  (Retired experiment, LAB_NOTES.md R5: always as k_mid's last workgroup -- 0.2902 / 0.2745 against 0.2914 / 0.2698 ms per step here.)
  *sched_done = threads >= 128;
  if (threads < 128) {
    apply_noise(m, d, run);
    return launch_pos(m, d, first, last, s);
  }
  lds = std::max(lds, (size_t)2048);  // (the schedule workgroup: 512 ints)
  NoiseArgs noise = run.noise;
  run.noise.n = 0;
  noise.sched = *sched_done ? 1 : 0;
  HIPCHK(set_lds(k_fwd_pos_plus<G>, lds));
  const int wpb = threads / G, npos = (d->nworld + wpb - 1) / wpb, nnoise = (noise.n + threads - 1) / threads;
  debug_occupancy("k_fwd_pos_plus", k_fwd_pos_plus<G>, npos + 1 + nnoise, threads, lds);
  hipLaunchKernelGGL(k_fwd_pos_plus<G>, dim3(npos + 1 + nnoise), dim3(threads), lds, s, *m, *d, first, last, npos, noise);
  return MJH_OK;
}
// Never launched, kept instantiated: it shares the 16-lane helper functions with k_mid<16>, and without this second caller the compiler inlines and
// allocates registers differently in k_mid<16> (24217 -> 24165 instructions).  It goes in a change that measures the Panda step (LAB_NOTES.md R6.14).
template __global__ void k_fwd_pos_plus<16>(MjhModel, MjhData, int, int, int, NoiseArgs);
static int launch_pos_plus(const MjhModel* m, const MjhData* d, int first, int last, bool* sched_done, Run& run) { return lanes64(m) && m->nbody > 32 ? launch_pos_plus_g<64>(m, d, first, last, sched_done, run) : launch_pos_plus_g<32>(m, d, first, last, sched_done, run); }  // (never 16 lanes: see lanes16)

static int check(const MjhModel* m, const MjhData* d) {
  if (!m || !d) return fail(MJH_E_ARG, "null model/data");
  if (d->nworld <= 0) return fail(MJH_E_ARG, "nworld must be positive");
  if (d->concap <= 0 || !d->ws_contact) return fail(MJH_E_ARG, "Data.ws_contact / concap missing (allocate Data with make_data/put_data)");
  if (m->integrator != INT_EULER && m->integrator != INT_IMPLICITFAST && m->integrator != INT_RK4 && m->integrator != INT_IMPLICIT)
    return fail(MJH_E_UNSUPPORTED, "integrator must be Euler, RK4, implicit or implicitfast");
  if (m->integrator == INT_IMPLICIT && (m->nv > 64 || !d->ws_iacc)) return fail(MJH_E_UNSUPPORTED, "fully implicit integrator: at most 64 dofs, Data allocated for this model");
  if (m->integrator == INT_RK4 && !d->ws_rk) return fail(MJH_E_ARG, "Data.ws_rk missing (allocate Data with make_data/put_data)");
  return MJH_OK;
}

// one wavefront per world (csrc/sleep.hpp k_sleep)
static int launch_sleep(const MjhModel* m, const MjhData* d, int phase, hipStream_t s) {
  if (m->has_connect) return fail(MJH_E_UNSUPPORTED, "k_sleep: connect equalities with sleeping (its wake and island passes index joints with an equality's ids)");
  const size_t lds = sizeof(int) * sleep_lds(m->ntree, m->nbody, m->nv, d->njmax, d->concap).total;
  if (lds > (size_t)kLdsPerCU) return fail(MJH_E_UNSUPPORTED, "k_sleep: the world's sleep tables do not fit in LDS");
  HIPCHK(set_lds(k_sleep, lds));
  hipLaunchKernelGGL(k_sleep, dim3(d->nworld), dim3(64), lds, s, *m, *d, phase);
  return MJH_OK;
}

// ---- the unfused stage order: one plain kernel per stage, written ONCE ----------------------------------------------------------------
// run_unfused is the whole forward / step; its pieces also serve MJH_STAGE_FWD_POSITION and the fused step of a trn_general model.  sleep: with
// the sleep bookkeeping between the stages (csrc/sleep.hpp).
static int launch_schedule(const MjhModel* m, const MjhData* d, const Run& run) {
  Scope sc(run, K_OTHER);
  hipLaunchKernelGGL(k_schedule_worlds, dim3(1), dim3(1024), 0, run.s, *d, sched_cls_host(*m, *d));
  return MJH_OK;
}
// the position stage up to `last` and, behind it, the general transmissions
static int run_pos_trn(const MjhModel* m, const MjhData* d, int last, const Run& run) {
  Scope sc(run, K_POS);
  TRY(launch_pos(m, d, POS_KINEMATICS, last, run.s));
  return launch_trn(m, d, run.s);
}
static int run_collide_constrain(const MjhModel* m, const MjhData* d, bool sleep, const Run& run) {
  const hipStream_t s = run.s;
  { Scope sc(run, K_COLLISION); TRY(launch_collision(m, d, s)); }
  if (sleep) {
    { Scope sc(run, K_OTHER); TRY(launch_sleep(m, d, (int)SLP_WAKE_COLLISION, s)); }
    // pass 2: waking only ever lets more pairs through the sleep filter, so the pairs of pass 1 plus "the pairs pass 1 skipped that
    // involve a newly awakened body" are the pairs that pass the filter now: the woken worlds recompute their list
    Scope sc(run, K_COLLISION);
    MjhData d2 = *d;
    d2.sleep_pass = 2;
    TRY(launch_collision(m, &d2, s));
  }
  // connect rows carry -Jdot qvel of the CURRENT state: the velocity kinematics (cvel, cdof_dot) go in front of them
  if (m->has_connect) { Scope sc(run, K_VEL); TRY(launch_vel(m, d, VEL_COMVEL, VEL_COMVEL, s)); }
  { Scope sc(run, K_CONSTRAINT); TRY(launch_constraint(m, d, s)); }
  if (sleep) { Scope sc(run, K_OTHER); TRY(launch_sleep(m, d, (int)SLP_POST_CONSTRAINT, s)); }
  return MJH_OK;
}
// collision -> constraint -> velocity: what k_mid does in one launch
static int run_mid_unfused(const MjhModel* m, const MjhData* d, bool sleep, const Run& run) {
  TRY(run_collide_constrain(m, d, sleep, run));
  Scope sc(run, K_VEL);
  return launch_vel(m, d, VEL_COMVEL, VEL_ACCEL, run.s);
}
// forward / step as plain kernels: the profiling pass (so that the event pairs time one kernel at a time), MJH_PLAIN, every model with
// sleeping enabled (forward.py:345-349, 652-675, 1290-1324, 1341-1347) and every model with connect equalities (k_mid does not carry them)
static int run_unfused(const MjhModel* m, const MjhData* d, bool step, bool sleep, Run& run) {
  const hipStream_t s = run.s;
  if (sleep) {
    if (!d->tree_asleep || !d->ws_sleep_J) return fail(MJH_E_ARG, "Data sleep tables missing (allocate Data with make_data/put_data)");
    if (m->solver != SOL_NEWTON) return fail(MJH_E_UNSUPPORTED, "sleeping requires the Newton solver (reference io.py:359)");
    if (step && m->integrator == INT_RK4) return fail(MJH_E_UNSUPPORTED, "sleeping with the RK4 integrator");
  }
  apply_noise(m, d, run);  // (no fused position launch to carry it; the wake-by-input test of k_sleep reads ctrl)
  if (sleep) { Scope sc(run, K_OTHER); TRY(launch_sleep(m, d, (int)SLP_WAKE, s)); }
  else TRY(launch_schedule(m, d, run));
  TRY(run_pos_trn(m, d, POS_CRB, run));
  TRY(run_mid_unfused(m, d, sleep, run));
  { Scope sc(run, K_OTHER); TRY(launch_sensor(m, d, 0, run)); }
  MjhData masked;  // sleep: the solver reads the masked copies (sleeping dofs frozen), and writes the public outputs
  if (sleep) {
    Scope sc(run, K_OTHER);
    if (m->nv > 0) hipLaunchKernelGGL(k_sleep_qfrc, dim3((d->nworld * m->nv + 255) / 256), dim3(256), 0, s, *m, *d);
    hipLaunchKernelGGL(k_sleep_mask, dim3(d->nworld), dim3(256), 0, s, *m, *d);
    masked = *d;
    masked.efc_J = d->ws_sleep_J;
    masked.qacc_warmstart = d->ws_sleep_warm;
  }
  { Scope sc(run, K_SOLVE); TRY(launch_solve(m, sleep ? &masked : d, run)); }
  { Scope sc(run, K_OTHER); TRY(launch_sensor(m, d, 1, run)); }
  if (step) { Scope sc(run, K_INTEGRATE); TRY(launch_integrate(m, d, integrator_mode(m), s)); }
  {
    // (round 6: these two public-output launches beside the solver on the side stream LOSE with sleeping -- clutter_synth 1.53 -> 1.36 M env-steps/s,
    // two interleaved pairs: their workgroups take LDS slots from the island solves, which are the step's critical path)
    Scope sc(run, K_OTHER);
    TRY(launch_publish(m, d, s));
    TRY(launch_factor_smooth(m, d, m->solver == SOL_NEWTON ? 1 : 0, s));  // CG and PGS write qacc_smooth themselves
  }
  if (sleep && step) {
    { Scope sc(run, K_OTHER); TRY(launch_sleep(m, d, (int)SLP_SLEEP, s)); }
    { Scope sc(run, K_VEL); TRY(launch_vel(m, d, VEL_COMVEL, VEL_RNE, s)); }
  }
  return MJH_OK;
}

static int run_stage(const MjhModel* m, const MjhData* d, int stage, Run& run);
// one stage as its launches; STEP with the RK4 integrator never comes here (run_stage splits it)
static int run_stage_impl(const MjhModel* m, const MjhData* d, int stage, Run& run) {
  const hipStream_t s = run.s;
  switch (stage) {
    case MJH_STAGE_KINEMATICS: { Scope sc(run, K_POS); return launch_pos(m, d, POS_KINEMATICS, POS_KINEMATICS, s); }
    case MJH_STAGE_COM_POS: { Scope sc(run, K_POS); return launch_pos(m, d, POS_COM, POS_COM, s); }
    case MJH_STAGE_CRB: { Scope sc(run, K_POS); return launch_pos(m, d, POS_CRB, POS_CRB, s); }
    case MJH_STAGE_FACTOR_M: { Scope sc(run, K_POS); return launch_pos(m, d, POS_FACTOR, POS_FACTOR, s); }
    case MJH_STAGE_COLLISION:
      { Scope sc(run, K_COLLISION); TRY(launch_collision(m, d, s)); }
      { Scope sc(run, K_OTHER); return launch_publish(m, d, s); }
    case MJH_STAGE_MAKE_CONSTRAINT:
      { Scope sc(run, K_CONSTRAINT); TRY(launch_constraint(m, d, s)); }
      { Scope sc(run, K_OTHER); return launch_publish(m, d, s); }
    case MJH_STAGE_TRANSMISSION: { Scope sc(run, K_POS); return launch_trn(m, d, s); }  // (hinge / slide scalar rows only: the length is produced by fwd_actuation)
    case MJH_STAGE_COM_VEL: { Scope sc(run, K_VEL); return launch_vel(m, d, VEL_COMVEL, VEL_COMVEL, s); }
    case MJH_STAGE_PASSIVE: { Scope sc(run, K_VEL); return launch_vel(m, d, VEL_PASSIVE, VEL_PASSIVE, s); }
    case MJH_STAGE_RNE: { Scope sc(run, K_VEL); return launch_vel(m, d, VEL_RNE, VEL_RNE, s); }
    case MJH_STAGE_FWD_VELOCITY: { Scope sc(run, K_VEL); return launch_vel(m, d, VEL_COMVEL, VEL_RNE, s); }
    case MJH_STAGE_FWD_ACTUATION: { Scope sc(run, K_VEL); return launch_vel(m, d, VEL_ACTUATION, VEL_ACTUATION, s); }
    case MJH_STAGE_FWD_ACCELERATION:
      { Scope sc(run, K_VEL); TRY(launch_vel(m, d, VEL_ACCEL, VEL_ACCEL, s)); }
      { Scope sc(run, K_OTHER); return launch_factor_smooth(m, d, 1, s); }
    case MJH_STAGE_SOLVE: { Scope sc(run, K_SOLVE); return launch_solve(m, d, run); }
    case MJH_STAGE_EULER: { Scope sc(run, K_INTEGRATE); return launch_integrate(m, d, 0, s); }
    case MJH_STAGE_IMPLICIT: { Scope sc(run, K_INTEGRATE); return launch_integrate(m, d, m->integrator == INT_IMPLICIT ? 2 : 1, s); }
    case MJH_STAGE_FWD_POSITION: {
      TRY(run_pos_trn(m, d, POS_FACTOR, run));
      TRY(run_collide_constrain(m, d, false, run));
      Scope sc(run, K_OTHER);
      return launch_publish(m, d, s);
    }
    case MJH_STAGE_RNE_POSTCONSTRAINT: {
      if (!d->cfrc_ext) return fail(MJH_E_ARG, "Data.cfrc_ext missing");
      Scope sc(run, K_OTHER);
      return launch_rne_postconstraint(m, d, s);
    }
    case MJH_STAGE_SUBTREE_VEL: {
      if (!d->subtree_linvel || !d->subtree_angmom) return fail(MJH_E_ARG, "Data.subtree_linvel / subtree_angmom missing");
      Scope sc(run, K_OTHER);
      return launch_subtree_vel(m, d, s);
    }
    case MJH_STAGE_ENERGY: { Scope sc(run, K_OTHER); return launch_energy(m, d, s); }
    case MJH_STAGE_SENSOR: { Scope sc(run, K_OTHER); TRY(launch_sensor(m, d, 0, run)); return launch_sensor(m, d, 1, run); }
    case MJH_STAGE_SENSOR_POSVEL: { Scope sc(run, K_OTHER); return launch_sensor(m, d, 0, run); }
    case MJH_STAGE_SENSOR_ACC: { Scope sc(run, K_OTHER); return launch_sensor(m, d, 1, run); }
    case MJH_STAGE_UPDATE_SLEEP:
    case MJH_STAGE_WAKE:
    case MJH_STAGE_WAKE_COLLISION:
    case MJH_STAGE_WAKE_EQUALITY:
    case MJH_STAGE_ISLAND:
    case MJH_STAGE_SLEEP: {
      if (!d->tree_asleep) return fail(MJH_E_ARG, "Data sleep tables missing (allocate Data with make_data/put_data)");
      const int phase = stage == MJH_STAGE_UPDATE_SLEEP ? SLP_UPDATE : stage == MJH_STAGE_WAKE ? SLP_WAKE : stage == MJH_STAGE_WAKE_COLLISION ? SLP_WAKE_COLLISION
                        : stage == MJH_STAGE_WAKE_EQUALITY ? SLP_WAKE_EQUALITY : stage == MJH_STAGE_ISLAND ? SLP_ISLAND : SLP_SLEEP;
      Scope sc(run, K_OTHER);
      return launch_sleep(m, d, phase, s);
    }
    case MJH_STAGE_RUNGEKUTTA4: {
      // forward.rungekutta4 (forward.py:524-557), called after a forward at t0: one k_rk4 launch after each evaluation
      // (accumulate + perturb; the last one restores t0 and advances); tableau A = (1/2, 1/2, 1), B = (1/6, 1/3, 1/3, 1/6)
      if (!d->ws_rk) return fail(MJH_E_ARG, "Data.ws_rk missing (allocate Data with make_data/put_data)");
      static const float A[4] = {0.5f, 0.5f, 1.0f, 0.0f}, B[4] = {1.0f / 6.0f, 1.0f / 3.0f, 1.0f / 3.0f, 1.0f / 6.0f};
      Run sub = run;
      sub.hist_insert = false;  // (history buffers: never written by a sub-evaluation)
      for (int k = 0; k < 4; ++k) {
        if (k) TRY(run_stage(m, d, MJH_STAGE_FORWARD, sub));
        Scope sc(run, K_INTEGRATE);
        hipLaunchKernelGGL(k_rk4<32>, dim3((d->nworld + 7) / 8), dim3(8 * 32), sizeof(float) * 8 * (m->nv + 1), s, *m, *d, k, A[k], B[k]);
      }
      return MJH_OK;
    }
    case MJH_STAGE_FORWARD:
    case MJH_STAGE_STEP: {
      const bool step = stage == MJH_STAGE_STEP;
      // MJH_PLAIN: developer knob, one plain kernel per stage, serial
      if (m->sleep_enabled || m->has_connect || KNOB_ONCE_FLAG("MJH_PLAIN") || (run.instr && run.instr->plain)) return run_unfused(m, d, step, m->sleep_enabled != 0, run);
      // fused step: four launches on the caller's stream (see "composite launches" above), as plan_step decides
      StepPlan p = plan_step(m, d, stage, run.instr != nullptr);
      Streams* side = p.riders == RIDE_SIDE ? side_streams(run) : nullptr;
      if (p.riders == RIDE_SIDE && !side) p = plan_step(m, d, stage, run.instr != nullptr, false);  // (a failing device: the riders go with the integrator launch)
      bool sched_done = false;
      { Scope sc(run, K_POS); TRY(launch_pos_plus(m, d, POS_KINEMATICS, POS_CRB, &sched_done, run)); }
      if (m->trn_general) {
        // k_mid's velocity-stage role is the default instantiation: such a model takes the roles as launches of their own, behind k_transmission
        { Scope sc(run, K_POS); TRY(launch_trn(m, d, s)); }
        if (!sched_done) TRY(launch_schedule(m, d, run));
        TRY(run_mid_unfused(m, d, false, run));
      } else {
        Scope sc(run, K_MID);
        TRY(launch_mid(m, d, !sched_done, s));
      }
      { Scope sc(run, K_OTHER); TRY(launch_sensor(m, d, 0, run)); }  // (no launch without sensors; before the solver, whose epilogue may integrate the state)
      if (side) {
        // (tried in round 3: forking the factor after k_fwd_pos, beside k_mid, with qacc_smooth as a separate solve after k_mid -- humanoid
        // Newton + 1.5 %, Panda - 5 %: the extra launch and the slower k_mid cost more than the shorter join wait saves)
        HIPCHK(hipEventRecord(side->fork, s));
        HIPCHK(hipStreamWaitEvent(side->stream[0], side->fork, 0));
        // both riders as roles of ONE launch (k_integrate_plus without integrator workgroups): their two chains overlap and one launch gap
        // goes (round 3, same-box A/B in two interleaved pairs against the two plain kernels of round 2: humanoid Newton 0.2842 -> 0.2829 /
        // 0.2835 -> 0.2822 ms, Panda 142.9 -> 142.0 us; the two-kernel form is retired)
        TRY(launch_integrate_plus(m, d, p.mode, false, true, side->stream[0]));
        HIPCHK(hipEventRecord(side->join[0], side->stream[0]));
      }
      { Scope sc(run, K_SOLVE); TRY(launch_solve_any(m, d, p, run)); }
      { Scope sc(run, K_OTHER); TRY(launch_sensor(m, d, 1, run)); }
      { Scope sc(run, K_INTEGRATE); TRY(launch_integrate_plus(m, d, p.mode, step && !p.fuse_euler, p.riders == RIDE_INTEGRATOR, s)); }
      if (side) HIPCHK(hipStreamWaitEvent(s, side->join[0], 0));  // every fork rejoins the caller's stream
      return MJH_OK;
    }
    default:
      return fail(MJH_E_ARG, "unknown stage");
  }
}

// Every stage goes through here.  A model with delayed actuators (MjhModel.nu_history, csrc/history.hpp) enters forward / step / fwd_actuation through
// k_history_ctrl: Data.ws_ctrl_delayed = the actuators' buffers read at Data.time (ctrl itself where there is no delay), and everything downstream
// gets a copy of MjhData whose ctrl points there (as run_unfused hands the solver its masked copies).  A step also stores (time, ctrl) in the
// buffers, once, in that launch: behind the read of the same lane, at the step's own start time.  run.hist_insert = false (the RK4 sub-evaluations:
// forward on the perturbed state) keeps every buffer read-only -- the sensors' too, see launch_sensor.
static int run_stage(const MjhModel* m, const MjhData* d, int stage, Run& run) {
  const MjhData* dc = d;  // what the stage's launches read: d, or its copy with the delayed ctrl
  MjhData delayed;
  if (m->nu_history > 0) {
    if (m->sleep_enabled) return fail(MJH_E_UNSUPPORTED, "actuator delays with sleeping enabled (the wake-by-input test reads ctrl)");
    const bool hist = run.hist_insert;
    // the integrator stages of a step taken stage by stage (step1 / step2, forward + rungekutta4): the step's ctrl sample goes in here, at its start time
    const bool integ = stage == MJH_STAGE_EULER || stage == MJH_STAGE_IMPLICIT || stage == MJH_STAGE_RUNGEKUTTA4;
    const bool fwd = stage == MJH_STAGE_FORWARD || stage == MJH_STAGE_STEP || stage == MJH_STAGE_FWD_ACTUATION;
    if (fwd) apply_noise(m, d, run);  // (k_history_ctrl reads ctrl, in front of any position launch that could carry the noise)
    // (an RK4 sub-evaluation, FORWARD with hist_insert == false: k_rk4 keeps Data.time at the step's start through all four evaluations, so the delayed
    // ctrl the first one read -- before the step's sample went in, which with a tight nsample evicted the sample read -- holds for the other three)
    if (integ || (fwd && (hist || stage != MJH_STAGE_FORWARD))) {
      Scope sc(run, K_OTHER);
      TRY(launch_history_ctrl(m, d, hist && (integ || stage == MJH_STAGE_STEP) ? 1 : 0, run.s));
    }
    // (the implicit integrators differentiate the actuator force: at the delayed ctrl.  RUNGEKUTTA4 keeps Data.ctrl: its forwards come back here)
    if (fwd || (integ && stage != MJH_STAGE_RUNGEKUTTA4)) {
      delayed = *d;
      delayed.ctrl = d->ws_ctrl_delayed;
      dc = &delayed;
    }
  }
  // a step with the RK4 integrator = forward + the RUNGEKUTTA4 stage (a sleep-enabled model goes on to run_unfused, which refuses it)
  if (stage == MJH_STAGE_STEP && m->integrator == INT_RK4 && !m->sleep_enabled) {
    TRY(run_stage_impl(m, dc, MJH_STAGE_FORWARD, run));
    return run_stage_impl(m, d, MJH_STAGE_RUNGEKUTTA4, run);
  }
  return run_stage_impl(m, dc, stage, run);
}

static int launch_solve_m(const MjhModel* m, const MjhData* d, float* x, const float* y, int mul, hipStream_t s) {
  const IntLayout lay = int_layout(m->nv, m->nC);
  TRY(launch_per_world(k_solve_m<32>, "k_solve_m: does not fit in LDS", 32, sizeof(int) * mstruct_ints(m->nv, m->nC), sizeof(float) * lay.total, d->nworld, s, *m, *d, x, y, mul));  // (see launch_factor_smooth)
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

// the C ABI is the only exported surface (the library is built with -fvisibility=hidden)
#pragma GCC visibility push(default)
extern "C" {

int mjh_abi_version(void) { return MJH_ABI_VERSION; }
int mjh_ws_ccd_floats(int nworld, int iterations, int nhfield, int npolygonmax, int nmeshdegmax, int npair, int concap, double* floats_out, int* nccdhand_out) {
  if (!floats_out || nworld < 0 || npair < 0 || concap < 0) return fail(MJH_E_ARG, "mjh_ws_ccd_floats: bad argument");
  const int ccap = collide_ccap(npair, concap), hand = ccd_handcap(nworld, ccap);
  *floats_out = (double)ccd_layout(nworld, iterations, nhfield, npolygonmax, nmeshdegmax, ccap, hand, npair).total;
  if (nccdhand_out) *nccdhand_out = hand;
  return MJH_OK;
}
const char* mjh_last_error(void) { return g_err; }
int mjh_dev_knob(const char* name, const char* value) {
  if (!name || strncmp(name, "MJH_", 4) != 0) return fail(MJH_E_ARG, "mjh_dev_knob: knob names start with MJH_");
  KnobTable& t = knobs();
  std::lock_guard<std::mutex> lock(t.mu);
  if (t.latched.count(name)) return fail(MJH_E_ARG, "mjh_dev_knob: %s is latched (read once, at its first use, which has happened): set it in the environment before the library is loaded", name);
  if (value) t.set(name, value);
  else t.kv.erase(name);
  t.n.store((int)t.kv.size(), std::memory_order_release);
  return MJH_OK;
}
const char* mjh_solver_kernel(const MjhModel* m, const MjhData* d) { return (m && d) ? solver_kernel_name(m, d) : "unsupported"; }

int mjh_stage(const MjhModel* m, const MjhData* d, int stage, void* stream) {
  TRY(check(m, d));
  Run run(stream);
  TRY(run_stage(m, d, stage, run));
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
int mjh_step(const MjhModel* m, const MjhData* d, void* stream) { return mjh_stage(m, d, MJH_STAGE_STEP, stream); }
int mjh_forward(const MjhModel* m, const MjhData* d, void* stream) { return mjh_stage(m, d, MJH_STAGE_FORWARD, stream); }

int mjh_solve_m(const MjhModel* m, const MjhData* d, float* x, const float* y, void* stream) {
  TRY(check(m, d));
  return launch_solve_m(m, d, x, y, 0, (hipStream_t)stream);
}
int mjh_mul_m(const MjhModel* m, const MjhData* d, float* res, const float* vec, void* stream) {
  TRY(check(m, d));
  return launch_solve_m(m, d, res, vec, 1, (hipStream_t)stream);
}

// ---- inverse dynamics (csrc/inverse.hpp; the kernel and its launchers are inverse_tu.hip's) ----------------------------------------------
// lanes per world of k_inverse: what k_mid / k_make_constraint choose for the model
static int inverse_lanes(const MjhModel* m) { return lanes16(m) ? 16 : (lanes64(m) ? 64 : 32); }
static const char INVERSE_SLEEP[] = "inverse dynamics with sleeping enabled (the two-pass collision and the asleep-tree shortcuts are not defined for it)";
int mjh_inv_constraint(const MjhModel* m, const MjhData* d, const float* qacc, float* qfrc_inverse, void* stream) {
  TRY(check(m, d));
  if (m->sleep_enabled) return fail(MJH_E_UNSUPPORTED, "%s", INVERSE_SLEEP);
  TRY(launch_inverse(m, d, qacc, qfrc_inverse, inverse_lanes(m), (hipStream_t)stream));
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
// inverse.inverse (inverse.py:148-182) through the stage launchers of mjh_stage: fwd_position (a model with connects: com_vel in front of its
// rows), fwd_velocity, the position / velocity sensors (one launch here, behind both stages), invdiscrete: the continuous-time acceleration,
// k_inverse, the acceleration sensors.  Data.qacc is only read: the continuous-time acceleration lives in `scratch`, where k_inverse and the
// acceleration sensors read it.
int mjh_inverse(const MjhModel* m, const MjhData* d, float* qfrc_inverse, float* scratch, void* stream) {
  TRY(check(m, d));
  if (!qfrc_inverse) return fail(MJH_E_ARG, "mjh_inverse: null qfrc_inverse");
  if (m->sleep_enabled) return fail(MJH_E_UNSUPPORTED, "%s", INVERSE_SLEEP);
  const bool discrete = (m->enableflags & ENBL_INVDISCRETE) != 0;
  if (discrete && m->integrator != INT_EULER)
    return fail(MJH_E_UNSUPPORTED, "discrete inverse dynamics (invdiscrete) with the %s integrator: only Euler is implemented",
                m->integrator == INT_RK4 ? "RK4" : (m->integrator == INT_IMPLICITFAST ? "implicitfast" : "implicit"));
  Run run(stream);
  const hipStream_t s = run.s;
  TRY(run_stage(m, d, MJH_STAGE_FWD_POSITION, run));
  TRY(run_stage(m, d, MJH_STAGE_FWD_VELOCITY, run));
  TRY(run_stage(m, d, MJH_STAGE_SENSOR_POSVEL, run));
  MjhData dq = *d;  // what k_inverse and the acceleration sensors read as qacc
  if (discrete && !(m->disableflags & (DSBL_EULERDAMP | DSBL_DAMPER)) && m->nv > 0) {
    // discrete_acc (inverse.py:79-119), Euler: qacc_c = M^-1 (M + h diag(dof_damping)) qacc = qacc + M^-1 (h dof_damping qacc)
    if (!scratch) return fail(MJH_E_ARG, "mjh_inverse: invdiscrete needs scratch [2, nworld, nv]");
    float* rhs = scratch;
    float* qacc_c = scratch + (size_t)d->nworld * m->nv;
    Scope sc(run, K_OTHER);
    TRY(launch_inverse_eulerdamp(m, d, rhs, 0, s));
    TRY(launch_solve_m(m, d, qacc_c, rhs, 0, s));
    TRY(launch_inverse_eulerdamp(m, d, qacc_c, 1, s));
    dq.qacc = qacc_c;
  }
  { Scope sc(run, K_SOLVE); TRY(launch_inverse(m, &dq, dq.qacc, qfrc_inverse, inverse_lanes(m), s)); }
  TRY(run_stage(m, &dq, MJH_STAGE_SENSOR_ACC, run));
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

int mjh_qld_dense(const MjhModel* m, const MjhData* d, float* qld_dense, int stride, void* stream) {
  TRY(check(m, d));
  if (!qld_dense || stride < 0) return fail(MJH_E_ARG, "mjh_qld_dense: null output");
  if (m->ntree == 0 || d->nworld == 0) return MJH_OK;
  hipLaunchKernelGGL(k_qld_dense, dim3(d->nworld * m->ntree), dim3(64), 0, (hipStream_t)stream, *m, *d, qld_dense, stride);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

int mjh_contact_force(const MjhModel* m, const MjhData* d, const int* contact_ids, int n, int to_world_frame, float* force, void* stream) {
  TRY(check(m, d));
  if (n < 0 || (n > 0 && (!contact_ids || !force))) return fail(MJH_E_ARG, "mjh_contact_force: null argument");
  if (n == 0) return MJH_OK;
  hipLaunchKernelGGL(k_contact_force, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *m, *d, contact_ids, n, to_world_frame, force);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

int mjh_jac(const MjhModel* m, const MjhData* d, float* jacp, float* jacr, const float* point, const int* body, void* stream) {
  TRY(check(m, d));
  if (!point || !body) return fail(MJH_E_ARG, "mjh_jac: null point / body");
  if (m->nv == 0 || (!jacp && !jacr)) return MJH_OK;
  hipLaunchKernelGGL(k_jac, dim3((d->nworld * m->nv + 255) / 256), dim3(256), 0, (hipStream_t)stream, *m, *d, jacp, jacr, point, body);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

int mjh_rays(const MjhModel* m, const MjhData* d, const float* pnt, const float* vec, int pnt_nworld, int nray, const float* geomgroup, int flg_static,
             const int* bodyexclude, float* dist, int* geomid, float* normal, void* stream) {
  TRY(check(m, d));
  if (!pnt || !vec || !dist) return fail(MJH_E_ARG, "mjh_rays: null pnt / vec / dist");
  if (nray < 0 || (pnt_nworld != 1 && pnt_nworld != d->nworld)) return fail(MJH_E_ARG, "mjh_rays: pnt_nworld must be 1 or nworld");
  if (nray == 0) return MJH_OK;
  if ((long long)d->nworld * nray > 0x7fffffffLL) return fail(MJH_E_ARG, "mjh_rays: nworld * nray exceeds 2^31 - 1 (cast the rays in several calls)");
  RayGroup gg;
  for (int i = 0; i < 6; ++i) gg.g[i] = geomgroup ? geomgroup[i] : -1.0f;
  // the model decides, not the caller (csrc/ray.hpp): primitive-only -> k_rays, untouched; meshes of few triangles (at most RAY_GROUP_MIN_FACES
  // per mesh on average) and no height field -> the same one-thread walk over ray_world_full; otherwise a lane group per ray
  const long long nr = (long long)d->nworld * nray;
  if (m->nhfield > 0 || (long long)m->nmeshface > (long long)RAY_GROUP_MIN_FACES * m->nmesh) {
    constexpr int per_block = 256 / RAY_LANES;
    hipLaunchKernelGGL(k_rays_group, dim3((unsigned)((nr + per_block - 1) / per_block)), dim3(256), 0, (hipStream_t)stream, *m, *d, pnt, vec, pnt_nworld, nray, gg, flg_static,
                       bodyexclude, dist, geomid, normal);
  } else if (m->nmeshface > 0)
    hipLaunchKernelGGL(k_rays_serial_full, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *m, *d, pnt, vec, pnt_nworld, nray, gg, flg_static, bodyexclude,
                       dist, geomid, normal);
  else
    hipLaunchKernelGGL(k_rays, dim3((d->nworld * nray + 255) / 256), dim3(256), 0, (hipStream_t)stream, *m, *d, pnt, vec, pnt_nworld, nray, gg, flg_static, bodyexclude, dist,
                       geomid, normal);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

// the cameras (csrc/render.hpp; the kernels are render_tu.hip's)
static int check_render(const char* who, const MjhModel* m, const MjhData* d, const MjhRender* rc) {
  if (!rc) return fail(MJH_E_ARG, "%s: null render context", who);
  if (rc->nworld != d->nworld) return fail(MJH_E_ARG, "%s: the render context was built for another nworld", who);
  if (rc->ncam < 0 || rc->npixel < 0 || rc->ntile < 0) return fail(MJH_E_ARG, "%s: negative size in the render context", who);
  if (rc->ncam == 0 || rc->npixel == 0) return MJH_OK;
  if (!rc->cam_bodyid || !rc->cam_pos || !rc->cam_quat || !rc->cam_res || !rc->cam_exclude || !rc->depth_adr || !rc->seg_adr || !rc->tile || !rc->ray || !rc->cam_xpos || !rc->cam_xmat)
    return fail(MJH_E_ARG, "%s: null table in the render context", who);
  if (rc->ntile == 0 || (long long)rc->ntile * 64 < rc->npixel) return fail(MJH_E_ARG, "%s: the tile table does not cover the pixels", who);
  if ((long long)d->nworld * rc->npixel > 0x7fffffffLL) return fail(MJH_E_ARG, "%s: nworld * npixel exceeds 2^31 - 1 (render fewer worlds or cameras per context)", who);
  if (!d->xpos || !d->xmat || !d->geom_xpos || !d->geom_xmat || (m->ngeom > 0 && !m->geom_rbound)) return fail(MJH_E_ARG, "%s: Data.xpos / xmat / geom_xpos / geom_xmat or Model.geom_rbound missing", who);
  return MJH_OK;
}
int mjh_render(const MjhModel* m, const MjhData* d, const MjhRender* rc, void* stream) {
  TRY(check(m, d));
  TRY(check_render("mjh_render", m, d, rc));
  if (rc->ncam == 0 || rc->npixel == 0) return MJH_OK;
  if (!rc->depth && !rc->seg && !rc->normal) return fail(MJH_E_ARG, "mjh_render: no output buffer (depth, seg and normal are all null)");
  return launch_render(m, d, rc, (hipStream_t)stream);
}
int mjh_camera_rays(const MjhModel* m, const MjhData* d, const MjhRender* rc, float* pnt, float* vec, void* stream) {
  TRY(check(m, d));
  TRY(check_render("mjh_camera_rays", m, d, rc));
  if (rc->ncam == 0 || rc->npixel == 0) return MJH_OK;
  if (!pnt || !vec) return fail(MJH_E_ARG, "mjh_camera_rays: null pnt / vec");
  return launch_camera_rays(m, d, rc, pnt, vec, (hipStream_t)stream);
}

int mjh_efc_j_sparse(const MjhModel* m, const MjhData* d, int njmax_nnz, int* rownnz, int* rowadr, int* colind, float* values, void* stream) {
  TRY(check(m, d));
  if (njmax_nnz < 0 || !rownnz || !rowadr || (njmax_nnz > 0 && (!colind || !values))) return fail(MJH_E_ARG, "mjh_efc_j_sparse: null output or negative njmax_nnz");
  hipLaunchKernelGGL(k_efc_j_sparse, dim3(d->nworld), dim3(64), 0, (hipStream_t)stream, *d, m->nv, njmax_nnz, rownnz, rowadr, colind, values);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

int mjh_ctrl_noise(const MjhModel* m, const MjhData* d, const float* ctrl_center, int step, float noise_std, float noise_rate, void* stream) {
  TRY(check(m, d));
  Run run(stream);
  run.noise = NoiseArgs{d->nworld * m->nu, step, noise_std, noise_rate, ctrl_center, 0};
  apply_noise(m, d, run);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

int mjh_release_thread_resources(void) {
  // the calling thread's side streams and events (one set per device it stepped a Newton or per-island model on)
  int rc = MJH_OK;
  for (int dev = 0; dev < 16; ++dev) {
    Streams* a = g_streams_per_dev[dev];
    if (!a) continue;
    g_streams_per_dev[dev] = nullptr;
    for (int k = 0; k < a->n; ++k) {
      if (hipStreamSynchronize(a->stream[k]) != hipSuccess) rc = MJH_E_LAUNCH;
      if (hipEventDestroy(a->join[k]) != hipSuccess) rc = MJH_E_LAUNCH;
      if (hipStreamDestroy(a->stream[k]) != hipSuccess) rc = MJH_E_LAUNCH;
    }
    if (hipEventDestroy(a->fork) != hipSuccess) rc = MJH_E_LAUNCH;
    delete a;
  }
  return rc == MJH_OK ? MJH_OK : fail(rc, "mjh_release_thread_resources: %s", "a HIP call failed");
}

// the graph of one step; reset != nullptr: with k_reset in front of it, on the same stream (one more node of the linear chain, no branch)
static int graph_create(const MjhModel* m, const MjhData* d, const MjhReset* reset, void* stream, void** graph_exec_out) {
  TRY(check(m, d));
  Run run(stream);
  const hipStream_t s = run.s;
  // warm the kernels (function attributes must be set outside capture)
  TRY(run_stage(m, d, MJH_STAGE_STEP, run));
  HIPCHK(hipStreamSynchronize(s));
  hipGraph_t graph;
  HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  int rc = reset ? launch_reset(m, d, reset, s) : MJH_OK;  // (k_reset sets no kernel attribute: nothing to warm)
  if (rc == MJH_OK) rc = run_stage(m, d, MJH_STAGE_STEP, run);
  hipError_t e = hipStreamEndCapture(s, &graph);  // always end the capture so the stream stays usable
  if (rc != MJH_OK) return rc;
  HIPCHK(e);
  hipGraphExec_t exec;
  HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  hipGraphDestroy(graph);
  *graph_exec_out = (void*)exec;
  return MJH_OK;
}
int mjh_graph_create(const MjhModel* m, const MjhData* d, void* stream, void** graph_exec_out) { return graph_create(m, d, nullptr, stream, graph_exec_out); }
int mjh_graph_create_reset(const MjhModel* m, const MjhData* d, const MjhReset* r, void* stream, void** graph_exec_out) {
  if (!r) return fail(MJH_E_ARG, "mjh_graph_create_reset: null reset arguments");
  return graph_create(m, d, r, stream, graph_exec_out);
}
int mjh_graph_launch(void* graph_exec, void* stream) {
  HIPCHK(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
  return MJH_OK;
}
int mjh_graph_destroy(void* graph_exec) {
  HIPCHK(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
  return MJH_OK;
}

int mjh_timed_steps(const MjhModel* m, const MjhData* d, int nstep, int step0, float noise_std, float noise_rate,
                    void* stream, float* ms_out, float* per_kernel_ms, int plain_kernels) {
  TRY(check(m, d));
  Instr instr;
  instr.plain = plain_kernels != 0;
  Run run(stream);
  if (per_kernel_ms) run.instr = &instr;
  const hipStream_t s = run.s;
  struct Event {  // (destroyed on every way out)
    hipEvent_t e = nullptr;
    ~Event() {
      if (e) hipEventDestroy(e);
    }
  } t0, t1;
  HIPCHK(hipEventCreate(&t0.e));
  HIPCHK(hipEventCreate(&t1.e));
  HIPCHK(hipEventRecord(t0.e, s));
  int rc = MJH_OK;
  for (int i = 0; i < nstep && rc == MJH_OK; ++i) {
    // the noise of step i is pending in the context (see Run::noise); the per-kernel profiling passes and the plain path keep it as its own kernel
    const bool plain_env = KNOB_ONCE_FLAG("MJH_PLAIN") || KNOB_ONCE_FLAG("MJH_NO_NOISE_FUSION");
    if (noise_std >= 0.0f && m->nu > 0) run.noise = NoiseArgs{d->nworld * m->nu, step0 + i, noise_std, noise_rate, nullptr, 0};
    if (run.instr || plain_env) apply_noise(m, d, run);
    rc = run_stage(m, d, MJH_STAGE_STEP, run);
  }
  hipError_t e = hipEventRecord(t1.e, s);
  if (e == hipSuccess) e = hipEventSynchronize(t1.e);
  if (e == hipSuccess) e = instr.err;
  float ms = 0.0f;
  hipEventElapsedTime(&ms, t0.e, t1.e);
  if (ms_out) *ms_out = ms;
  if (per_kernel_ms) {
    for (int k = 0; k < MJH_NKERNEL; ++k) per_kernel_ms[k] = 0.0f;
    for (size_t i = 0; i < instr.cls.size(); ++i) {
      float t = 0.0f;
      hipEventElapsedTime(&t, instr.ev[2 * i], instr.ev[2 * i + 1]);
      per_kernel_ms[instr.cls[i]] += t;
      hipEventDestroy(instr.ev[2 * i]);
      hipEventDestroy(instr.ev[2 * i + 1]);
    }
  }
  if (rc != MJH_OK) return rc;
  HIPCHK(e);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

}  // extern "C"
#pragma GCC visibility pop

MJH_DEFINE_PHASE_TICKS  // (host.hpp)
