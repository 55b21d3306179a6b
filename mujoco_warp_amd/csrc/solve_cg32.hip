// solve_cg32.hip -- k_solve_plus instantiations: CG, 32 lanes per world (one translation unit of libmjhip.so, see host.hpp)
#include "solve_tu.hpp"

int launch_solve_32_cg(const MjhModel* m, const MjhData* d, int nr, bool with_factor, int fuse_euler, hipStream_t s, int lo, int hi) {
  switch (nr) {
    case 2: return launch_solve_32<2, false>(m, d, with_factor, fuse_euler, s, lo, hi);
    case 6: return launch_solve_32<6, false>(m, d, with_factor, fuse_euler, s, lo, hi);
    default: return fail(MJH_E_ARG, "k_solve: unsupported rows per lane");
  }
}

// the worlds the pooled CG kernel flagged (solver_cgp.hpp): k_solve<cg>'s body, two rows per lane
int launch_solve_32_cg_deferred(const MjhModel* m, const MjhData* d, int fuse_euler, hipStream_t s) {
  return dispatch_nv4_32((m->nv + 3) / 4, [&](auto NV4) { return launch_solve_deferred_t<NV4(), 2, false, 32>(m, d, fuse_euler, s); });
}

MJH_DEFINE_PHASE_TICKS  // (host.hpp)
