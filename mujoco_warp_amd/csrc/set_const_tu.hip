// set_const_tu.hip -- k_set_const and its entry point mjh_set_const (one translation unit of libmjhip.so, see host.hpp): the derived model
// constants are recomputed off the step path and touch no step kernel.  Built WITHOUT the fast-division flags: the inverse weights are
// quotients and the kinematics take square roots, both correctly rounded here.
#include "host.hpp"

#include "set_const.hpp"

#pragma GCC visibility push(default)
extern "C" int mjh_set_const(const MjhModel* m, int nbatch, float* body_subtreemass, float* dof_invweight0, float* body_invweight0, float* stat_meaninertia,
                             int what, void* stream) {
  if (!m) return fail(MJH_E_ARG, "mjh_set_const: null model");
  if (nbatch < 1) return fail(MJH_E_ARG, "mjh_set_const: nbatch must be at least 1");
  if (what & ~(MJH_SET_CONST_FIXED | MJH_SET_CONST_0)) return fail(MJH_E_ARG, "mjh_set_const: unknown bit in `what`");
  if (m->nbody < 1 || m->nv < 0) return fail(MJH_E_ARG, "mjh_set_const: bad model sizes");
  if (!(what & MJH_SET_CONST_FIXED)) body_subtreemass = nullptr;
  if (!(what & MJH_SET_CONST_0)) dof_invweight0 = body_invweight0 = stat_meaninertia = nullptr;
  if (!body_subtreemass && !dof_invweight0 && !body_invweight0 && !stat_meaninertia) return MJH_OK;  // nothing requested
  const struct { const char* name; int nb; } in[] = {
      {"body_mass", m->body_mass_nb},       {"body_inertia", m->body_inertia_nb}, {"body_ipos", m->body_ipos_nb}, {"body_iquat", m->body_iquat_nb},
      {"body_pos", m->body_pos_nb},         {"body_quat", m->body_quat_nb},       {"jnt_pos", m->jnt_pos_nb},     {"jnt_axis", m->jnt_axis_nb},
      {"dof_armature", m->dof_armature_nb}, {"qpos0", m->qpos0_nb}};
  for (const auto& f : in)  // (world w reads row w % nb: a row count other than 1 and nbatch would pair rows with the wrong outputs)
    if (f.nb > 1 && f.nb != nbatch) return fail(MJH_E_ARG, "mjh_set_const: the leading dimension of %s is neither 1 nor nbatch", f.name);
  const SetConstLayout sl = set_const_layout(m->nq, m->nv, m->nbody, m->njnt, m->nC, m->tree_nvmax);
  const size_t lds = (size_t)sl.total * sizeof(float);
  if (lds > (size_t)kLdsPerCU) return fail(MJH_E_UNSUPPORTED, "mjh_set_const: the model's working set does not fit the 160 KiB of LDS");
  HIPCHK(set_lds(k_set_const, lds));
  hipLaunchKernelGGL(k_set_const, dim3(nbatch), dim3(64), lds, (hipStream_t)stream, *m, body_subtreemass, dof_invweight0, body_invweight0, stat_meaninertia, what);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
#pragma GCC visibility pop
