// render_tu.hip -- k_render_cams, k_render, k_camera_rays (one translation unit of libmjhip.so, see host.hpp): the cameras touch no step kernel
#include "host.hpp"

#define MJH_RAY_NO_KERNELS  // (k_rays* live in mjhip.hip)
#include "render.hpp"

static void launch_render_cams(const MjhModel* m, const MjhData* d, const MjhRender* rc, hipStream_t s) {
  hipLaunchKernelGGL(k_render_cams, dim3((d->nworld * rc->ncam + 255) / 256), dim3(256), 0, s, *m, *d, *rc);
}
int launch_render(const MjhModel* m, const MjhData* d, const MjhRender* rc, hipStream_t s) {
  launch_render_cams(m, d, rc, s);
  const long long ntile = (long long)d->nworld * rc->ntile;
  hipLaunchKernelGGL(k_render, dim3((unsigned)((ntile + RENDER_TILES_PER_BLOCK - 1) / RENDER_TILES_PER_BLOCK)), dim3(64 * RENDER_TILES_PER_BLOCK), 0, s, *m, *d, *rc);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
int launch_camera_rays(const MjhModel* m, const MjhData* d, const MjhRender* rc, float* pnt, float* vec, hipStream_t s) {
  launch_render_cams(m, d, rc, s);
  const long long n = (long long)d->nworld * rc->npixel;
  hipLaunchKernelGGL(k_camera_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *d, *rc, pnt, vec);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
