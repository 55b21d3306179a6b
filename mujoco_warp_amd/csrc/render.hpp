// Batched depth / segmentation cameras (reference render.py, render_util.py): render() and camera_rays() of the public API.
// Every pixel reports the hit rays() would report for its ray -- the intersection functions are ray.hpp's, unchanged, and the winner is
// ray_hit_before's (distance, geom, sub) minimum -- but the rays of an image are not independent: the 64 pixels of an 8 x 8 tile see almost
// the same few geoms.  One wavefront takes one tile of one (world, camera); a 256-thread workgroup holds four tiles.
//   Cull: the lanes take the world's geoms 64 at a time.  Each lane runs ray_eliminate for its geom and tests the geom's bounding sphere
//     (geom_xpos, geom_rbound) against the tile's cone; a ballot compacts the survivors into the wavefront's LDS list (type, geom, pos, mat,
//     size: RENDER_ENTRY words), primitives from the front, meshes and height fields from the back.
//   Primitives: every lane casts its own pixel ray against the front list (ray_geom).
//   Meshes: every lane applies ray_mesh_cull for its ray; the tile then walks the triangles together, every lane testing the same triangle
//     for its own ray, so a triangle is fetched once per tile.  Height fields: ray_hfield with the lane as a group of one.
// Pixels past the image edge (a partial tile) are masked, not skipped: their lanes cast the nearest edge pixel's ray and write nothing.
// No BVH: the tile cull is the acceleration structure.
#pragma once
#include "ray.hpp"

constexpr int RENDER_TILE = 8;     // tile edge in pixels: RENDER_TILE^2 = one wavefront
constexpr int RENDER_ENTRY = 17;   // words of a list entry: type, geom, pos[3], mat[9], size[3]
constexpr int RENDER_TILES_PER_BLOCK = 4;
constexpr int RENDER_OBJ_GEOM = 5;  // mjOBJ_GEOM: the object type segmentation reports

// world frames of the cameras: cam_xpos = xpos[b] + xmat[b] cam_pos, cam_xmat = xmat[b] R(cam_quat)
__global__ void __launch_bounds__(256) k_render_cams(MjhModel m, MjhData d, MjhRender rc) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= d.nworld * rc.ncam) return;
  const int w = idx / rc.ncam, c = idx - w * rc.ncam, b = rc.cam_bodyid[c];
  const float* xm = d.xmat + ((size_t)w * m.nbody + b) * 9;
  st3(rc.cam_xpos + (size_t)idx * 3, ld3(d.xpos + ((size_t)w * m.nbody + b) * 3) + mat_mul(xm, ld3(rc.cam_pos + 3 * c)));
  float R[9];
  quat_to_mat(ld4(rc.cam_quat + 4 * c), R);
  float* out = rc.cam_xmat + (size_t)idx * 9;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = xm[3 * i] * R[j] + xm[3 * i + 1] * R[3 + j] + xm[3 * i + 2] * R[6 + j];
}

// world-frame direction of a pixel ray.  Not inlined: render and camera_rays must produce the same float32 bits, whatever the compiler
// would do with the nine products in either caller (a 1-ulp difference flips silhouette pixels against rays() on camera_rays' output)
__device__ __noinline__ V3 render_ray_dir(const float* cam_xmat, const float* ray_cam) { return mat_mul(cam_xmat, ld3(ray_cam)); }

__global__ void __launch_bounds__(256) k_camera_rays(MjhData d, MjhRender rc, float* pnt, float* vec) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)d.nworld * rc.npixel) return;
  const int w = (int)(idx / rc.npixel), p = (int)(idx - (long long)w * rc.npixel);
  int c = 0;
  while (c + 1 < rc.ncam && rc.depth_adr[c + 1] <= p) ++c;
  st3(pnt + idx * 3, ld3(rc.cam_xpos + ((size_t)w * rc.ncam + c) * 3));
  st3(vec + idx * 3, render_ray_dir(rc.cam_xmat + ((size_t)w * rc.ncam + c) * 9, rc.ray + (size_t)p * 3));
}

// may a ray from `o` inside the cone (unit axis a, cos / sin of the half angle ct / st, below 90 degrees) touch the sphere (c, r)?  With
// v = c - o, beta the angle between a and v: the sphere's angular radius is asin(r / |v|), so it meets the cone when sin(beta - theta) <= r / |v|
// (and beta - theta <= 90 degrees), or when it contains o.  Everything is kept multiplied by |v|; the margin covers the float32 rounding of
// the test itself (a few operations on terms of at most |c| + |o|: below 1e-6 of that), so the cull never drops a hit
DEV bool render_cone_sphere(V3 o, V3 a, float ct, float st, V3 c, float r) {
  const V3 v = c - o;
  const float margin = 1e-5f * (fabsf(c.x) + fabsf(c.y) + fabsf(c.z) + fabsf(o.x) + fabsf(o.y) + fabsf(o.z) + r) + 1e-9f;
  const float rr = r + margin;
  if (dot(v, v) <= rr * rr) return true;
  const float av = dot(a, v), xv = length(cross(a, v));
  return av * ct + xv * st >= 0.0f && xv * ct - av * st <= rr;
}

// mesh geom g against the rays of a tile: ray_mesh's walk (ray.hpp) with every lane on the same triangle.  `skip`: this lane's ray misses
// the mesh's box (ray_mesh_cull) or the lane has nothing to add; such a lane still walks along (the loop is wave-uniform)
DEV void render_mesh_tile(const MjhModel& m, int g, const float* mat, V3 pos, V3 pnt, V3 vec, bool skip, RayHit& h) {
  const int id = m.geom_dataid[g];
  if (id < 0 || id >= m.nmesh || m.nmeshface == 0) return;
  const V3 lp = matT_mul(mat, pnt - pos), lv = matT_mul(mat, vec);
  V3 b0, b1;
  ray_basis(normalize(lv), b0, b1);
  const float* vert = m.mesh_vert + 3 * (size_t)m.mesh_vertadr[id];
  const int f0 = m.mesh_faceadr[id], f1 = id + 1 < m.nmesh ? m.mesh_faceadr[id + 1] : m.nmeshface;
  bool took = false;
  for (int f = f0; f < f1; ++f) {
    const int* fv = m.mesh_face + 3 * (size_t)f;
    const V3 v0 = ld3(vert + 3 * fv[0]), v1 = ld3(vert + 3 * fv[1]), v2 = ld3(vert + 3 * fv[2]);
    if (skip) continue;
    V3 n;
    const float x = ray_triangle(v0, v1, v2, lp, lv, b0, b1, n);
    if (x >= 0.0f && x < MJ_MAXVAL && ray_hit_before(x, g, f - f0, h)) {
      h = RayHit{x, g, f - f0, n};
      took = true;
    }
  }
  if (took) h.n = mat_mul(mat, h.n);
}

__global__ void __launch_bounds__(64 * RENDER_TILES_PER_BLOCK) k_render(MjhModel m, MjhData d, MjhRender rc) {
  __shared__ float lds[RENDER_TILES_PER_BLOCK][64 * RENDER_ENTRY];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long q = (long long)blockIdx.x * RENDER_TILES_PER_BLOCK + wave;
  if (q >= (long long)d.nworld * rc.ntile) return;  // (whole wavefronts leave; no workgroup barrier below)
  // neighbouring wavefronts: the same tile in neighbouring worlds (they walk the same model-constant triangles)
  const int t = (int)(q / d.nworld), w = (int)(q - (long long)t * d.nworld);
  const int c = rc.tile[3 * t], width = rc.cam_res[2 * c], height = rc.cam_res[2 * c + 1];
  const int px = rc.tile[3 * t + 1] + (lane & (RENDER_TILE - 1)), py = rc.tile[3 * t + 2] + (lane >> 3);
  const bool valid = px < width && py < height;
  const int pix = min(py, height - 1) * width + min(px, width - 1);  // (a masked lane casts the nearest edge pixel's ray)
  const float* ray_cam = rc.ray + ((size_t)rc.depth_adr[c] + pix) * 3;
  const V3 o = ld3(rc.cam_xpos + ((size_t)w * rc.ncam + c) * 3);
  const V3 vec = render_ray_dir(rc.cam_xmat + ((size_t)w * rc.ncam + c) * 9, ray_cam);
  // the tile's cone: axis = the mean direction, half angle = the largest angle of a pixel ray to it (a corner pixel's)
  V3 a = vec;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a = a + V3{__shfl_xor(a.x, off, 64), __shfl_xor(a.y, off, 64), __shfl_xor(a.z, off, 64)};
  a = normalize(V3{__shfl(a.x, 0, 64), __shfl(a.y, 0, 64), __shfl(a.z, 0, 64)});  // (one lane's sum: the butterfly's order of additions differs between lanes)
  float st = length(cross(a, vec)) / fmaxf(length(vec), MJ_MINVAL), ct = dot(a, vec);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    st = fmaxf(st, __shfl_xor(st, off, 64));
    ct = fminf(ct, __shfl_xor(ct, off, 64));
  }
  const bool no_cone = !(ct > 0.0f);  // 90 degrees or more (or a degenerate axis): nothing is culled by the cone
  st = fminf(st * (1.0f + 1e-5f) + 1e-7f, 1.0f);
  ct = sqrtf(fmaxf(0.0f, 1.0f - st * st));
  RayGroup gg;
  for (int i = 0; i < 6; ++i) gg.g[i] = (rc.groupmask >> i) & 1 ? 1.0f : 0.0f;
  const int ex = rc.cam_exclude[c];
  float* list = lds[wave];
  RayHit h = RayHit{MJ_MAXVAL, -1, 0, V3{0, 0, 0}};
  for (int g0 = 0; g0 < m.ngeom; g0 += 64) {
    const int g = g0 + lane;
    bool keep = false, shared = false;
    int type = -1;
    V3 pos = V3{0, 0, 0};
    if (g < m.ngeom && !ray_eliminate(m, g, gg, 1, ex)) {
      type = m.geom_type[g];
      pos = ld3(d.geom_xpos + ((size_t)w * m.ngeom + g) * 3);
      shared = type == G_MESH || type == G_HFIELD;
      keep = type == G_PLANE || type == G_HFIELD || no_cone || render_cone_sphere(o, a, ct, st, pos, BF(m, geom_rbound, w)[g]);
    }
    const unsigned long long kp = __ballot(keep && !shared), ks = __ballot(keep && shared), below = (1ull << lane) - 1ull;
    const int nprim = __popcll(kp), nshared = __popcll(ks);
    if (keep) {
      float* e = list + RENDER_ENTRY * (shared ? 63 - __popcll(ks & below) : __popcll(kp & below));
      const float* mat = d.geom_xmat + ((size_t)w * m.ngeom + g) * 9;
      const float* size = BF(m, geom_size, w) + 3 * g;
      e[0] = __int_as_float(type);
      e[1] = __int_as_float(g);
      st3(e + 2, pos);
      for (int i = 0; i < 9; ++i) e[5 + i] = mat[i];
      st3(e + 14, ld3(size));
    }
    gsync();
    for (int i = 0; i < nprim; ++i) {
      const float* e = list + RENDER_ENTRY * i;
      V3 n;
      const float x = ray_geom(__float_as_int(e[0]), ld3(e + 2), e + 5, ld3(e + 14), o, vec, n);
      ray_hit_take(h, x, __float_as_int(e[1]), 0, n);
    }
    for (int i = 0; i < nshared; ++i) {
      const float* e = list + RENDER_ENTRY * (63 - i);
      const int gs = __float_as_int(e[1]);
      const V3 pos_s = ld3(e + 2);
      float mat[9];
      for (int k = 0; k < 9; ++k) mat[k] = e[5 + k];
      if (__float_as_int(e[0]) == G_MESH) {
        const bool skip = ray_mesh_cull(m, w, gs, pos_s, mat, o, vec);
        if (__ballot(!skip) != 0ull) render_mesh_tile(m, gs, mat, pos_s, o, vec, skip, h);
      } else {
        ray_hfield(m, gs, pos_s, mat, o, vec, 0, 1, h);
      }
    }
    gsync();  // (the next chunk overwrites the list)
  }
  if (!valid) return;
  const size_t out = (size_t)w * rc.npixel + rc.depth_adr[c] + pix;
  const bool hit = h.geom >= 0 && h.dist < MJ_MAXVAL;
  if (rc.depth) rc.depth[out] = hit ? h.dist * -ray_cam[2] : 0.0f;
  if (rc.seg) {
    int* s = rc.seg + ((size_t)w * rc.npixel + rc.seg_adr[c] + pix) * 2;
    s[0] = hit ? h.geom : -1;
    s[1] = hit ? RENDER_OBJ_GEOM : -1;
  }
  if (rc.normal) st3(rc.normal + out * 3, hit ? h.n : V3{0, 0, 0});
}
