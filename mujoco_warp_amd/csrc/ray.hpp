// Ray casting (reference ray.py): ray() / rays() of the public API and the rangefinder sensor.
// Primitive-only models: one thread per (world, ray) walks the world's geoms (k_rays) -- a model has tens of them and a caller of rays()
// brings hundreds of rays per world, so the rays are the parallel axis (the reference spends a block per ray and its threads on the geoms).
// Models with a height field or with large meshes: a group of RAY_LANES lanes per (world, ray) (k_rays_group) strides over the geoms, then
// over the triangles of every mesh that survives the box cull and over the cells of every height field; one lexicographic
// (distance, geom, triangle) min-reduction picks the winner the serial walk (ray_world_full, the rangefinder's path) would pick.
// Models whose meshes have few triangles each: one thread per (world, ray) over that serial walk (k_rays_serial_full), which measured faster there.
// No BVH; the cameras (render.hpp) cast their pixel rays with the device functions below.
#pragma once
#include "dev_common.hpp"

// smallest non-negative root of a x^2 + 2 b x + c = 0 (ray.py:105-125 _ray_quad); both roots in x0, x1 (-1 when there is none)
DEV float ray_quad(float a, float b, float c, float& x0, float& x1) {
  x0 = x1 = -1.0f;
  float det = b * b - a * c;
  if (det < MJ_MINVAL) return -1.0f;
  det = sqrtf(det);
  const float den = safe_div(1.0f, a);
  x0 = (-b - det) * den;
  x1 = (-b + det) * den;
  return x0 >= 0.0f ? x0 : (x1 >= 0.0f ? x1 : -1.0f);
}
DEV float ray_sphere(V3 pos, float dist_sqr, V3 pnt, V3 vec, V3& normal) {  // ray.py:237-251
  const V3 dif = pnt - pos;
  float x0, x1;
  const float sol = ray_quad(dot(vec, vec), dot(vec, dif), dot(dif, dif) - dist_sqr, x0, x1);
  normal = sol >= 0.0f ? normalize(pnt + vec * sol - pos) : V3{0, 0, 0};
  return sol;
}
DEV float ray_plane(V3 pos, const float* mat, V3 size, V3 pnt, V3 vec, V3& normal) {  // ray.py:213-234: front face only, inside the rendered rectangle
  normal = V3{0, 0, 0};
  const V3 lp = matT_mul(mat, pnt - pos), lv = matT_mul(mat, vec);
  if (lv.z > -MJ_MINVAL) return -1.0f;
  const float x = -lp.z / lv.z;
  if (x < 0.0f) return -1.0f;
  const float px = lp.x + x * lv.x, py = lp.y + x * lv.y;
  if ((size.x <= 0.0f || fabsf(px) <= size.x) && (size.y <= 0.0f || fabsf(py) <= size.y)) {
    normal = V3{mat[2], mat[5], mat[8]};
    return x;
  }
  return -1.0f;
}
DEV float ray_capsule(V3 pos, const float* mat, V3 size, V3 pnt, V3 vec, V3& normal) {  // ray.py:254-325
  const float ssz = size.x + size.y;
  if (ray_sphere(pos, ssz * ssz, pnt, vec, normal) < 0.0f) {
    normal = V3{0, 0, 0};
    return -1.0f;
  }
  const V3 lp = matT_mul(mat, pnt - pos), lv = matT_mul(mat, vec);
  float x = -1.0f, x0, x1;
  const float r2 = size.x * size.x;
  float a = lv.x * lv.x + lv.y * lv.y;
  float sol = ray_quad(a, lv.x * lp.x + lv.y * lp.y, lp.x * lp.x + lp.y * lp.y - r2, x0, x1);
  int part = 0;  // -1 bottom cap, 0 side, 1 top cap
  if (sol >= 0.0f && fabsf(lp.z + sol * lv.z) <= size.y) x = sol;
  a += lv.z * lv.z;
  for (int cap = 1; cap >= -1; cap -= 2) {  // top first, then bottom: only the outer half of each sphere
    const V3 ld = V3{lp.x, lp.y, lp.z - (float)cap * size.y};
    ray_quad(a, dot(lv, ld), dot(ld, ld) - r2, x0, x1);
    for (int i = 0; i < 2; ++i) {
      const float xi = i ? x1 : x0;
      if (xi >= 0.0f && (float)cap * (lp.z + xi * lv.z) >= size.y && (x < 0.0f || xi < x)) {
        x = xi;
        part = cap;
      }
    }
  }
  normal = V3{0, 0, 0};
  if (x >= 0.0f) {
    const V3 n = V3{lp.x + lv.x * x, lp.y + lv.y * x, part == 0 ? 0.0f : lp.z + lv.z * x - size.y * (float)part};
    normal = mat_mul(mat, normalize(n));
  }
  return x;
}
DEV float ray_ellipsoid(V3 pos, const float* mat, V3 size, V3 pnt, V3 vec, V3& normal) {  // ray.py:328-356
  const V3 lp = matT_mul(mat, pnt - pos), lv = matT_mul(mat, vec);
  const V3 s = V3{safe_div(1.0f, size.x * size.x), safe_div(1.0f, size.y * size.y), safe_div(1.0f, size.z * size.z)};
  const V3 slv = V3{s.x * lv.x, s.y * lv.y, s.z * lv.z}, slp = V3{s.x * lp.x, s.y * lp.y, s.z * lp.z};
  float x0, x1;
  const float sol = ray_quad(dot(slv, lv), dot(slv, lp), dot(slp, lp) - 1.0f, x0, x1);
  normal = V3{0, 0, 0};
  if (sol >= 0.0f) {
    const V3 l = lp + lv * sol;
    normal = mat_mul(mat, normalize(V3{s.x * l.x, s.y * l.y, s.z * l.z}));
  }
  return sol;
}
DEV float ray_cylinder(V3 pos, const float* mat, V3 size, V3 pnt, V3 vec, V3& normal) {  // ray.py:359-417
  if (ray_sphere(pos, size.x * size.x + size.y * size.y, pnt, vec, normal) < 0.0f) {
    normal = V3{0, 0, 0};
    return -1.0f;
  }
  const V3 lp = matT_mul(mat, pnt - pos), lv = matT_mul(mat, vec);
  float x = -1.0f;
  int part = 0;
  if (fabsf(lv.z) > MJ_MINVAL)
    for (int side = -1; side <= 1; side += 2) {
      const float sol = ((float)side * size.y - lp.z) / lv.z;
      if (sol >= 0.0f) {
        const float px = lp.x + sol * lv.x, py = lp.y + sol * lv.y;
        if (px * px + py * py <= size.x * size.x && (x < 0.0f || sol < x)) {
          x = sol;
          part = side;
        }
      }
    }
  float x0, x1;
  const float sol = ray_quad(lv.x * lv.x + lv.y * lv.y, lv.x * lp.x + lv.y * lp.y, lp.x * lp.x + lp.y * lp.y - size.x * size.x, x0, x1);
  if (sol >= 0.0f && fabsf(lp.z + sol * lv.z) <= size.y && (x < 0.0f || sol < x)) {
    x = sol;
    part = 0;
  }
  normal = V3{0, 0, 0};
  if (x >= 0.0f) {
    const V3 l = lp + lv * x;
    normal = mat_mul(mat, part == 0 ? normalize(V3{l.x, l.y, 0.0f}) : V3{0, 0, (float)part});
  }
  return x;
}
DEV float ray_box(V3 pos, const float* mat, V3 size, V3 pnt, V3 vec, V3& normal) {  // ray.py:420-471
  if (ray_sphere(pos, dot(size, size), pnt, vec, normal) < 0.0f) {
    normal = V3{0, 0, 0};
    return -1.0f;
  }
  const V3 lpv = matT_mul(mat, pnt - pos), lvv = matT_mul(mat, vec);
  const float lp[3] = {lpv.x, lpv.y, lpv.z}, lv[3] = {lvv.x, lvv.y, lvv.z}, sz[3] = {size.x, size.y, size.z};
  float x = -1.0f;
  int face_axis = -1, face_side = -1;
  for (int i = 0; i < 3; ++i) {
    if (!(fabsf(lv[i]) > MJ_MINVAL)) continue;
    for (int side = -1; side <= 1; side += 2) {
      const float sol = ((float)side * sz[i] - lp[i]) / lv[i];
      if (sol < 0.0f) continue;
      const int id0 = i == 0 ? 1 : 0, id1 = i == 2 ? 1 : 2;
      if (fabsf(lp[id0] + sol * lv[id0]) <= sz[id0] && fabsf(lp[id1] + sol * lv[id1]) <= sz[id1] && (x < 0.0f || sol < x)) {
        x = sol;
        face_axis = i;
        face_side = side;
      }
    }
  }
  normal = V3{0, 0, 0};
  if (x >= 0.0f) normal = V3{mat[face_axis], mat[3 + face_axis], mat[6 + face_axis]} * (float)face_side;
  return x;
}
DEV float ray_geom(int type, V3 pos, const float* mat, V3 size, V3 pnt, V3 vec, V3& normal) {  // ray.py:798-819
  normal = V3{0, 0, 0};
  switch (type) {
    case G_PLANE: return ray_plane(pos, mat, size, pnt, vec, normal);
    case G_SPHERE: return ray_sphere(pos, size.x * size.x, pnt, vec, normal);
    case G_CAPSULE: return ray_capsule(pos, mat, size, pnt, vec, normal);
    case G_ELLIPSOID: return ray_ellipsoid(pos, mat, size, pnt, vec, normal);
    case G_CYLINDER: return ray_cylinder(pos, mat, size, pnt, vec, normal);
    case G_BOX: return ray_box(pos, mat, size, pnt, vec, normal);
    default: return -1.0f;
  }
}
// ray_box with the distance at which the ray crosses each of the six faces inside the face's rectangle (ray.py:420-471 `all`: index
// 2 * axis + (side + 1) / 2, -1 where it does not); the height field's walls need them.  (ray_box itself stays as it was.)
DEV float ray_box_all(V3 pos, const float* mat, V3 size, V3 pnt, V3 vec, float* all, V3& normal) {
  for (int i = 0; i < 6; ++i) all[i] = -1.0f;
  if (ray_sphere(pos, dot(size, size), pnt, vec, normal) < 0.0f) {
    normal = V3{0, 0, 0};
    return -1.0f;
  }
  const V3 lpv = matT_mul(mat, pnt - pos), lvv = matT_mul(mat, vec);
  const float lp[3] = {lpv.x, lpv.y, lpv.z}, lv[3] = {lvv.x, lvv.y, lvv.z}, sz[3] = {size.x, size.y, size.z};
  float x = -1.0f;
  int face_axis = -1, face_side = -1;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (!(fabsf(lv[i]) > MJ_MINVAL)) continue;
#pragma unroll
    for (int side = -1; side <= 1; side += 2) {
      const float sol = ((float)side * sz[i] - lp[i]) / lv[i];
      if (sol < 0.0f) continue;
      const int id0 = i == 0 ? 1 : 0, id1 = i == 2 ? 1 : 2;
      if (fabsf(lp[id0] + sol * lv[id0]) <= sz[id0] && fabsf(lp[id1] + sol * lv[id1]) <= sz[id1]) {
        if (x < 0.0f || sol < x) {
          x = sol;
          face_axis = i;
          face_side = side;
        }
        all[2 * i + (side + 1) / 2] = sol;
      }
    }
  }
  normal = V3{0, 0, 0};
  if (x >= 0.0f) normal = V3{mat[face_axis], mat[3 + face_axis], mat[6 + face_axis]} * (float)face_side;
  return x;
}
// two unit vectors spanning the plane normal to the unit vector v (ray.py:128-151 _orthogonal_basis: Duff et al. 2017)
DEV void ray_basis(V3 v, V3& b0, V3& b1) {
  const float sign = v.z >= 0.0f ? 1.0f : -1.0f;
  const float a = -1.0f / (sign + v.z), b = v.x * v.y * a;
  b0 = V3{1.0f + sign * v.x * v.x * a, sign * b, -sign * v.x};
  b1 = V3{b, sign + v.y * v.y * a, -v.y};
}
// ray against one triangle (ray.py:154-210 _ray_triangle): the triangle is projected on the plane normal to the ray (b0, b1) and the origin
// located in it by barycentric coordinates; both sides hit; the normal is that of the vertex order, not turned towards the ray
DEV float ray_triangle(V3 v0, V3 v1, V3 v2, V3 pnt, V3 vec, V3 b0, V3 b1, V3& normal) {
  const V3 d0 = v0 - pnt, d1 = v1 - pnt, d2 = v2 - pnt;
  const float p00 = dot(d0, b0), p01 = dot(d0, b1), p10 = dot(d1, b0), p11 = dot(d1, b1), p20 = dot(d2, b0), p21 = dot(d2, b1);
  if ((p00 > 0.0f && p10 > 0.0f && p20 > 0.0f) || (p00 < 0.0f && p10 < 0.0f && p20 < 0.0f) || (p01 > 0.0f && p11 > 0.0f && p21 > 0.0f) ||
      (p01 < 0.0f && p11 < 0.0f && p21 < 0.0f))
    return -1.0f;
  const float A00 = p00 - p20, A10 = p10 - p20, A01 = p01 - p21, A11 = p11 - p21;
  const float det = A00 * A11 - A10 * A01;
  if (fabsf(det) < MJ_MINVAL) return -1.0f;
  const float t0 = (A11 * -p20 - A10 * -p21) / det, t1 = (-A01 * -p20 + A00 * -p21) / det;
  if (t0 < 0.0f || t1 < 0.0f || t0 + t1 > 1.0f) return -1.0f;
  const V3 nrm = cross(v0 - v2, v1 - v2);
  const float denom = dot(vec, nrm);
  if (fabsf(denom) < MJ_MINVAL) return -1.0f;
  const float dist = -dot(pnt - v2, nrm) / denom;
  if (dist < 0.0f) return -1.0f;
  normal = normalize(nrm);
  return dist;
}
// the nearest hit so far.  Candidates are ordered by (distance, geom, sub) -- sub numbers the pieces of one geom in the order the reference
// walks them (a mesh's triangles; a height field's base box, cell triangles, walls) -- so the minimum is the hit the reference's serial walk
// keeps (it replaces only on a strictly smaller distance), whatever the number of lanes that share the walk
struct RayHit {
  float dist;
  int geom, sub;
  V3 n;
};
DEV bool ray_hit_before(float dist, int geom, int sub, const RayHit& h) {
  return dist < h.dist || (dist == h.dist && (geom < h.geom || (geom == h.geom && sub < h.sub)));
}
DEV void ray_hit_take(RayHit& h, float dist, int geom, int sub, V3 n) {
  if (dist >= 0.0f && dist < MJ_MAXVAL && ray_hit_before(dist, geom, sub, h)) h = RayHit{dist, geom, sub, n};
}
// may the ray (local frame of the box) touch the box centre +- half?  Slab test on a box grown by a margin that covers the float32 rounding
// of the test itself (a mesh's box is tight: its outermost triangles lie in the box's faces), so the cull never drops a hit
DEV bool ray_box_overlap(V3 centre, V3 half, V3 lpnt, V3 lvec) {
  const V3 o = lpnt - centre;
  const float eps = 1e-5f * (fabsf(o.x) + fabsf(o.y) + fabsf(o.z) + half.x + half.y + half.z) + 1e-9f;
  const float op[3] = {o.x, o.y, o.z}, lv[3] = {lvec.x, lvec.y, lvec.z}, hs[3] = {half.x + eps, half.y + eps, half.z + eps};
  float t0 = 0.0f, t1 = MJ_MAXVAL;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!(fabsf(lv[k]) > MJ_MINVAL)) {
      if (fabsf(op[k]) > hs[k]) return false;
    } else {
      const float ta = (-hs[k] - op[k]) / lv[k], tb = (hs[k] - op[k]) / lv[k];
      t0 = fmaxf(t0, fminf(ta, tb));
      t1 = fminf(t1, fmaxf(ta, tb));
    }
  }
  return t1 >= t0 * (1.0f - 1e-5f);
}
// mesh geom g (ray.py:628-687 ray_mesh): this lane's share (triangles lane, lane + nlane, ...) of the mesh's triangles, in the geom frame.
// The reference culls with a box of geom_size about the geom origin; the mesh frame here is the principal frame at the centre of mass, whose
// bounding box is not centred, so the cull takes the geom's own geom_aabb (centre and half sizes)
DEV bool ray_mesh_cull(const MjhModel& m, int w, int g, V3 pos, const float* mat, V3 pnt, V3 vec) {  // true: the ray misses the mesh's box
  const float* ab = BF(m, geom_aabb, w) + 6 * g;
  return !ray_box_overlap(ld3(ab), ld3(ab + 3), matT_mul(mat, pnt - pos), matT_mul(mat, vec));
}
DEV void ray_mesh(const MjhModel& m, int g, V3 pos, const float* mat, V3 pnt, V3 vec, int lane, int nlane, RayHit& h) {
  const int id = m.geom_dataid[g];
  if (id < 0 || id >= m.nmesh || m.nmeshface == 0) return;
  const V3 lp = matT_mul(mat, pnt - pos), lv = matT_mul(mat, vec);
  V3 b0, b1;
  ray_basis(normalize(lv), b0, b1);  // (of the unit direction: rays() takes vec of any length; the reference's basis is only orthogonal for |vec| = 1)
  const float* vert = m.mesh_vert + 3 * (size_t)m.mesh_vertadr[id];
  const int f0 = m.mesh_faceadr[id], f1 = id + 1 < m.nmesh ? m.mesh_faceadr[id + 1] : m.nmeshface;
  bool took = false;
  for (int f = f0 + lane; f < f1; f += nlane) {
    const int* fv = m.mesh_face + 3 * (size_t)f;
    V3 n;
    const float x = ray_triangle(ld3(vert + 3 * fv[0]), ld3(vert + 3 * fv[1]), ld3(vert + 3 * fv[2]), lp, lv, b0, b1, n);
    if (x >= 0.0f && x < MJ_MAXVAL && ray_hit_before(x, g, f - f0, h)) {
      h = RayHit{x, g, f - f0, n};
      took = true;
    }
  }
  if (took) h.n = mat_mul(mat, h.n);
}
// height-field geom g (ray.py:474-625 ray_hfield): base box, then -- if the ray meets the box around the elevated part -- the two triangles of
// every grid cell under the segment inside that box (one cell of padding), then the four walls under the height profile.  The cells are
// shared out over the lanes; lane 0 also takes the base box and the walls
DEV void ray_hfield(const MjhModel& m, int g, V3 pos, const float* mat, V3 pnt, V3 vec, int lane, int nlane, RayHit& h) {
  const int hid = m.geom_dataid[g];
  if (hid < 0 || hid >= m.nhfield) return;
  const int nrow = m.hfield_nrow[hid], ncol = m.hfield_ncol[hid];
  const float* size = m.hfield_size + 4 * hid;
  const float* data = m.hfield_data + m.hfield_adr[hid];
  const V3 zax = V3{mat[2], mat[5], mat[8]};
  V3 nb, nt;
  float all[6];
  const float xbase = ray_box(pos - zax * (size[3] * 0.5f), mat, V3{size[0], size[1], size[3] * 0.5f}, pnt, vec, nb);
  if (lane == 0) ray_hit_take(h, xbase, g, 0, nb);
  const float top = ray_box_all(pos + zax * (size[2] * 0.5f), mat, V3{size[0], size[1], size[2] * 0.5f}, pnt, vec, all, nt);
  if (top < 0.0f || nrow < 2 || ncol < 2) return;
  const V3 lp = matT_mul(mat, pnt - pos), lv = matT_mul(mat, vec);
  V3 b0, b1;
  ray_basis(normalize(lv), b0, b1);
  float s0 = 0.0f, s1 = top;  // the part of the ray inside the top box
  for (int i = 0; i < 6; ++i)
    if (all[i] > s1) {
      s0 = top;
      s1 = all[i];
    }
  const float dx = safe_div(2.0f * size[0], (float)(ncol - 1)), dy = safe_div(2.0f * size[1], (float)(nrow - 1));
  const float sx0 = safe_div(lp.x + s0 * lv.x + size[0], dx), sx1 = safe_div(lp.x + s1 * lv.x + size[0], dx);
  const float sy0 = safe_div(lp.y + s0 * lv.y + size[1], dy), sy1 = safe_div(lp.y + s1 * lv.y + size[1], dy);
  const int cmin = max(0, (int)(floorf(fminf(sx0, sx1)) - 1.0f)), cmax = min(ncol - 1, (int)(ceilf(fmaxf(sx0, sx1)) + 1.0f));
  const int rmin = max(0, (int)(floorf(fminf(sy0, sy1)) - 1.0f)), rmax = min(nrow - 1, (int)(ceilf(fmaxf(sy0, sy1)) + 1.0f));
  const int nc = cmax - cmin, ncell = nc > 0 && rmax > rmin ? nc * (rmax - rmin) : 0;
  bool took = false;
  for (int k = lane; k < ncell; k += nlane) {
    const int r = rmin + k / nc, c = cmin + k % nc;
    const float xa = dx * (float)c - size[0], xb = dx * (float)(c + 1) - size[0], ya = dy * (float)r - size[1], yb = dy * (float)(r + 1) - size[1];
    const V3 v00 = V3{xa, ya, data[r * ncol + c] * size[2]}, v10 = V3{xb, ya, data[r * ncol + c + 1] * size[2]};
    const V3 v11 = V3{xb, yb, data[(r + 1) * ncol + c + 1] * size[2]}, v01 = V3{xa, yb, data[(r + 1) * ncol + c] * size[2]};
    const int sub = 1 + 2 * (r * (ncol - 1) + c);
    V3 n;
    float x = ray_triangle(v00, v10, v11, lp, lv, b0, b1, n);
    if (x >= 0.0f && x < MJ_MAXVAL && ray_hit_before(x, g, sub, h)) {
      h = RayHit{x, g, sub, n};
      took = true;
    }
    x = ray_triangle(v00, v11, v01, lp, lv, b0, b1, n);
    if (x >= 0.0f && x < MJ_MAXVAL && ray_hit_before(x, g, sub + 1, h)) {
      h = RayHit{x, g, sub + 1, n};
      took = true;
    }
  }
  if (lane == 0) {
    const int wall0 = 1 + 2 * (nrow - 1) * (ncol - 1);
    for (int i = 0; i < 4; ++i) {
      if (!(all[i] >= 0.0f)) continue;
      const float z = safe_div(lp.z + all[i] * lv.z, size[2]);  // height of the crossing, in units of the elevation data
      float y, z0, z1;
      int y0;
      if (i < 2) {  // the walls at -x / +x: along the rows of the first / last column
        y = safe_div(lp.y + all[i] * lv.y + size[1], dy);
        y0 = (int)fmaxf(0.0f, fminf((float)(nrow - 2), floorf(y)));
        const int c = i == 1 ? ncol - 1 : 0;
        z0 = data[y0 * ncol + c];
        z1 = data[(y0 + 1) * ncol + c];
      } else {  // the walls at -y / +y: along the columns of the first / last row
        y = safe_div(lp.x + all[i] * lv.x + size[0], dx);
        y0 = (int)fmaxf(0.0f, fminf((float)(ncol - 2), floorf(y)));
        const int r = i == 3 ? nrow - 1 : 0;
        z0 = data[r * ncol + y0];
        z1 = data[r * ncol + y0 + 1];
      }
      if (z < z0 * ((float)y0 + 1.0f - y) + z1 * (y - (float)y0) && all[i] < MJ_MAXVAL && ray_hit_before(all[i], g, wall0 + i, h)) {
        h = RayHit{all[i], g, wall0 + i, V3{(float)(i == 1) - (float)(i == 0), (float)(i == 3) - (float)(i == 2), 0.0f}};
        took = true;
      }
    }
  }
  if (took) h.n = mat_mul(mat, h.n);
}
struct RayGroup {
  float g[6];
};
// geoms a ray ignores (ray.py:52-102 _ray_eliminate): the excluded body's, invisible ones (alpha 0 on the geom or on its material),
// static ones unless flg_static, and those outside the group mask (a mask of six -1 includes every group)
DEV bool ray_eliminate(const MjhModel& m, int g, const RayGroup& gg, int flg_static, int bodyexclude) {
  const int b = m.geom_bodyid[g], mat = m.geom_matid[g];
  if (b == bodyexclude) return true;
  if (mat < 0 && m.geom_rgba[4 * g + 3] == 0.0f) return true;
  if (mat >= 0 && m.mat_rgba[4 * mat + 3] == 0.0f) return true;
  if (!flg_static && m.body_weldid[b] == 0) return true;
  bool none = true;
  for (int i = 0; i < 6; ++i) none = none && gg.g[i] == -1.0f;
  if (none) return false;
  return gg.g[min(5, max(0, m.geom_group[g]))] == 0.0f;
}
// nearest hit of one ray in world w (ray.py:907-1011 _ray): distance (-1: none), the geom and the surface normal there
DEV float ray_world(const MjhModel& m, const MjhData& d, int w, V3 pnt, V3 vec, const RayGroup& gg, int flg_static, int bodyexclude, int& geomid, V3& normal) {
  float best = MJ_MAXVAL;
  geomid = -1;
  normal = V3{0, 0, 0};
  for (int g = 0; g < m.ngeom; ++g) {
    if (ray_eliminate(m, g, gg, flg_static, bodyexclude)) continue;
    V3 n;
    const float dist = ray_geom(m.geom_type[g], ld3(d.geom_xpos + ((size_t)w * m.ngeom + g) * 3), d.geom_xmat + ((size_t)w * m.ngeom + g) * 9,
                                ld3(BF(m, geom_size, w) + 3 * g), pnt, vec, n);
    if (dist >= 0.0f && dist < best) {
      best = dist;
      geomid = g;
      normal = n;
    }
  }
  return best >= MJ_MAXVAL ? -1.0f : best;
}
#ifndef MJH_RAY_NO_KERNELS  // (render_tu.hip takes the device functions only: a kernel is defined in one translation unit)
// rays (ray.py:1219-1325): pnt / vec [pnt_nworld (1 or nworld), nray, 3]; bodyexclude [nray]; outputs [nworld, nray]
__global__ void __launch_bounds__(256) k_rays(MjhModel m, MjhData d, const float* pnt, const float* vec, int pnt_nworld, int nray, RayGroup gg, int flg_static,
                                              const int* bodyexclude, float* dist, int* geomid, float* normal) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= d.nworld * nray) return;
  const int w = idx / nray, r = idx - w * nray;
  const size_t src = ((size_t)(w % pnt_nworld) * nray + r) * 3;
  int g;
  V3 n;
  const float x = ray_world(m, d, w, ld3(pnt + src), ld3(vec + src), gg, flg_static, bodyexclude ? bodyexclude[r] : -1, g, n);
  dist[idx] = x;
  if (geomid) geomid[idx] = g;
  if (normal) st3(normal + (size_t)idx * 3, n);
}
#endif

// ---- models with mesh triangles or height fields ----
// lanes of a (world, ray) group in k_rays_group (one DPP row: the closing reduction stays inside a row) and the model size from which the group
// pays: measured on an MI355X (profiles/ray_mesh.json) -- aloha_pot (490 triangles per mesh on average), 8192 worlds x 256 rays:
// one thread per ray 44.7 ms, 16 lanes 6.46, 32 lanes 6.95, 64 lanes 8.34; clutter_synth (10 per mesh), 2048 x 256: one thread 170 us, 16 lanes
// 251, 32 lanes 408, 64 lanes 634 -- every lane of a group repeats a mesh's set-up, which a walk of a few triangles does not repay
constexpr int RAY_LANES = 16;
constexpr int RAY_GROUP_MIN_FACES = 64;  // mean triangles per mesh above which rays() takes the lane-group kernel: four strides of a group
// a primitive geom, whole; for a mesh or a height field: does the ray need its triangles (ray_shared below)?
DEV bool ray_geom_first(const MjhModel& m, const MjhData& d, int w, int g, V3 pnt, V3 vec, RayHit& h) {
  const int type = m.geom_type[g];
  const V3 pos = ld3(d.geom_xpos + ((size_t)w * m.ngeom + g) * 3);
  const float* mat = d.geom_xmat + ((size_t)w * m.ngeom + g) * 9;
  if (type == G_MESH) return !ray_mesh_cull(m, w, g, pos, mat, pnt, vec);
  if (type == G_HFIELD) return true;
  V3 n;
  const float x = ray_geom(type, pos, mat, ld3(BF(m, geom_size, w) + 3 * g), pnt, vec, n);
  ray_hit_take(h, x, g, 0, n);
  return false;
}
// this lane's share (of nlane) of the triangles / cells of mesh or height-field geom g
DEV void ray_shared(const MjhModel& m, const MjhData& d, int w, int g, V3 pnt, V3 vec, int lane, int nlane, RayHit& h) {
  const V3 pos = ld3(d.geom_xpos + ((size_t)w * m.ngeom + g) * 3);
  const float* mat = d.geom_xmat + ((size_t)w * m.ngeom + g) * 9;
  if (m.geom_type[g] == G_MESH) ray_mesh(m, g, pos, mat, pnt, vec, lane, nlane, h);
  else ray_hfield(m, g, pos, mat, pnt, vec, lane, nlane, h);
}
// ray_world with mesh and height-field geoms, walked by one lane: the rangefinder sensor's path (one thread per sensor: a model with
// rangefinders and large meshes pays the whole triangle walk per sensor and world)
DEV float ray_world_full(const MjhModel& m, const MjhData& d, int w, V3 pnt, V3 vec, const RayGroup& gg, int flg_static, int bodyexclude, int& geomid, V3& normal) {
  RayHit h = RayHit{MJ_MAXVAL, -1, 0, V3{0, 0, 0}};
  for (int g = 0; g < m.ngeom; ++g) {
    if (ray_eliminate(m, g, gg, flg_static, bodyexclude)) continue;
    if (ray_geom_first(m, d, w, g, pnt, vec, h)) ray_shared(m, d, w, g, pnt, vec, 0, 1, h);
  }
  geomid = h.geom;
  normal = h.n;
  return h.dist >= MJ_MAXVAL ? -1.0f : h.dist;
}
#ifndef MJH_RAY_NO_KERNELS
// rays() on a model with large meshes or a height field: G = RAY_LANES lanes per (world, ray).  Groups are numbered ray-major (group q: world q % nworld, ray q / nworld), so the
// 256 / G groups of a workgroup cast the same ray in neighbouring worlds: with a broadcast pnt / vec, and for static geoms in any case, they
// walk the same model-constant triangles, which the workgroup then fetches once into its L1 / from L2 instead of once per world.
// Round one: lane l takes geoms l, l + G, ... -- elimination, primitives whole, the box cull of meshes; a ballot collects the meshes that
// survive it and the height fields.
// Round two: the group walks those one after the other, lanes striding over the triangles / cells.  Then one min-reduction.
__global__ void __launch_bounds__(256) k_rays_group(MjhModel m, MjhData d, const float* pnt, const float* vec, int pnt_nworld, int nray, RayGroup gg, int flg_static,
                                                    const int* bodyexclude, float* dist, int* geomid, float* normal) {
  constexpr int G = RAY_LANES;
  const int q = blockIdx.x * (256 / G) + threadIdx.x / G, lane = threadIdx.x % G;
  if (q >= d.nworld * nray) return;  // (whole groups leave: the cross-lane steps below stay inside a group)
  const int r = q / d.nworld, w = q - r * d.nworld;
  const size_t src = ((size_t)(w % pnt_nworld) * nray + r) * 3;
  const V3 p = ld3(pnt + src), v = ld3(vec + src);
  const int ex = bodyexclude ? bodyexclude[r] : -1;
  RayHit h = RayHit{MJ_MAXVAL, -1, 0, V3{0, 0, 0}};
  for (int g0 = 0; g0 < m.ngeom; g0 += G) {
    const int g = g0 + lane;
    bool shared = false;
    if (g < m.ngeom && !ray_eliminate(m, g, gg, flg_static, ex)) shared = ray_geom_first(m, d, w, g, p, v, h);
    unsigned long long todo = gballot<G>(shared);
    while (todo) {
      const int gs = g0 + __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      ray_shared(m, d, w, gs, p, v, lane, G, h);
    }
  }
  // the group's minimum of (dist, geom, sub): after the butterfly every lane knows the winner, the lane that holds it writes
  float bd = h.dist;
  int bg = h.geom, bs = h.sub;
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) {
    const float od = __shfl_xor(bd, off, G);
    const int og = __shfl_xor(bg, off, G), os = __shfl_xor(bs, off, G);
    if (od < bd || (od == bd && (og < bg || (og == bg && os < bs)))) {
      bd = od;
      bg = og;
      bs = os;
    }
  }
  const size_t out = (size_t)w * nray + r;
  if (bg < 0) {
    if (lane == 0) {
      dist[out] = -1.0f;
      if (geomid) geomid[out] = -1;
      if (normal) st3(normal + out * 3, V3{0, 0, 0});
    }
  } else if (h.geom == bg && h.sub == bs && h.dist == bd) {  // (geom, sub) names one candidate, which one lane evaluated
    dist[out] = bd;
    if (geomid) geomid[out] = bg;
    if (normal) st3(normal + out * 3, h.n);
  }
}

// rays() on a model whose meshes have few triangles each: one thread per (world, ray), like k_rays, over ray_world_full
__global__ void __launch_bounds__(256) k_rays_serial_full(MjhModel m, MjhData d, const float* pnt, const float* vec, int pnt_nworld, int nray, RayGroup gg, int flg_static,
                                                          const int* bodyexclude, float* dist, int* geomid, float* normal) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= d.nworld * nray) return;
  const int w = idx / nray, r = idx - w * nray;
  const size_t src = ((size_t)(w % pnt_nworld) * nray + r) * 3;
  int g;
  V3 n;
  const float x = ray_world_full(m, d, w, ld3(pnt + src), ld3(vec + src), gg, flg_static, bodyexclude ? bodyexclude[r] : -1, g, n);
  dist[idx] = x;
  if (geomid) geomid[idx] = g;
  if (normal) st3(normal + (size_t)idx * 3, n);
}
#endif  // MJH_RAY_NO_KERNELS
