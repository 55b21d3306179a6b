"""Ground truth for rays against mesh and height-field geoms: a brute-force caster over every triangle, NumPy, Moeller-Trumbore (the
engine and the reference project the triangle on the ray's normal plane instead: the two formulations share no arithmetic).

A mesh geom is its triangle soup (Model.mesh_face over mesh_vert) moved to the world frame with the oracle's geom_xpos / geom_xmat.  A
height-field geom is the closed surface of the solid: the 2 (nrow - 1) (ncol - 1) triangles of the elevation grid, the four side walls
between z = 0 and the profile, and the base box below z = 0.  Every triangle carries the normal the engine reports for it (the vertex
order's normal cross(v0 - v2, v1 - v2) for mesh and grid triangles -- not turned towards the ray --, the outward one for walls and base).

`dtype` runs the whole computation in float64 (the ground truth) or float32 (to count, on the CPU, the grazing rays whose answer depends
on the precision)."""

import numpy as np

MESH, HFIELD = 7, 1


def moller_trumbore(pnt, vec, tri, dtype=np.float64):
  """pnt, vec [nray, 3]; tri [ntri, 3, 3] -> (t [nray, ntri], inf where the ray misses; edge [nray, ntri]: the smallest barycentric
  coordinate of the hit).  Both sides of a triangle hit; t is in units of |vec|, hits at t < 0 are misses."""
  pnt, vec, tri = np.asarray(pnt, dtype=dtype), np.asarray(vec, dtype=dtype), np.asarray(tri, dtype=dtype)
  e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]  # [ntri, 3]
  P = np.cross(vec[:, None, :], e2[None, :, :])  # [nray, ntri, 3]
  det = np.einsum("rtk,tk->rt", P, e1)
  T = pnt[:, None, :] - tri[None, :, 0, :]
  Q = np.cross(T, e1[None, :, :])
  with np.errstate(divide="ignore", invalid="ignore"):
    inv = dtype(1.0) / det
    u = np.einsum("rtk,rtk->rt", T, P) * inv
    v = np.einsum("rtk,rk->rt", Q, vec) * inv
    t = np.einsum("rtk,tk->rt", Q, e2) * inv
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
    edge = np.minimum(np.minimum(u, v), dtype(1.0) - u - v)
  return np.where(ok, t, np.inf), np.where(ok, edge, -np.inf)


def _vertex_order_normals(tri):
  n = np.cross(tri[:, 0] - tri[:, 2], tri[:, 1] - tri[:, 2])
  return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


def mesh_triangles(mjm, g):
  """Triangles [nface, 3, 3] of mesh geom g in the geom frame."""
  i = int(mjm.geom_dataid[g])
  v = np.asarray(mjm.mesh_vert, dtype=np.float64)[mjm.mesh_vertadr[i] : mjm.mesh_vertadr[i] + mjm.mesh_vertnum[i]]
  f0 = int(mjm.mesh_faceadr[i])
  f1 = int(mjm.mesh_faceadr[i + 1]) if i + 1 < len(mjm.mesh_faceadr) else int(mjm.nmeshface)
  return v[np.asarray(mjm.mesh_face)[f0:f1]]


def hfield_triangles(mjm, g):
  """(triangles [n, 3, 3], normals [n, 3]) of height-field geom g in the geom frame: grid, walls, base box."""
  h = int(mjm.geom_dataid[g])
  nrow, ncol = int(mjm.hfield_nrow[h]), int(mjm.hfield_ncol[h])
  sx, sy, sz, base = (float(x) for x in mjm.hfield_size[h])
  z = np.asarray(mjm.hfield_data, dtype=np.float64)[mjm.hfield_adr[h] : mjm.hfield_adr[h] + nrow * ncol].reshape(nrow, ncol) * sz
  xs, ys = np.linspace(-sx, sx, ncol), np.linspace(-sy, sy, nrow)
  P = lambda r, c: np.array([xs[c], ys[r], z[r, c]])
  tris, nrms = [], []
  for r in range(nrow - 1):
    for c in range(ncol - 1):
      for t in ((P(r, c), P(r, c + 1), P(r + 1, c + 1)), (P(r, c), P(r + 1, c + 1), P(r + 1, c))):
        tris.append(t)
        nrms.append(None)

  def quad(a, b, c, d, n):  # a, b, c, d around the rectangle
    for t in ((a, b, c), (a, c, d)):
      tris.append(t)
      nrms.append(np.array(n, dtype=np.float64))

  flat = lambda p: np.array([p[0], p[1], 0.0])
  for c in range(ncol - 1):  # walls at -y (row 0) and +y (last row)
    for r, n in ((0, (0, -1, 0)), (nrow - 1, (0, 1, 0))):
      quad(flat(P(r, c)), flat(P(r, c + 1)), P(r, c + 1), P(r, c), n)
  for r in range(nrow - 1):  # walls at -x (column 0) and +x (last column)
    for c, n in ((0, (-1, 0, 0)), (ncol - 1, (1, 0, 0))):
      quad(flat(P(r, c)), flat(P(r + 1, c)), P(r + 1, c), P(r, c), n)
  lo, hi = np.array([-sx, -sy, -base]), np.array([sx, sy, 0.0])
  for ax in range(3):  # base box
    for side, val in ((-1, lo[ax]), (1, hi[ax])):
      a1, a2 = (ax + 1) % 3, (ax + 2) % 3
      cs = []
      for p1, p2 in ((lo[a1], lo[a2]), (hi[a1], lo[a2]), (hi[a1], hi[a2]), (lo[a1], hi[a2])):
        p = np.zeros(3)
        p[ax], p[a1], p[a2] = val, p1, p2
        cs.append(p)
      n = np.zeros(3)
      n[ax] = side
      quad(*cs, n)
  tris = np.array(tris, dtype=np.float64)
  vn = _vertex_order_normals(tris)
  return tris, np.array([vn[k] if n is None else n for k, n in enumerate(nrms)])


def eliminated(mjm, g, geomgroup=None, flg_static=True, bodyexclude=-1):
  """The reference's _ray_eliminate (ray.py:52) for geom g."""
  b, mat = int(mjm.geom_bodyid[g]), int(mjm.geom_matid[g])
  if b == bodyexclude:
    return True
  if (mat < 0 and mjm.geom_rgba[g][3] == 0) or (mat >= 0 and mjm.mat_rgba[mat][3] == 0):
    return True
  if not flg_static and int(mjm.body_weldid[b]) == 0:
    return True
  if geomgroup is None or all(x == -1 for x in geomgroup):
    return False
  return geomgroup[min(5, max(0, int(mjm.geom_group[g])))] == 0


class Caster:
  """Brute-force caster over the mesh and height-field geoms of `mjm` posed by the oracle state `sim` (after sim.forward())."""

  def __init__(self, mjm, sim, dtype=np.float64):
    self.mjm, self.dtype, self.geoms = mjm, dtype, []
    for g in range(mjm.ngeom):
      t = int(mjm.geom_type[g])
      if t not in (MESH, HFIELD) or int(mjm.geom_dataid[g]) < 0:
        continue
      R, p = np.asarray(sim.geom_xmat[g], dtype=np.float64).reshape(3, 3), np.asarray(sim.geom_xpos[g], dtype=np.float64)
      if t == MESH:
        tri = mesh_triangles(mjm, g)
        nrm = _vertex_order_normals(tri)
      else:
        tri, nrm = hfield_triangles(mjm, g)
      self.geoms.append((g, tri @ R.T + p, nrm @ R.T))

  def cast(self, pnt, vec, geomgroup=None, flg_static=True, bodyexclude=-1):
    """(dist [nray] (-1: none), geomid [nray], normal [nray, 3], edge [nray]: smallest barycentric coordinate of the winning hit)."""
    n = len(pnt)
    best, gid, nrm, edge = np.full(n, np.inf), np.full(n, -1), np.zeros((n, 3)), np.zeros(n)
    for g, tri, tn in self.geoms:
      if eliminated(self.mjm, g, geomgroup, flg_static, bodyexclude):
        continue
      t, e = moller_trumbore(pnt, vec, tri, self.dtype)
      k = np.argmin(t, axis=1)
      tk = t[np.arange(n), k]
      ek = e[np.arange(n), k]
      # coincident triangles with different normals (thin double-sided parts of real meshes store a face once per side): like a shared edge,
      # they tie on distance, and which one a float32 walk keeps is not geometry -- the hit's normal is marked as not comparable (edge 0)
      with np.errstate(invalid="ignore"):
        tied = np.isfinite(tk)[:, None] & (np.abs(t - tk[:, None]) <= 1e-7 * np.maximum(1.0, np.abs(tk))[:, None])
      ek = np.where((tied & ((tn[None, :, :] * tn[k][:, None, :]).sum(axis=2) < 1.0 - 1e-6)).any(axis=1), 0.0, ek)
      take = tk < best  # (geoms in ascending order: a tie keeps the lower id)
      best[take], gid[take], nrm[take], edge[take] = tk[take], g, tn[k[take]], ek[take]
    miss = ~np.isfinite(best)
    best[miss] = -1.0
    return best, gid, nrm, edge


def expected(caster, sim, pnt, vec, geomgroup=None, flg_static=True, bodyexclude=-1):
  """The nearer of the brute force (meshes, height fields) and the oracle's primitive walk (RefSim.ray) for every ray; ties: lower geom id."""
  dist, gid, nrm, edge = caster.cast(pnt, vec, geomgroup, flg_static, bodyexclude)
  dist, gid, nrm, edge = dist.copy(), gid.copy(), nrm.copy(), edge.copy()
  dt = caster.dtype
  for r in range(len(pnt)):
    pd, pg, pn = sim.ray(np.asarray(pnt[r], dtype=dt), np.asarray(vec[r], dtype=dt), geomgroup=geomgroup, flg_static=flg_static, bodyexclude=bodyexclude)
    if pg >= 0 and (gid[r] < 0 or pd < dist[r] or (pd == dist[r] and pg < gid[r])):
      dist[r], gid[r], nrm[r], edge[r] = pd, pg, pn, 1.0  # (a primitive's normal is always compared)
  return dist, gid, nrm, edge
