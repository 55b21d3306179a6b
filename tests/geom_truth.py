"""Geometric ground truth for the primitive colliders: plain NumPy float64, closed forms and one-dimensional searches on the shapes
themselves.  Nothing here knows the colliders' algorithms and nothing calls the oracle: a contact is compared with the geometry it
claims to describe (same role as tests/ray_bruteforce.py for rays and cameras).

A shape is (kind, pos, mat, size[, vert]): `mat` is the 3x3 rotation whose columns are the shape's axes in the world, `size` follows the
geom_size convention (sphere r | capsule r, half length | box half extents | cylinder r, half height | ellipsoid radii), a plane is
the half space below z = 0 of its frame, a mesh is the convex hull of `vert` (geom frame).
"""

import itertools

import numpy as np

from mujoco_warp_amd import _npmath


class Shape:
  def __init__(self, kind, pos, mat, size=(), vert=None):
    self.kind = kind
    self.pos = np.asarray(pos, dtype=np.float64).reshape(3)
    self.mat = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    self.size = np.asarray(size, dtype=np.float64).reshape(-1)
    self.vert = None if vert is None else np.asarray(vert, dtype=np.float64).reshape(-1, 3)

  def local(self, x):
    return (np.asarray(x, dtype=np.float64) - self.pos) @ self.mat  # mat' (x - pos), for x[..., 3]

  def world(self, x):
    return np.asarray(x, dtype=np.float64) @ self.mat.T + self.pos

  @property
  def axis(self):
    return self.mat[:, 2]


def from_quat(kind, pos, quat, size=(), vert=None):
  return Shape(kind, pos, _npmath.quat_to_mat(_npmath.quat_normalize(np.asarray(quat, dtype=np.float64))).reshape(3, 3), size, vert)


# ------------------------------------------------------------------------------------------------------ signed distance
def sdf(shape, x):
  """Signed distance of the points x[..., 3] to the shape's surface, negative inside (closed form)."""
  l, s, k = shape.local(x), shape.size, shape.kind
  if k == "plane":
    return l[..., 2]
  if k == "sphere":
    return np.linalg.norm(l, axis=-1) - s[0]
  if k == "capsule":
    d = l.copy()
    d[..., 2] -= np.clip(l[..., 2], -s[1], s[1])
    return np.linalg.norm(d, axis=-1) - s[0]
  if k == "box":
    q = np.abs(l) - s[:3]
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
  if k == "cylinder":
    q = np.stack([np.hypot(l[..., 0], l[..., 1]) - s[0], np.abs(l[..., 2]) - s[1]], axis=-1)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)
  raise ValueError(f"no closed-form signed distance for {k}")


def sdf_gradient(shape, x, h=1e-7):
  """Central-difference gradient of the signed distance at one point (unit length away from the medial axis)."""
  x = np.asarray(x, dtype=np.float64)
  e = np.eye(3) * h
  return (sdf(shape, x + e) - sdf(shape, x - e)) / (2 * h)


def ellipsoid_implicit(shape, x):
  """F(x) = sum (x_i / r_i)^2 - 1 in the ellipsoid's frame and the norm of its gradient: F / |grad F| is the first-order distance of x
  to the surface."""
  l = shape.local(x)
  F = np.sum((l / shape.size[:3]) ** 2, axis=-1) - 1.0
  return F, np.linalg.norm(2.0 * l / shape.size[:3] ** 2, axis=-1)


# ------------------------------------------------------------------------------------------------------------- support
def support_point(shape, direction):
  """A point of the shape furthest along `direction` (world)."""
  d = np.asarray(direction, dtype=np.float64)
  d = d / np.linalg.norm(d)
  dl, s, k = shape.mat.T @ d, shape.size, shape.kind
  sgn = lambda v: np.where(v >= 0, 1.0, -1.0)
  if k == "sphere":
    return shape.pos + s[0] * d
  if k == "capsule":
    return shape.pos + shape.axis * (sgn(dl[2]) * s[1]) + s[0] * d
  if k == "box":
    return shape.world(sgn(dl) * s[:3])
  if k == "cylinder":
    rn = np.hypot(dl[0], dl[1])
    rad = np.array([dl[0], dl[1]]) * (s[0] / rn) if rn > 0 else np.zeros(2)
    return shape.world(np.array([rad[0], rad[1], sgn(dl[2]) * s[1]]))
  if k == "ellipsoid":
    return shape.world(s[:3] ** 2 * dl / np.linalg.norm(s[:3] * dl))
  if k == "mesh":
    return shape.world(shape.vert[np.argmax(shape.vert @ dl)])
  raise ValueError(f"no support function for {k}")


def support(shape, direction):
  """h_X(direction) = max over the shape of <x, direction / |direction|>."""
  d = np.asarray(direction, dtype=np.float64)
  return float(support_point(shape, d) @ (d / np.linalg.norm(d)))


def plane_distance(plane, shape):
  """Signed distance of a convex shape to a plane: the height of its lowest point, -h_X(-n) in the plane's offset."""
  n = plane.axis
  return -support(shape, -n) - float(plane.pos @ n)


# ---------------------------------------------------------------------------------------------- one-dimensional searches
_INVPHI = (np.sqrt(5.0) - 1.0) / 2.0


def segment_shape_distance(p, q, shape, tol=1e-12):
  """(min over the segment p-q of the shape's signed distance, the parameter where it is attained) by golden-section search.  The signed
  distance of a convex set is a convex function, so its restriction to a segment is unimodal: outside, and inside as well."""
  p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
  f = lambda t: float(sdf(shape, p + t * (q - p)))
  a, b = 0.0, 1.0
  c, d = b - _INVPHI * (b - a), a + _INVPHI * (b - a)
  fc, fd = f(c), f(d)
  while b - a > tol:
    if fc < fd:
      b, d, fd = d, c, fc
      c = b - _INVPHI * (b - a)
      fc = f(c)
    else:
      a, c, fc = c, d, fd
      d = a + _INVPHI * (b - a)
      fd = f(d)
  cands = [(f(t), t) for t in (0.0, 1.0, 0.5 * (a + b))]
  return min(cands)


def point_segment_distance(x, p, q):
  pq = q - p
  den = float(pq @ pq)
  t = 0.0 if den == 0.0 else min(1.0, max(0.0, float((x - p) @ pq) / den))
  return float(np.linalg.norm(x - (p + t * pq)))


def segment_segment_distance(p1, q1, p2, q2):
  """Distance of two segments: the interior / clamped solution (Ericson, Real-Time Collision Detection 5.1.9) and, for the nearly parallel
  case where its determinant carries no digits, the four endpoint-to-segment distances; every candidate is a distance between two points
  of the segments, so the minimum is the answer."""
  p1, q1, p2, q2 = (np.asarray(v, dtype=np.float64) for v in (p1, q1, p2, q2))
  d1, d2, r = q1 - p1, q2 - p2, p1 - p2
  a, e, f, c, b = d1 @ d1, d2 @ d2, d2 @ r, d1 @ r, d1 @ d2
  if a == 0.0 or e == 0.0:  # a point
    return point_segment_distance(p1, p2, q2) if a == 0.0 else point_segment_distance(p2, p1, q1)
  den = a * e - b * b
  s = min(1.0, max(0.0, (b * f - c * e) / den)) if den > 1e-14 * a * e else 0.0
  t = (b * s + f) / e
  if t < 0.0:
    t, s = 0.0, min(1.0, max(0.0, -c / a))
  elif t > 1.0:
    t, s = 1.0, min(1.0, max(0.0, (b - c) / a))
  best = float(np.linalg.norm(p1 + s * d1 - p2 - t * d2))
  return min(best, point_segment_distance(p1, p2, q2), point_segment_distance(q1, p2, q2), point_segment_distance(p2, p1, q1),
             point_segment_distance(q2, p1, q1))


# ----------------------------------------------------------------------------------------------------------- box - box
_CORNERS = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))
_EDGES = [(i, j) for i in range(8) for j in range(i + 1, 8) if np.sum(_CORNERS[i] != _CORNERS[j]) == 1]  # 12 edges


def box_vertices(box):
  return box.world(_CORNERS * box.size[:3])


def box_box_distance(b1, b2):
  """Distance of two SEPARATED boxes: the closest features are a vertex and a face or two edges (face-face and edge-face contacts contain
  a vertex-face or edge-edge pair at the same distance): min over 16 vertex-vs-box signed distances and 144 edge-edge distances."""
  v1, v2 = box_vertices(b1), box_vertices(b2)
  best = min(float(sdf(b2, v1).min()), float(sdf(b1, v2).min()))
  for i, j in _EDGES:
    for k, l in _EDGES:
      best = min(best, segment_segment_distance(v1[i], v1[j], v2[k], v2[l]))
  return best


def box_box_sat_depth(b1, b2):
  """(minimum overlap over the 15 separating axes, that axis as a unit vector pointing from b1 to b2, its index: 0-2 faces of b1, 3-5
  faces of b2, 6-14 edge x edge) -- the penetration depth of two overlapping boxes; negative when an axis separates them."""
  axes = [b1.mat[:, i] for i in range(3)] + [b2.mat[:, i] for i in range(3)]
  for i in range(3):
    for j in range(3):
      axes.append(np.cross(b1.mat[:, i], b2.mat[:, j]))
  dp = b2.pos - b1.pos
  best = (np.inf, None, -1)
  for idx, L in enumerate(axes):
    nrm = np.linalg.norm(L)
    if nrm < 1e-9:  # parallel edges: the axis is covered by the face axes
      continue
    L = L / nrm
    r1 = float(np.abs(b1.mat.T @ L) @ b1.size[:3])
    r2 = float(np.abs(b2.mat.T @ L) @ b2.size[:3])
    c = float(L @ dp)
    overlap = r1 + r2 - abs(c)
    if overlap < best[0] - (1e-12 if idx >= 6 else 0.0):  # (a tie goes to the face axis: for aligned faces edge x edge axes repeat it)
      best = (overlap, L if c >= 0 else -L, idx)
  return best
