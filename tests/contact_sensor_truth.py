"""Plain-numpy statement of what a <contact> sensor reads, for ONE world (no engine code; used by tests/test_contact_sensor.py).

A sensor selects contacts (by geom, body, subtree or site volume, optionally a second object), numbers the matches in contact order, keeps
the first `maxmatch`, optionally sorts them (stable: ties keep contact order) by distance or force, and writes `num` slots of the requested
fields; `netforce` writes one slot holding the net wrench about the force-weighted centroid.  Everything is computed in float64 from the
values given; fields that are copies (dist, pos, normal, tangent, found, and the per-contact force components) come out as exactly the
float32 numbers that went in, so a caller may compare them bitwise after a cast to float32.
"""

import numpy as np

FIELDS = (("found", 1), ("force", 3), ("torque", 3), ("dist", 1), ("pos", 3), ("normal", 3), ("tangent", 3))
UNKNOWN, BODY, XBODY, GEOM, SITE = 0, 1, 2, 5, 6
NONE, MINDIST, MAXFORCE, NETFORCE = 0, 1, 2, 3
SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX = 2, 3, 4, 5, 6


def slot_layout(dataspec):
  """([(field, offset in the slot, floats)], floats per slot) of a dataspec bit mask."""
  out, off = [], 0
  for i, (name, n) in enumerate(FIELDS):
    if dataspec >> i & 1:
      out.append((name, off, n))
      off += n
  return out, off


def labels(dataspec, num):
  """Field name of every float of a sensor with `num` slots."""
  lay, size = slot_layout(dataspec)
  one = [None] * size
  for name, off, n in lay:
    one[off : off + n] = [name] * n
  return np.array(one * num)


def inside(stype, size, xpos, xmat, point):
  """Is `point` strictly inside the site volume (xmat: world-from-site rotation, 3 x 3)."""
  p = np.asarray(xmat, dtype=np.float64).reshape(3, 3).T @ (np.asarray(point, dtype=np.float64) - np.asarray(xpos, dtype=np.float64))
  s = np.asarray(size, dtype=np.float64)
  if stype == SPHERE:
    return p @ p < s[0] ** 2
  if stype == CAPSULE:
    dz = p[2] - np.clip(p[2], -s[1], s[1])
    return p[0] ** 2 + p[1] ** 2 + dz**2 < s[0] ** 2
  if stype == ELLIPSOID:
    return np.sum((p / s) ** 2) < 1.0
  if stype == CYLINDER:
    return abs(p[2]) < s[1] and p[0] ** 2 + p[1] ** 2 < s[0] ** 2
  if stype == BOX:
    return bool(np.all(np.abs(p) < s))
  return False


def _is_object(body_parentid, body, geom, objtype, objid):
  if objtype in (UNKNOWN, SITE):
    return True
  if objtype == GEOM:
    return geom == objid
  if objtype == BODY:
    return body == objid
  if objtype == XBODY:  # the subtree rooted at objid: bodies are numbered depth first
    while body > objid:
      body = body_parentid[body]
    return body == objid
  return False


def matches(objtype, objid, reftype, refid, geom_bodyid, body_parentid, site_type, site_size, site_xpos, site_xmat, pos, geom):
  """[(contact index, direction)] in contact order, uncapped."""
  out = []
  for c in range(len(geom)):
    if objtype == SITE and not inside(int(site_type[objid]), site_size[objid], site_xpos[objid], site_xmat[objid], pos[c]):
      continue
    direction = 1.0
    if objtype != UNKNOWN or reftype != UNKNOWN:
      g1, g2 = int(geom[c][0]), int(geom[c][1])
      b1, b2 = int(geom_bodyid[g1]), int(geom_bodyid[g2])
      m11, m12 = _is_object(body_parentid, b1, g1, objtype, objid), _is_object(body_parentid, b2, g2, objtype, objid)
      m21, m22 = _is_object(body_parentid, b1, g1, reftype, refid), _is_object(body_parentid, b2, g2, reftype, refid)
      if not (m11 or m12) or not (m21 or m22):
        continue
      if objtype != UNKNOWN and reftype != UNKNOWN:
        regular, reverse = m11 and m22, m12 and m21
        if not regular and not reverse:
          continue
        if reverse and not regular:
          direction = -1.0
      elif objtype != UNKNOWN:
        direction = 1.0 if m11 else -1.0
      else:
        direction = 1.0 if m22 else -1.0
    out.append((c, direction))
  return out


def criteria(reduce, kept, dist, force):
  """Sort keys of the kept matches (ascending)."""
  if reduce == MINDIST:
    return [np.float32(dist[c]) for c, _ in kept]
  f = np.asarray(force, dtype=np.float64)
  return [-(f[c, 0] ** 2 + f[c, 1] ** 2 + f[c, 2] ** 2) for c, _ in kept]


def sensor(objtype, objid, reftype, refid, intprm, geom_bodyid, body_parentid, site_type, site_size, site_xpos, site_xmat, dist, pos, frame, geom, force,
           maxmatch=64):
  """(float64 sensordata [num * slot size], overflowed) of one contact sensor in one world.

  dist [n] (float32 as published), pos [n, 3], frame [n, 3, 3] (rows: normal, tangent 1, tangent 2), geom [n, 2], force [n, 6] (contact
  frame: normal, two tangents, spin, two rolls), all in contact order.
  """
  dataspec, reduce, num = (int(x) for x in intprm)
  lay, size = slot_layout(dataspec)
  frame = np.asarray(frame).reshape(-1, 3, 3)
  found = matches(objtype, objid, reftype, refid, geom_bodyid, body_parentid, site_type, site_size, site_xpos, site_xmat, pos, geom)
  kept = found[:maxmatch]
  nmatch = len(kept)
  out = np.zeros(num * size, dtype=np.float64)
  if reduce == NETFORCE:
    wsum, centroid, fnet, tnet = 0.0, np.zeros(3), np.zeros(3), np.zeros(3)
    for c, direction in kept:
      f = np.asarray(force[c], dtype=np.float64)
      p = np.asarray(pos[c], dtype=np.float64)
      weight = np.linalg.norm(f[:3])
      centroid += weight * p
      wsum += weight
      fg = direction * (frame[c].astype(np.float64).T @ f[:3])
      fnet += fg
      tnet += direction * (frame[c].astype(np.float64).T @ f[3:]) + np.cross(p, fg)
    centroid /= max(wsum, 1e-15)
    tnet -= np.cross(centroid, fnet)
    value = {"found": [nmatch], "force": fnet, "torque": tnet, "dist": [0.0], "pos": centroid, "normal": [1.0, 0.0, 0.0], "tangent": [0.0, 1.0, 0.0]}
    for name, off, n in lay:
      out[off : off + n] = value[name]
    return out, len(found) > maxmatch
  if reduce in (MINDIST, MAXFORCE):
    key = criteria(reduce, kept, dist, force)
    kept = [kept[i] for i in sorted(range(nmatch), key=lambda i: key[i])]  # (sorted is stable)
  for slot, (c, direction) in enumerate(kept[:num]):
    f = np.asarray(force[c], dtype=np.float32)
    d32 = np.float32(direction)
    value = {"found": [nmatch], "force": [f[0], f[1], d32 * f[2]], "torque": [f[3], f[4], d32 * f[5]], "dist": [np.float32(dist[c])], "pos": np.asarray(pos[c], dtype=np.float32),
             "normal": d32 * frame[c][0].astype(np.float32), "tangent": d32 * frame[c][1].astype(np.float32)}
    for name, off, n in lay:
      out[slot * size + off : slot * size + off + n] = value[name]
  return out, len(found) > maxmatch
