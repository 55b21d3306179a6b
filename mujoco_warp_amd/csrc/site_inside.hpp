// site_inside.hpp -- the point-in-site-volume test shared by the contact sensors (csrc/sensor_contact.hpp: contacts inside a site) and the
// insidesite sensor (csrc/sensor.hpp).
#pragma once
#include "dev_common.hpp"

// util_misc.py:676-705 inside_geom: is the point strictly inside the site's volume
DEV bool cs_inside(int type, V3 size, V3 pos, const float* mat, V3 point) {
  const V3 vec = point - pos;
  if (type == G_SPHERE) return dot(vec, vec) < size.x * size.x;
  const V3 p = matT_mul(mat, vec);
  if (type == G_CAPSULE) {
    const float zd = p.z - fminf(fmaxf(p.z, -size.y), size.y);
    return p.x * p.x + p.y * p.y + zd * zd < size.x * size.x;
  }
  if (type == G_ELLIPSOID) {
    const V3 q = V3{p.x / size.x, p.y / size.y, p.z / size.z};
    return dot(q, q) < 1.0f;
  }
  if (type == G_CYLINDER) return fabsf(p.z) < size.y && p.x * p.x + p.y * p.y < size.x * size.x;
  if (type == G_BOX) return fabsf(p.x) < size.x && fabsf(p.y) < size.y && fabsf(p.z) < size.z;
  if (type == G_PLANE) return p.z < 0.0f;
  return false;
}
