// ls_bracket_host.cpp -- host check of the line search's bracket-end update (tests/test_host.py compiles and runs it).
// bracket_update (csrc/linesearch.hpp: three keys, one minimum, one select) against a restatement of the reference's chained
// update (solver.py:1222-1290: in_bracket + take, three candidates in turn) over a grid of (end, y1, y2, y3) derivatives:
// the selected candidate (c, g, h, alpha) and the "end moved" flag must be bitwise equal in every case.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "linesearch.hpp"

static bool in_bracket(const P3& x, const P3& y) { return (x.g < y.g && y.g < 0.0f) || (x.g > y.g && y.g > 0.0f); }
static void take(bool c, P3& dst, float& da, const P3& src, float sa) {
  dst.c = c ? src.c : dst.c;
  dst.g = c ? src.g : dst.g;
  dst.h = c ? src.h : dst.h;
  da = c ? sa : da;
}
static bool chain_update(P3& end, float& end_a, const P3& y1, float a1, const P3& y2, float a2, const P3& y3, float a3) {
  const bool s1 = in_bracket(end, y1);
  take(s1, end, end_a, y1, a1);
  const bool s2 = in_bracket(end, y2);
  take(s2, end, end_a, y2, a2);
  const bool s3 = in_bracket(end, y3);
  take(s3, end, end_a, y3, a3);
  return s1 || s2 || s3;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float den = std::numeric_limits<float>::denorm_min(), big = std::nextafterf(3.0e38f, 0.0f);  // just below the key's sentinel
  // both signs and both zeros, a denormal, ordinary magnitudes (every value occurs in every slot: ties, candidates beyond the end and
  // on the far side of zero), the largest magnitudes below 3.0e38, the infinities and NaN
  const float v[] = {0.0f, -0.0f, den, -den, 0.5f, -0.5f, 1.0f, -1.0f, 2.0f, -2.0f, 2.9e38f, -2.9e38f, big, -big, inf, -inf, nan};
  const int n = sizeof(v) / sizeof(v[0]);
  long cases = 0, bad = 0, moved = 0;
  for (int i0 = 0; i0 < n; ++i0)
    for (int i1 = 0; i1 < n; ++i1)
      for (int i2 = 0; i2 < n; ++i2)
        for (int i3 = 0; i3 < n; ++i3) {
          // (cost, curvature and step size differ per slot, so that the bits tell WHICH candidate was taken)
          const P3 y1 = P3{1.0f, v[i1], 11.0f}, y2 = P3{2.0f, v[i2], 12.0f}, y3 = P3{3.0f, v[i3], 13.0f};
          P3 ea = P3{0.0f, v[i0], 10.0f}, eb = ea;
          float aa = 20.0f, ab = 20.0f;
          const bool fa = chain_update(ea, aa, y1, 21.0f, y2, 22.0f, y3, 23.0f);
          const bool fb = bracket_update(eb, ab, y1, 21.0f, y2, 22.0f, y3, 23.0f);
          ++cases;
          moved += fa;
          if (fa != fb || std::memcmp(&ea, &eb, sizeof(P3)) != 0 || std::memcmp(&aa, &ab, sizeof(float)) != 0) {
            if (bad++ < 10)
              std::printf("differs: end %g  candidates %g %g %g: chain -> alpha %g moved %d, bracket_update -> alpha %g moved %d\n", v[i0], v[i1], v[i2],
                          v[i3], aa, (int)fa, ab, (int)fb);
          }
        }
  std::printf("%ld cases, %ld moved the end, %ld differ\n", cases, moved, bad);
  return bad ? 1 : 0;
}
