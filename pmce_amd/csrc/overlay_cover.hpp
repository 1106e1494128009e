// The coverage rules of the debug overlay (overlay.hip), written once for the device and for the host
// (scripts/overlay_cover_host.cpp runs them over cases from a file, so that the 128-bit arithmetic is checked against Python integers
// without a GPU).  Everything after the quantisation is integer arithmetic, evaluated exactly.
//
// Units.  A coordinate v in pixels becomes q = rint(16 v): 4 sub-pixel bits, ties to even (16 v is exact in fp64).  Pixel (x, y) has its
// centre at (16 x + 8, 16 y + 8).  The callers drop what lies beyond the guard band |v| > 2^14 px, so |q| <= 2^18; frames are at most
// 8192 wide and high, so a pixel centre is below 2^17 + 8.  With d = b - a and p = c - a every component is below 2^19 + 2^17, d.d and
// p.d are below 2^40, and |p|^2 (d.d) is below 2^81: the one product that needs 128 bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OVERLAY_HD __host__ __device__ __forceinline__
#else
#define OVERLAY_HD inline
#endif

namespace overlay_cover {

constexpr int SUB_BITS = 4;
constexpr int SUB_ONE = 1 << SUB_BITS;   // units per pixel
constexpr int SUB_HALF = SUB_ONE / 2;    // a pixel centre inside its pixel
constexpr double GUARD_PX = 16384.0;     // 2^14
constexpr int MAX_THICKNESS = 64, MAX_RADIUS = 64;

// v is finite and inside the guard band (the callers test both first)
OVERLAY_HD int quantise(double v) { return (int)rint(v * (double)SUB_ONE); }

// also true for a NaN
OVERLAY_HD bool beyond_guard(double v) { return !(fabs(v) <= GUARD_PX); }

OVERLAY_HD int pixel_centre(int x) { return x * SUB_ONE + SUB_HALF; }

// the pixels whose centres lie in [lo, hi] units, clipped to [0, n - 1]: empty when p1 < p0
OVERLAY_HD void centre_span(int lo, int hi, int n, int& p0, int& p1) {
  p0 = (lo + SUB_HALF - 1) >> SUB_BITS;
  p1 = (hi - SUB_HALF) >> SUB_BITS;
  if (p0 < 0) p0 = 0;
  if (p1 > n - 1) p1 = n - 1;
}

// the centre (cx, cy) lies within 8 t units (half a line of thickness t pixels) of the segment a -> b
OVERLAY_HD bool segment_covers(int ax, int ay, int bx, int by, int cx, int cy, int thickness) {
  const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay;
  const int64_t px = (int64_t)cx - ax, py = (int64_t)cy - ay;
  const int64_t r2 = (int64_t)(SUB_HALF * thickness) * (SUB_HALF * thickness);
  const int64_t L = dx * dx + dy * dy, s = px * dx + py * dy, pp = px * px + py * py;
  if (L == 0 || s <= 0) return pp <= r2;
  if (s >= L) {
    const int64_t ex = (int64_t)cx - bx, ey = (int64_t)cy - by;
    return ex * ex + ey * ey <= r2;
  }
  // |p|^2 - s^2 / L <= r^2, cleared of the division; 0 < s < L, so s^2 < L^2 < 2^80
  return (__int128)pp * L - (__int128)s * s <= (__int128)r2 * L;
}

// the centre lies within `radius` pixels of the keypoint k
OVERLAY_HD bool disc_covers(int kx, int ky, int cx, int cy, int radius) {
  const int64_t ex = (int64_t)cx - kx, ey = (int64_t)cy - ky;
  const int64_t r = (int64_t)SUB_ONE * radius;
  return ex * ex + ey * ey <= r * r;
}

}  // namespace overlay_cover
