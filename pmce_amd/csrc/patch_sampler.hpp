// The sampling body shared by the person crops (crops.hip: pmce_crop_patches, S x S) and the 2D pose stage's patches (pose2d.hip:
// pmce_pose_patches, SH x SW): an axis-aligned inverse map x_src = ix x_dst + tx, y_src = iy y_dst + ty, sampled by the fixed-point
// bilinear rule that OpenCV documents for warpAffine(INTER_LINEAR, BORDER_CONSTANT) on 8-bit images (include/pmce_hip.h, the crops
// section, states it), then normalised through the 3 x 256 table.  Integer arithmetic from the four coefficients on.
//
// A wavefront owns one output row at a time: its lanes take four adjacent x each, so that every plane row leaves as contiguous 16-byte
// stores, and everything that depends on the row alone (the source rows, their validity, the vertical fraction) is computed once per row
// and is wave-uniform.  What depends on the column alone (tap column, horizontal fraction) is computed once per lane and kept across the
// rows of the workgroup's band.
#pragma once
#include "common.hpp"

namespace patch_sampler {

constexpr int MAX_SIDE = 1024;       // output width / height
constexpr int MAX_DIM = 16384;       // frame width / height
constexpr int ROWS_PER_BLOCK = 32;   // output rows of one workgroup: 8 per wave
constexpr double COORD_LIMIT = 1048576.0;   // 2^20 px

__device__ __forceinline__ bool in_reach(double v) { return fabs(v) <= COORD_LIMIT; }   // false for NaN and inf

// One quad of one output row: planes of[c][y][x0..x0+3] and bytes ou[y][x0..x0+3][c].  ALIGNED: SW % 4 == 0, every quad is whole and
// 16-byte aligned.
template <bool ALIGNED>
__device__ __forceinline__ void store_quad(float* __restrict__ of, unsigned char* __restrict__ ou, size_t plane, int SW, int y, int x0,
                                           const float (&r)[3][4], const unsigned char (&u)[4][3]) {
  const size_t o = (size_t)y * SW + x0;
  if (ALIGNED) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(of + c * plane + o) = f32x4{r[c][0], r[c][1], r[c][2], r[c][3]};
    if (ou) {
      uint32_t wds[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= (uint32_t)u[(4 * k + j) / 3][(4 * k + j) % 3] << (8 * j);
        wds[k] = v;
      }
      uint32_t* d = reinterpret_cast<uint32_t*>(ou + o * 3);
      d[0] = wds[0];
      d[1] = wds[1];
      d[2] = wds[2];
    }
  } else {
    const int ne = min(4, SW - x0);
    for (int e = 0; e < ne; ++e) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        of[c * plane + o + e] = r[c][e];
        if (ou) ou[(o + e) * 3 + c] = u[e][c];
      }
    }
  }
}

// The rows [y_begin, y_end) of one job's SH x SW patch, by the 256 threads of a workgroup.  `live` false: the all-border patch, no frame
// is read.  lut: the table in LDS.  of / ou: this job's planes [3][SH][SW] and bytes [SH][SW][3] (ou may be null).  MIRROR: of_m / ou_m
// receive the same patch mirrored in x (column SW - 1 - x).
template <bool ALIGNED, bool MIRROR>
__device__ __forceinline__ void sample_rows(const unsigned char* __restrict__ frame, int H, int W, bool live, double ix, double tx,
                                            double iy, double ty, int SH, int SW, int y_begin, int y_end, int swap_rb,
                                            const float* lut, float* __restrict__ of, unsigned char* __restrict__ ou,
                                            float* __restrict__ of_m, unsigned char* __restrict__ ou_m) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t plane = (size_t)SH * SW;
  const long long X0 = live ? (long long)rint(tx * 1024.0) + 16 : 0;
  const int c_r = swap_rb ? 2 : 0, c_b = swap_rb ? 0 : 2;     // source byte of output channels 0 and 2
  const int quads = (SW + 3) >> 2;

  for (int q = lane; q < quads; q += 64) {
    const int x0 = q * 4;
    int Xs[4];                                   // per column: (tap column << 5) | fraction
#pragma unroll
    for (int e = 0; e < 4; ++e) Xs[e] = live ? (int)((X0 + (long long)rint(ix * (double)(x0 + e) * 1024.0)) >> 5) : 0;
    for (int y = y_begin + wave; y < y_end; y += 4) {
      float r[3][4];
      unsigned char u[4][3];
      if (live) {
        const long long Yl = ((long long)rint((iy * (double)y + ty) * 1024.0) + 16) >> 5;
        const int Y = __builtin_amdgcn_readfirstlane((int)Yl);
        const int row = Y >> 5, b = Y & 31;
        const bool v0 = row >= 0 && row < H, v1 = row + 1 >= 0 && row + 1 < H;
        const unsigned char* p0 = frame + (size_t)min(max(row, 0), H - 1) * W * 3;
        const unsigned char* p1 = frame + (size_t)min(max(row + 1, 0), H - 1) * W * 3;
        const int wb0 = v0 ? 32 - b : 0, wb1 = v1 ? b : 0;      // a row outside the frame contributes nothing
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = Xs[e] >> 5, a = Xs[e] & 31;
          const int o0 = min(max(col, 0), W - 1) * 3, o1 = min(max(col + 1, 0), W - 1) * 3;
          const int wa0 = (col >= 0 && col < W) ? 32 - a : 0, wa1 = (col + 1 >= 0 && col + 1 < W) ? a : 0;
          const int w00 = wb0 * wa0 * 32, w01 = wb0 * wa1 * 32, w10 = wb1 * wa0 * 32, w11 = wb1 * wa1 * 32;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int sc = c == 0 ? c_r : (c == 2 ? c_b : 1);
            const int sum = w00 * p0[o0 + sc] + w01 * p0[o1 + sc] + w10 * p1[o0 + sc] + w11 * p1[o1 + sc];
            const int v = (sum + 16384) >> 15;
            u[e][c] = (unsigned char)v;
            r[c][e] = lut[c * 256 + v];
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            u[e][c] = 0;
            r[c][e] = lut[c * 256];
          }
      }
      store_quad<ALIGNED>(of, ou, plane, SW, y, x0, r, u);
      if (MIRROR) {
        if (ALIGNED) {                           // the mirrored quad is whole and aligned too: columns SW - 4 - x0 .. SW - 1 - x0
          float rm[3][4];
          unsigned char um[4][3];
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              rm[c][e] = r[c][3 - e];
              um[e][c] = u[3 - e][c];
            }
          store_quad<true>(of_m, ou_m, plane, SW, y, SW - 4 - x0, rm, um);
        } else {
          const int ne = min(4, SW - x0);
          for (int e = 0; e < ne; ++e) {
            const size_t o = (size_t)y * SW + (SW - 1 - x0 - e);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              of_m[c * plane + o] = r[c][e];
              if (ou_m) ou_m[o * 3 + c] = u[e][c];
            }
          }
        }
      }
    }
  }
}

}  // namespace patch_sampler
