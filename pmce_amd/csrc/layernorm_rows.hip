// nn.LayerNorm over rows of any width C with C % 16 == 0 and C <= 2048 (pmce_ln_chain_f32 serves the lifter's 256 and 512 only), with the
// optional broadcast addend of a ViT's position embedding in front:
//     y = x + add[row % add_mod]      (add == null: y = x);      out1 = y (optional: the new residual stream; may be x itself);
//     out  = LN(y; w, b, eps)         fp32, or pre-split [row][C/16][16 hi | 16 lo*2^11] f16 - the A operand of a three-product f16 GEMM,
//                                     or (pmce_layernorm_rows_f16) plain f16 [row][C], each value rounded once by r16 - gemm_f16.hip's.
// One wave per row, the row in registers (up to eight 16-byte pieces per lane); two-pass fp32 statistics: the mean, then the mean of
// the squared deviations (biased, as nn.LayerNorm), each summed in-lane in piece order and then across the wave - a row's result
// depends on nothing but the row.
#include "gemm_split_common.hpp"

namespace {

constexpr int LN_MAX_PIECES = 8;  // 64 lanes x 8 x 4 floats = 2048 channels

template <int NP>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* x, long long rows, int C, const float* __restrict__ add,
                                                             int add_mod, float* out1, const float* __restrict__ w,
                                                             const float* __restrict__ b, float eps, float* __restrict__ out, int out_split) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c4 = C >> 2;  // 16-byte pieces per row
  const float* xr = x + row * C;
  const float* ar = add ? add + (long long)(row % add_mod) * C : nullptr;
  f32x4 v[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int p = lane + 64 * i;
    v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p < c4) {
      v[i] = *reinterpret_cast<const f32x4*>(xr + 4 * p);
      if (ar) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(ar + 4 * p);
        v[i] = f32x4{v[i].x + a.x, v[i].y + a.y, v[i].z + a.z, v[i].w + a.w};
      }
    }
  }
  if (out1) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = lane + 64 * i;
      if (p < c4) *reinterpret_cast<f32x4*>(out1 + row * C + 4 * p) = v[i];
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);  // (the pieces past the row hold zeros)
  const float mean = wave_sum(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int p = lane + 64 * i;
    if (p < c4) {
      const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
      ss += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  // A variance beyond fp32 (one |x| past 1.8e19) makes the row NaN like any other overflow: 1 / sqrt(inf) = 0 would return b, a finite row
  // that no check downstream could tell from a result.  Every finite variance takes the same arithmetic as before.
  const float var = wave_sum(ss) / (float)C;
  const float inv = var <= 3.402823466e+38f ? 1.0f / sqrtf(var + eps) : __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int p = lane + 64 * i;
    if (p < c4) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(w + 4 * p);
      const f32x4 be = *reinterpret_cast<const f32x4*>(b + 4 * p);
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * inv * g[e] + be[e];
      if (out_split == 2) {  // plain f16 [rows][C], each value rounded once by r16: the A operand of gemm_f16.hip
        f16x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = r16(pinned(y[e]));
        *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(out) + row * C + 4 * p) = h;
      } else if (out_split) store4_split_f16(out + row * C, 4 * p, y);
      else *reinterpret_cast<f32x4*>(out + row * C + 4 * p) = y;
    }
  }
}

// out_form: 0 fp32, 1 planes, 2 plain f16
int layernorm_rows_any(const float* x, long long rows, int C, const float* add, int add_mod, float* out1, const float* w, const float* b, float eps,
                       float* out, int out_split, hipStream_t stream) {
  PMCE_REQUIRE(x && w && b && out, "layernorm_rows: null pointer");
  PMCE_REQUIRE(C >= 16 && C % 16 == 0 && C <= 64 * 4 * LN_MAX_PIECES, "layernorm_rows: C must be a multiple of 16 in 16..2048 (got C=%d)", C);
  PMCE_REQUIRE(rows >= 1 && (rows + 3) / 4 < (1ll << 31), "layernorm_rows: rows must be in 1..2^33 (got %lld)", rows);
  PMCE_REQUIRE(!add || add_mod >= 1, "layernorm_rows: an addend needs add_mod >= 1 (got %d)", add_mod);
  PMCE_REQUIRE(eps > 0.f, "layernorm_rows: eps must be positive");
  const uintptr_t all = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(add) | reinterpret_cast<uintptr_t>(out1) |
                        reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out);
  PMCE_REQUIRE((all & 15) == 0, "layernorm_rows: every buffer must be 16-byte aligned");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  const int np = (C / 4 + 63) / 64;
#define PMCE_LN_CASE(NP_) \
  if (np <= NP_) { \
    hipLaunchKernelGGL((layernorm_rows_kernel<NP_>), grid, block, 0, stream, x, rows, C, add, add_mod, out1, w, b, eps, out, out_split); \
    return pmce_check_launch("layernorm_rows"); \
  }
  PMCE_LN_CASE(1)
  PMCE_LN_CASE(2)
  PMCE_LN_CASE(4)
  PMCE_LN_CASE(5)
  PMCE_LN_CASE(8)
#undef PMCE_LN_CASE
  return PMCE_OK;
}

}  // namespace

extern "C" int pmce_layernorm_rows_f32(const float* x, long long rows, int C, const float* add, int add_mod, float* out1, const float* w,
                                       const float* b, float eps, float* out, int out_split, hipStream_t stream) {
  return layernorm_rows_any(x, rows, C, add, add_mod, out1, w, b, eps, out, out_split ? 1 : 0, stream);
}

// The same statistics and the same fp32 result, stored as r16(y) in plain f16 [rows][C] (the single-product f16 mode's operand).
extern "C" int pmce_layernorm_rows_f16(const float* x, long long rows, int C, const float* add, int add_mod, float* out1, const float* w,
                                       const float* b, float eps, void* out16, hipStream_t stream) {
  return layernorm_rows_any(x, rows, C, add, add_mod, out1, w, b, eps, static_cast<float*>(out16), 2, stream);
}
