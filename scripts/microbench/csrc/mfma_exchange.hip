// Diagnostics: is v_mfma_f32_32x32x16_f16 bit-symmetric in its two operands?  One 64 x 64 x K product in the three-product f16 form
// (pre-split A, blocked packed W, the k order and product order of gemm_split_kernel), computed twice by every wave: with the
// activation fragment as the A operand (the GEMM's form: lane = column, registers = rows) and with the operands exchanged (lane = row,
// registers = columns - the form the fused qkv + attention kernel uses for q and k).  Both results are written as [64][64] fp32;
// tests/test_gpu_qkv_attention_fused.py compares them bitwise, and with the product kernel's result.
#include "common.hpp"

namespace {
__global__ __launch_bounds__(256) void mfma_exchange_kernel(const float* __restrict__ Ap, const float* __restrict__ Wp,
                                                            const float* __restrict__ wscale, float* __restrict__ out_plain,
                                                            float* __restrict__ out_exch, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave & 1, wn = wave >> 1, n0 = lane & 31, hb = lane >> 5;
  f32x16 plain, exch;
#pragma unroll
  for (int r = 0; r < 16; ++r) plain[r] = exch[r] = 0.f;
  const _Float16* a = reinterpret_cast<const _Float16*>(Ap) + (size_t)(wm * 32 + n0) * (K / 16) * 32 + 8 * hb;
  const _Float16* w = reinterpret_cast<const _Float16*>(Wp) + (size_t)(wn * 32 + n0) * 32 + 8 * hb;
  for (int kt = 0; kt < K / 16; ++kt) {
    const f16x8 ahi = *reinterpret_cast<const f16x8*>(a + kt * 32), alo = *reinterpret_cast<const f16x8*>(a + kt * 32 + 16);
    const f16x8 whi = *reinterpret_cast<const f16x8*>(w + (size_t)kt * 64 * 32), wlo = *reinterpret_cast<const f16x8*>(w + (size_t)kt * 64 * 32 + 16);
    const f16x8 wh2 = whi * (_Float16)0.00048828125f;
    plain = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, whi, plain, 0, 0, 0);
    plain = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, wlo, plain, 0, 0, 0);
    plain = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, wh2, plain, 0, 0, 0);
    exch = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi, ahi, exch, 0, 0, 0);
    exch = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo, ahi, exch, 0, 0, 0);
    exch = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh2, alo, exch, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = 4 * hb + (r & 3) + 8 * (r >> 2);
    out_plain[(wm * 32 + i) * 64 + wn * 32 + n0] = plain[r] * wscale[wn * 32 + n0];
    out_exch[(wm * 32 + n0) * 64 + wn * 32 + i] = exch[r] * wscale[wn * 32 + i];
  }
}
}  // namespace

// Ap: pre-split [64][K/16][16 hi | 16 lo*2^11] f16; Wp / wscale: pmce_gemm_pack_split_f16(blocked = 1) of a [64][K] weight; outputs [64][64]
extern "C" int pmce_dbg_mfma_exchange(const float* Ap, const float* Wp, const float* wscale, float* out_plain, float* out_exch, int K,
                                      hipStream_t stream) {
  PMCE_REQUIRE(Ap && Wp && wscale && out_plain && out_exch && K >= 16 && K % 16 == 0, "dbg_mfma_exchange: bad arguments");
  hipLaunchKernelGGL(mfma_exchange_kernel, dim3(1), dim3(256), 0, stream, Ap, Wp, wscale, out_plain, out_exch, K);
  return pmce_check_launch("dbg_mfma_exchange");
}
