// The lifter's matrix-pipe attention at the head sizes whose chunks are not 1 KB: HD = 16 (C = 128) and HD = 48 (C = 384).  Part of the
// translation unit of seq_attention_mfma.hip, whose kernel serves HD = 32 and 64.  The arithmetic of a head is that file's attention_head,
// called by both kernels: S^T = K Q^T in (hi, lo) planes with two accumulators, the exact two-pass softmax on log2-scaled scores, P split
// once per head, out^T = V^T P^T, the result pre-split, keys >= N at -inf, a non-finite result reported to the overflow sink.
//
// What differs is the work split.  A unit is still one sequence x 4 waves x whole heads, but a wave's strip of a row is 128 B (two heads
// of 16 channels) or 192 B (one head of 48): the unit's chunk is 512 B (the whole row at C = 128) or 768 B (half a row at C = 384).  Neither
// is what one LDS-DMA instruction moves (64 lanes x 16 B into consecutive LDS bytes), so K and V travel global -> registers -> LDS and are
// split on the way.  A wave reads only what it wrote - the strip holds whole heads - so its LDS region is private: no workgroup barrier,
// no counted wait, no ring; the waves of a workgroup share nothing but the unit's coordinates (and the cache lines of its rows).  The region
// is small (2 N rows of 144 / 208 B per wave, 32 KB per workgroup at most), so occupancy rather than a software pipeline hides the chain
// load -> split -> scores -> softmax -> P V -> store.
//
// Output blocks.  out^T has HD rows; the matrix tile has 32.  At HD = 16 rows 16..31 of the one tile, at HD = 48 rows 16..31 of the second,
// carry a clamped (repeated) channel and are not stored (attention_head) - the choice between that and a 16 x 16 x 32 tile is recorded in
// DESIGN.md section 3.
namespace {

template <int HD, int N>
struct LifterAttnCfg {
  static constexpr int C = 8 * HD;
  static constexpr int HPW = HD == 16 ? 2 : 1;  // heads per wave
  static constexpr int SWF = HPW * HD;          // floats of a row in a wave's strip: 32 / 48
  static constexpr int CHUNKF = 4 * SWF;        // floats of a row in a unit: 128 / 192
  static constexpr int UPS = C / CHUNKF;        // units per sequence: 1 / 2
  static constexpr int P4 = SWF / 4;            // 16-byte pieces of a strip row: 8 / 12
  static constexpr int RS = SWF * 4 + 16;       // LDS row stride in bytes: 9 / 13 sixteen-byte slots (odd: the rows a ds_read_b128 group touches spread over the banks)
  static constexpr int WAVE_BYTES = 2 * N * RS; // K rows, V rows of the strip
  static constexpr int QL = 2 * HeadCfg<HD, N>::KSTEPS * HPW;  // 16-byte Q loads per lane and unit
  static constexpr int KV = 2 * N * P4;         // 16-byte pieces of K and V per wave and unit
  static constexpr int NI = (KV + 63) / 64;
  static constexpr int OUTP = N * P4, NO = (OUTP + 63) / 64;
};

template <int HD, int N, bool OUT16>
__global__ __launch_bounds__(256) void lifter_attention_mfma_kernel(const float* __restrict__ qkv, float* __restrict__ out, int nseq,
                                                                  int seq_div, long long seq_lo, long long seq_hi,
                                                                  long long tok_stride, unsigned* oflow) {
  using Cfg = LifterAttnCfg<HD, N>;
  constexpr int C = Cfg::C, UPS = Cfg::UPS, HPW = Cfg::HPW, RS = Cfg::RS, P4 = Cfg::P4, QL = Cfg::QL;
  constexpr int KSTEPS = HeadCfg<HD, N>::KSTEPS;
  static_assert(HD % 16 == 0 && C % Cfg::CHUNKF == 0 && RS % 16 == 0, "whole 16-channel groups, whole units, 16-byte rows");
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * Cfg::WAVE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hb = lane >> 5;
  unsigned char* const U = smem + wave * Cfg::WAVE_BYTES;  // this wave's region: nobody else reads or writes it
  const int total = nseq * UPS;
  const int rowc = min(l31, N - 1);  // this lane's key row (A operand of K Q^T) and query row (B operand), clamped into the sequence

  bool bad = false;
  for (int u = (int)blockIdx.x; u < total; u += (int)gridDim.x) {
    const int seq = u / UPS, g = u - seq * UPS;
    const long long tb = (long long)(seq % seq_div) * seq_lo + (long long)(seq / seq_div) * seq_hi;
    const int col0 = g * Cfg::CHUNKF + wave * Cfg::SWF;  // the strip's first channel
    // ---- Q: row rowc, per head and k-step the 8 channels 16 ks + 8 hb + [0, 8) ----
    f32x4 qraw[QL];
    {
      const float* row = qkv + (tb + (long long)rowc * tok_stride) * (3 * C) + col0 + hb * 8;
#pragma unroll
      for (int i = 0; i < QL / 2; ++i) {  // i = head-in-wave * KSTEPS + ks: consecutive 16-channel groups of the strip
        qraw[2 * i] = *reinterpret_cast<const f32x4*>(row + i * 16);
        qraw[2 * i + 1] = *reinterpret_cast<const f32x4*>(row + i * 16 + 4);
      }
    }
    // ---- the strip of every K and V row: global -> registers -> planes in LDS ([16 hi | 16 lo*2^11] per 16 channels) ----
    {
      f32x4 x[Cfg::NI];
#pragma unroll
      for (int i = 0; i < Cfg::NI; ++i) {
        const int idx = min(lane + 64 * i, Cfg::KV - 1);  // (the tail repeats the last piece: loaded, not stored)
        const int r2 = idx / P4, piece = idx - r2 * P4;
        const int a = r2 / N, r = r2 - a * N;  // a = 0: K, 1: V
        x[i] = *reinterpret_cast<const f32x4*>(qkv + (tb + (long long)r * tok_stride) * (3 * C) + (a + 1) * C + col0 + piece * 4);
      }
      // the previous unit's result rows have left this region (a wave's LDS operations complete in order; the fence is for the compiler)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int i = 0; i < Cfg::NI; ++i) {
        const int idx = lane + 64 * i;
        const int r2 = idx / P4, piece = idx - r2 * P4;
        f16x4 xh, xl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xh[e] = (_Float16)x[i][e];
          xl[e] = lo_plane(x[i][e], xh[e]);
        }
        if (idx < Cfg::KV) {
          unsigned char* grp = U + r2 * RS + (piece >> 2) * 64 + (piece & 3) * 8;
          *reinterpret_cast<f16x4*>(grp) = xh;
          *reinterpret_cast<f16x4*>(grp + 32) = xl;
        }
      }
    }
    f16x8 qh[QL / 2], ql[QL / 2];
#pragma unroll
    for (int i = 0; i < QL / 2; ++i) split8_fused(qraw[2 * i], qraw[2 * i + 1], qh[i], ql[i]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int h = 0; h < HPW; ++h)  // h * HD * 4: this head's bytes inside a row of the strip
      attention_head<HD, N, RS, false>(U, h * (HD * 4), rowc, l31, hb, qh + h * KSTEPS, ql + h * KSTEPS, bad);
    // ---- the strip of every result row: LDS (written by other lanes of the wave) -> global, 16 bytes per lane ----
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < Cfg::NO; ++i) {
      const int idx = lane + 64 * i;
      const int row = idx / P4, piece = idx - row * P4;
      if (idx < Cfg::OUTP) {
        if constexpr (OUT16) {  // channels 4 piece + [0, 4) of the strip: the hi half of group piece >> 2, flushed (flush4_f16); 8 bytes per lane
          const f16x4 h = *reinterpret_cast<const f16x4*>(U + row * RS + (piece >> 2) * 64 + (piece & 3) * 8);
          *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(out) + (tb + (long long)row * tok_stride) * C + col0 + piece * 4) = flush4_f16(h);
        } else {
          const f32x4 t = *reinterpret_cast<const f32x4*>(U + row * RS + piece * 16);
          *reinterpret_cast<f32x4*>(out + (tb + (long long)row * tok_stride) * C + col0 + piece * 4) = t;
        }
      }
    }
  }
  report_nonfinite(oflow, bad);
}

template <int HD, int N, bool OUT16>
int launch_lifter_attention(const float* qkv, float* out, int nseq, int seq_div, long long seq_lo, long long seq_hi, long long tok_stride,
                            hipStream_t stream) {
  using Cfg = LifterAttnCfg<HD, N>;
  const long long units = (long long)nseq * Cfg::UPS;
  const int grid = units < 1024 ? (int)units : 1024;  // persistent beyond four workgroups per CU
  hipLaunchKernelGGL((lifter_attention_mfma_kernel<HD, N, OUT16>), dim3(grid), dim3(256), 0, stream, qkv, out, nseq, seq_div, seq_lo, seq_hi, tok_stride,
                     pmce_overflow_sink());
  return pmce_check_launch("lifter_attention_split_f16");
}

}  // namespace

// The lifter's matrix-pipe attention at every width the model accepts.  256 and 512 are pmce_seq_attention_split_f16 (forwarded: the same
// launch, the same bits); 128 and 384 are the kernel above.
extern "C" int pmce_lifter_attention_split_supported(int N, int C) {
  return (C == 128 || C == 256 || C == 384 || C == 512) && (N == 16 || N == 17 || N == 19) ? 1 : 0;
}

// out_form 1: the result pre-split [16 hi | 16 lo*2^11] per 16 channels in the bytes of the fp32 rows (the three-product GEMM's A operand);
// 2: plain f16 rows [token][C] - the hi plane with |x| < 2^-14 flushed to zero - the single-product GEMM's (half the bytes written).
extern "C" int pmce_lifter_attention_split_f16_form(const float* qkv, float* out, int nseq, int N, int C, int seq_div, long long seq_lo,
                                                    long long seq_hi, long long tok_stride, int out_form, hipStream_t stream) {
  PMCE_REQUIRE(qkv && out && nseq > 0, "lifter_attention_split_f16: bad arguments");
  PMCE_REQUIRE(pmce_lifter_attention_split_supported(N, C),
               "lifter_attention_split_f16: C must be 128, 256, 384 or 512 and N 16, 17 or 19 (got N=%d C=%d)", N, C);
  PMCE_REQUIRE(out_form == 1 || out_form == 2, "lifter_attention_split_f16: out_form is 1 (pre-split planes) or 2 (plain f16), got %d", out_form);
  if (C == 256 || C == 512) return seq_attention_split_form(qkv, out, nseq, N, C, seq_div, seq_lo, seq_hi, tok_stride, out_form, stream);
  if (seq_div <= 0) seq_div = 0x7fffffff;  // (as pmce_seq_attention_f32: sequence s starts at token s * seq_lo)
  PMCE_REQUIRE(tok_stride > 0 && (long long)nseq * 2 < (1ll << 31), "lifter_attention_split_f16: bad token stride or too many sequences");
#define PMCE_LATTN_CASE(HD_, N_)                                                                                                        \
  if (C == 8 * HD_ && N == N_)                                                                                                          \
  return out_form == 2 ? launch_lifter_attention<HD_, N_, true>(qkv, out, nseq, seq_div, seq_lo, seq_hi, tok_stride, stream)             \
                       : launch_lifter_attention<HD_, N_, false>(qkv, out, nseq, seq_div, seq_lo, seq_hi, tok_stride, stream)
  PMCE_LATTN_CASE(16, 16);
  PMCE_LATTN_CASE(16, 17);
  PMCE_LATTN_CASE(16, 19);
  PMCE_LATTN_CASE(48, 16);
  PMCE_LATTN_CASE(48, 17);
  PMCE_LATTN_CASE(48, 19);
#undef PMCE_LATTN_CASE
  return PMCE_OK;
}

// the pre-split form (the same launch, the same bits as before the form argument existed)
extern "C" int pmce_lifter_attention_split_f16(const float* qkv, float* out, int nseq, int N, int C, int seq_div, long long seq_lo,
                                               long long seq_hi, long long tok_stride, hipStream_t stream) {
  return pmce_lifter_attention_split_f16_form(qkv, out, nseq, N, C, seq_div, seq_lo, seq_hi, tok_stride, 1, stream);
}
