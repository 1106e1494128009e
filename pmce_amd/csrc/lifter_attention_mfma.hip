// The lifter's matrix-pipe attention at the head sizes whose chunks are not 1 KB: HD = 16 (C = 128) and HD = 48 (C = 384).  Part of the
// translation unit of seq_attention_mfma.hip, whose kernel serves HD = 32 and 64 and whose arithmetic this one repeats statement by
// statement: S^T = K Q^T in (hi, lo) planes with two accumulators, the exact two-pass softmax on log2-scaled scores, P split once per
// head, out^T = V^T P^T, the result pre-split, keys >= N at -inf, a non-finite result reported to the overflow sink.
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
// carry a clamped (repeated) channel and are not stored - the choice between that and a 16 x 16 x 32 tile is recorded in DESIGN.md section 3.
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
  static constexpr int KSTEPS = HD / 16, DBLK = (HD + 31) / 32, PSTEPS = N > 16 ? 2 : 1;
  static constexpr int QL = 2 * KSTEPS * HPW;   // 16-byte Q loads per lane and unit
  static constexpr int KV = 2 * N * P4;         // 16-byte pieces of K and V per wave and unit
  static constexpr int NI = (KV + 63) / 64;
  static constexpr int OUTP = N * P4, NO = (OUTP + 63) / 64;
};

template <int HD, int N>
__global__ __launch_bounds__(256) void lifter_attention_mfma_kernel(const float* __restrict__ qkv, float* __restrict__ out, int nseq,
                                                                  int seq_div, long long seq_lo, long long seq_hi,
                                                                  long long tok_stride, unsigned* oflow) {
  using Cfg = LifterAttnCfg<HD, N>;
  constexpr int C = Cfg::C, UPS = Cfg::UPS, HPW = Cfg::HPW, RS = Cfg::RS, P4 = Cfg::P4, QL = Cfg::QL;
  static_assert(HD % 16 == 0 && C % Cfg::CHUNKF == 0 && RS % 16 == 0, "whole 16-channel groups, whole units, 16-byte rows");
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * Cfg::WAVE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hb = lane >> 5;
  unsigned char* const U = smem + wave * Cfg::WAVE_BYTES;  // this wave's region: nobody else reads or writes it
  const int total = nseq * UPS;
  const int rowc = min(l31, N - 1);  // this lane's key row (A operand of K Q^T) and query row (B operand), clamped into the sequence

  // hd^-0.5 * log2(e): scores in log2 units, softmax on the hardware 2^x
  constexpr float scale = (HD == 16 ? 0.25f : 0.14433756729740643f) * 1.44269504088896340736f;
  constexpr float two_m11 = 0.00048828125f;
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
    for (int h = 0; h < HPW; ++h) {
      const int hoff = h * (HD * 4);  // this head's bytes inside a row of the strip
      const unsigned char* pk = U + rowc * RS + hoff + hb * 16;
      f16x8 kh[Cfg::KSTEPS], kl[Cfg::KSTEPS];
#pragma unroll
      for (int ks = 0; ks < Cfg::KSTEPS; ++ks) {
        kh[ks] = *reinterpret_cast<const f16x8*>(pk + ks * 64);
        kl[ks] = *reinterpret_cast<const f16x8*>(pk + ks * 64 + 32);
      }
      f16x8 vh[Cfg::DBLK][Cfg::PSTEPS], vl[Cfg::DBLK][Cfg::PSTEPS];
#pragma unroll
      for (int blk = 0; blk < Cfg::DBLK; ++blk) {
        // f16 index of channel ch = 32 blk + l31 inside the row's planes: group ch >> 4 of 32 halves, hi at ch & 15, lo 16 further; the rows of
        // the tile past the head's last channel repeat that channel (computed, never stored)
        const int ch = min(32 * blk + l31, HD - 1);
        const _Float16* pv = reinterpret_cast<const _Float16*>(U + N * RS + hoff) + (ch >> 4) * 32 + (ch & 15);
#pragma unroll
        for (int s = 0; s < Cfg::PSTEPS; ++s) {
          // keys 16.. exist only up to N - 1 (and only in the hb = 0 half): the other slots carry p = 0 and may hold any finite v
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int key = 16 * s + (e & 3) + 8 * (e >> 2);  // + 4 hb
            if (s == 0 || key < N) {
              const _Float16* pr = pv + (size_t)min(key + 4 * hb, N - 1) * (RS / 2);
              vh[blk][s][e] = pr[0];
              vl[blk][s][e] = pr[16];
            } else {
              vh[blk][s][e] = vh[blk][s][0];
              vl[blk][s][e] = vl[blk][s][0];
            }
          }
        }
      }
      // ---- S^T = K Q^T ----
      f32x16 s_main, s_cross;
#pragma unroll
      for (int r = 0; r < 16; ++r) s_main[r] = s_cross[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < Cfg::KSTEPS; ++ks) {
        s_main = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[ks], qh[h * Cfg::KSTEPS + ks], s_main, 0, 0, 0);
        s_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[ks], ql[h * Cfg::KSTEPS + ks], s_cross, 0, 0, 0);
        s_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl[ks], qh[h * Cfg::KSTEPS + ks], s_cross, 0, 0, 0);
      }
      // ---- softmax over the keys of this lane's query: register r is key 4 hb + (r & 3) + 8 (r >> 2) ----
      float p[16];
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = 4 * hb + (r & 3) + 8 * (r >> 2);
        const float sv = fmaf(s_cross[r], two_m11, s_main[r]) * scale;
        p[r] = (r < 8 || N > 16) ? (key < N ? sv : -INFINITY) : -INFINITY;  // (N <= 16: registers 8..15 are keys >= 16)
        mx = fmaxf(mx, p[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = __builtin_amdgcn_exp2f(p[r] - mx);
        sum += p[r];
      }
      sum += __shfl_xor(sum, 32);
      const float inv = 1.0f / sum;
      // ---- out^T = V^T P^T, one 32-channel block at a time; P split once for the head ----
      f16x8 ph[Cfg::PSTEPS], pl[Cfg::PSTEPS];
#pragma unroll
      for (int s = 0; s < Cfg::PSTEPS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float pv32 = pinned(p[8 * s + e]);
          ph[s][e] = (_Float16)pv32;
          pl[s][e] = lo_plane(pv32, ph[s][e]);
        }
#pragma unroll
      for (int blk = 0; blk < Cfg::DBLK; ++blk) {
        f32x16 o_main, o_cross;
#pragma unroll
        for (int r = 0; r < 16; ++r) o_main[r] = o_cross[r] = 0.f;
#pragma unroll
        for (int s = 0; s < Cfg::PSTEPS; ++s) {
          o_main = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[blk][s], ph[s], o_main, 0, 0, 0);
          o_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[blk][s], pl[s], o_cross, 0, 0, 0);
          o_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl[blk][s], ph[s], o_cross, 0, 0, 0);
        }
        // register r is channel 32 blk + 4 hb + (r & 3) + 8 (r >> 2) of query l31: four consecutive channels per r >> 2, written
        // pre-split into this head's bytes of the (dead) K row of that query; the quads past the head's last channel are dropped
        if (l31 < N) {
          unsigned char* po = U + l31 * RS + hoff;
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            if (32 * blk + 8 * rq >= HD) continue;
            f16x4 oh, ol;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = pinned(fmaf(o_cross[4 * rq + e], two_m11, o_main[4 * rq + e]) * inv);
              bad = bad || nonfinite(v);
              oh[e] = (_Float16)v;
              ol[e] = lo_plane(v, oh[e]);
            }
            const int g16 = 2 * blk + (rq >> 1), idx = 8 * (rq & 1) + 4 * hb;
            *reinterpret_cast<f16x4*>(po + g16 * 64 + idx * 2) = oh;
            *reinterpret_cast<f16x4*>(po + g16 * 64 + 32 + idx * 2) = ol;
          }
        }
      }
    }
    // ---- the strip of every result row: LDS (written by other lanes of the wave) -> global, 16 bytes per lane ----
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < Cfg::NO; ++i) {
      const int idx = lane + 64 * i;
      const int row = idx / P4, piece = idx - row * P4;
      if (idx < Cfg::OUTP) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(U + row * RS + piece * 16);
        *reinterpret_cast<f32x4*>(out + (tb + (long long)row * tok_stride) * C + col0 + piece * 4) = t;
      }
    }
  }
  report_nonfinite(oflow, bad);
}

template <int HD, int N>
int launch_lifter_attention(const float* qkv, float* out, int nseq, int seq_div, long long seq_lo, long long seq_hi, long long tok_stride,
                            hipStream_t stream) {
  using Cfg = LifterAttnCfg<HD, N>;
  const long long units = (long long)nseq * Cfg::UPS;
  const int grid = units < 1024 ? (int)units : 1024;  // persistent beyond four workgroups per CU
  hipLaunchKernelGGL((lifter_attention_mfma_kernel<HD, N>), dim3(grid), dim3(256), 0, stream, qkv, out, nseq, seq_div, seq_lo, seq_hi, tok_stride,
                     pmce_overflow_sink());
  return pmce_check_launch("lifter_attention_split_f16");
}

}  // namespace

// The lifter's matrix-pipe attention at every width the model accepts.  256 and 512 are pmce_seq_attention_split_f16 (forwarded: the same
// launch, the same bits); 128 and 384 are the kernel above.
extern "C" int pmce_lifter_attention_split_supported(int N, int C) {
  return (C == 128 || C == 256 || C == 384 || C == 512) && (N == 16 || N == 17 || N == 19) ? 1 : 0;
}

extern "C" int pmce_lifter_attention_split_f16(const float* qkv, float* out, int nseq, int N, int C, int seq_div, long long seq_lo,
                                               long long seq_hi, long long tok_stride, hipStream_t stream) {
  PMCE_REQUIRE(qkv && out && nseq > 0, "lifter_attention_split_f16: bad arguments");
  PMCE_REQUIRE(pmce_lifter_attention_split_supported(N, C),
               "lifter_attention_split_f16: C must be 128, 256, 384 or 512 and N 16, 17 or 19 (got N=%d C=%d)", N, C);
  if (C == 256 || C == 512) return pmce_seq_attention_split_f16(qkv, out, nseq, N, C, seq_div, seq_lo, seq_hi, tok_stride, stream);
  if (seq_div <= 0) seq_div = 0x7fffffff;  // (as pmce_seq_attention_f32: sequence s starts at token s * seq_lo)
  PMCE_REQUIRE(tok_stride > 0 && (long long)nseq * 2 < (1ll << 31), "lifter_attention_split_f16: bad token stride or too many sequences");
#define PMCE_LATTN_CASE(HD_, N_) \
  if (C == 8 * HD_ && N == N_) return launch_lifter_attention<HD_, N_>(qkv, out, nseq, seq_div, seq_lo, seq_hi, tok_stride, stream)
  PMCE_LATTN_CASE(16, 16);
  PMCE_LATTN_CASE(16, 17);
  PMCE_LATTN_CASE(16, 19);
  PMCE_LATTN_CASE(48, 16);
  PMCE_LATTN_CASE(48, 17);
  PMCE_LATTN_CASE(48, 19);
#undef PMCE_LATTN_CASE
  return PMCE_OK;
}
