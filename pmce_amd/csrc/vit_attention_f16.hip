// Multi-head attention of a ViT block in the single-product f16 mode (vitpose.cpp, precision 1): vit_attention.hip's kernel without
// the lo planes.  Input format, work split, bounds rules and supported shapes are that kernel's: q, k, v are the fp32 rows the qkv
// product wrote ([n N][3 C], a row = q | k | v, each (heads, hd)), 1..192 tokens, heads of 64 or 80 channels, one workgroup of four waves
// per (image, head), wave w takes the query tiles w, w + 4.
//
// Arithmetic.  q, k, v are rounded once with r16 (common.hpp: nearest even, |x| < 2^-14 flushed to zero) on their way to the matrix
// pipe; S^T = K Q^T in ONE fp32 accumulator of v_mfma_f32_32x32x16_f16; s = q.k hd^-0.5; p~ = exp(s - max) (the hardware 2^x on
// log2-scaled scores, two-pass, all keys of a query tile in registers); the output is (r16(p~) . r16(v)) / sum(p~), the sum over the
// UNROUNDED fp32 p~, rounded once with r16 and stored as plain f16 [n N][C] - the A operand of `proj` (gemm_f16.hip).
// LDS: K as one f16 image [key][hd] (row stride hd * 2 + 16 bytes: an odd number of 16-byte slots), V transposed Vt[channel][key
// position] as one f16 image, the key positions of a 32-key tile permuted into the register order of P^T (vit_attention.hip).
//
// Bounds.  Keys and queries at or beyond N read the image's row N - 1 (clamped); such keys get a score of -inf and a zero V, such
// queries are not stored.  Nothing of an (image, head) depends on another image or on n.
#include <atomic>

#include "gemm_split_common.hpp"

namespace {

template <int HD, int NT>
struct VitAttn16Cfg {
  static constexpr int KS = HD / 16;               // k-steps of q.k
  static constexpr int DB = (HD + 31) / 32;        // 32-channel output blocks
  static constexpr int KRS = HD * 2 + 16;          // K row stride in LDS (bytes)
  static constexpr int VRS = NT * 64 + 16;         // Vt row stride (bytes): NT * 32 key positions of f16 + 16
  static constexpr int K_BYTES = NT * 32 * KRS;
  static constexpr int V_BYTES = HD * VRS;
  static constexpr int LDS_BYTES = K_BYTES + V_BYTES;
};

// position of key `w` (0..31) of a key tile inside the tile's 32 Vt columns
__device__ __forceinline__ int vt16_pos(int w) {
  const int w16 = w & 15;
  return (w & 16) + ((w16 >> 2) & 1) * 8 + ((w16 >> 3) << 2) + (w16 & 3);
}

template <int HD, int NT>
__global__ __launch_bounds__(256, 1) void vit_attention_f16_kernel(const float* __restrict__ qkv, _Float16* __restrict__ out, int N, int heads,
                                                                  unsigned* oflow) {
  using Cfg = VitAttn16Cfg<HD, NT>;
  constexpr int KS = Cfg::KS, DB = Cfg::DB, KRS = Cfg::KRS, VRS = Cfg::VRS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const Ks = smem;
  unsigned char* const Vt = smem + Cfg::K_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hb = lane >> 5;
  const int img = (int)blockIdx.x / heads, head = (int)blockIdx.x - img * heads;
  const int C = heads * HD;
  const size_t row0 = (size_t)img * N;  // the image's first row
  const float* const base = qkv + row0 * (size_t)(3 * C) + head * HD;

  // ---- K -> f16 rows, V -> the transposed f16 image ----
  constexpr int C4 = HD / 4;
  for (int i = tid; i < NT * 32 * C4; i += 256) {
    const int key = i / C4, c = 4 * (i - key * C4);
    const float* src = base + (size_t)min(key, N - 1) * (size_t)(3 * C) + c;
    const f32x4 kx = *reinterpret_cast<const f32x4*>(src + C);
    f32x4 vx = *reinterpret_cast<const f32x4*>(src + 2 * C);
    if (key >= N) vx = f32x4{0.f, 0.f, 0.f, 0.f};  // p = 0 there, and 0 * v must stay 0
    f16x4 kh;
#pragma unroll
    for (int e = 0; e < 4; ++e) kh[e] = r16(kx[e]);
    *reinterpret_cast<f16x4*>(Ks + key * KRS + c * 2) = kh;
    const int pos = (key & ~31) + vt16_pos(key & 31);
#pragma unroll
    for (int e = 0; e < 4; ++e) *reinterpret_cast<_Float16*>(Vt + (c + e) * VRS + pos * 2) = r16(vx[e]);
  }
  __syncthreads();

  // hd^-0.5 * log2(e): scores in log2 units, softmax on the hardware 2^x
  constexpr float scale = (HD == 64 ? 0.125f : 0.11180339887498948482f) * 1.44269504088896340736f;
  bool bad = false;
  const int nqt = (N + 31) >> 5;
  for (int qt = wave; qt < nqt; qt += 4) {
    const int query = qt * 32 + l31;
    // this lane's part of Q: row `query` (clamped), per k-step the 8 channels 16 ks + 8 hb + [0, 8)
    f16x8 qh[KS];
    {
      const float* qrow = base + (size_t)min(query, N - 1) * (size_t)(3 * C) + hb * 8;
      f32x4 qraw[2 * KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qraw[2 * ks] = *reinterpret_cast<const f32x4*>(qrow + ks * 16);
        qraw[2 * ks + 1] = *reinterpret_cast<const f32x4*>(qrow + ks * 16 + 4);
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) qh[ks][e] = r16(qraw[2 * ks + (e >> 2)][e & 3]);
    }
    // ---- pass 1: S^T = K Q^T for every key tile; register r of tile kt is key 32 kt + 4 hb + (r & 3) + 8 (r >> 2) ----
    float sc[NT][16];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      const unsigned char* pk = Ks + (kt * 32 + l31) * KRS + hb * 16;
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x8 kh = *reinterpret_cast<const f16x8*>(pk + ks * 32);
        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], s, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + 4 * hb + (r & 3) + 8 * (r >> 2);
        sc[kt][r] = key < N ? s[r] * scale : -INFINITY;
        mx = fmaxf(mx, sc[kt][r]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[kt][r] = __builtin_amdgcn_exp2f(sc[kt][r] - mx);
        sum += sc[kt][r];
      }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    // ---- pass 2: out^T = V^T P^T; rows = the channels 32 blk + l31 (clamped into the head), k = the keys in P^T's register order ----
    f32x16 o[DB];
#pragma unroll
    for (int blk = 0; blk < DB; ++blk)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[blk][r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f16x8 ph;
#pragma unroll
        for (int e = 0; e < 8; ++e) ph[e] = r16(pinned(sc[kt][8 * s + e]));
#pragma unroll
        for (int blk = 0; blk < DB; ++blk) {
          const int ch = min(32 * blk + l31, HD - 1);
          const f16x8 vh = *reinterpret_cast<const f16x8*>(Vt + ch * VRS + (kt * 32 + s * 16 + hb * 8) * 2);
          o[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o[blk], 0, 0, 0);
        }
      }
    // register r of block blk is channel 32 blk + 4 hb + (r & 3) + 8 (r >> 2) of query l31: four consecutive channels per r >> 2
    if (query < N) {
      _Float16* const orow = out + (row0 + query) * (size_t)C + head * HD;
#pragma unroll
      for (int blk = 0; blk < DB; ++blk)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int ch0 = 32 * blk + 8 * rq + 4 * hb;  // (a multiple of 4; a group of four lies inside the head or outside it)
          if (ch0 < HD) {
            f16x4 oh;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = pinned(o[blk][4 * rq + e] * inv);
              bad = bad || nonfinite(v);
              oh[e] = r16(v);
              bad = bad || __builtin_amdgcn_classh(oh[e], 0x207);
            }
            *reinterpret_cast<f16x4*>(orow + ch0) = oh;
          }
        }
    }
  }
  report_nonfinite(oflow, bad);
}

template <int HD, int NT>
int launch_vit_attention_f16(const float* qkv, _Float16* out, int n, int N, int heads, hipStream_t stream) {
  using Cfg = VitAttn16Cfg<HD, NT>;
  static std::atomic<unsigned long long> done{0};
  PMCE_TRY(pmce_opt_in_lds(reinterpret_cast<const void*>(&vit_attention_f16_kernel<HD, NT>), Cfg::LDS_BYTES, done, "vit_attention_f16"));
  hipLaunchKernelGGL((vit_attention_f16_kernel<HD, NT>), dim3((unsigned)(n * heads)), dim3(256), Cfg::LDS_BYTES, stream, qkv, out, N, heads,
                     pmce_overflow_sink());
  return pmce_check_launch("vit_attention_f16");
}

template <int HD>
int dispatch_vit_attention_f16(const float* qkv, _Float16* out, int n, int N, int heads, hipStream_t stream) {
  switch ((N + 31) / 32) {
    case 1: return launch_vit_attention_f16<HD, 1>(qkv, out, n, N, heads, stream);
    case 2: return launch_vit_attention_f16<HD, 2>(qkv, out, n, N, heads, stream);
    case 3: return launch_vit_attention_f16<HD, 3>(qkv, out, n, N, heads, stream);
    case 4: return launch_vit_attention_f16<HD, 4>(qkv, out, n, N, heads, stream);
    case 5: return launch_vit_attention_f16<HD, 5>(qkv, out, n, N, heads, stream);
    default: return launch_vit_attention_f16<HD, 6>(qkv, out, n, N, heads, stream);
  }
}

}  // namespace

extern "C" int pmce_vit_attention_f16(const float* qkv, void* out16, int n, int N, int C, int heads, hipStream_t stream) {
  PMCE_REQUIRE(qkv && out16, "vit_attention_f16: null pointer");
  PMCE_REQUIRE(n >= 1 && (long long)n * heads < (1ll << 31), "vit_attention_f16: n must be at least 1 and n * heads below 2^31 (got n=%d)", n);
  PMCE_REQUIRE(N >= 1 && N <= 192, "vit_attention_f16: N must be in 1..192 (got N=%d)", N);
  PMCE_REQUIRE(heads >= 1 && C >= 1 && C % heads == 0 && (C / heads == 64 || C / heads == 80),
               "vit_attention_f16: C / heads must be 64 or 80 (got C=%d heads=%d)", C, heads);
  PMCE_REQUIRE(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(out16)) & 15) == 0,
               "vit_attention_f16: qkv and the result must be 16-byte aligned");
  if (C / heads == 64) return dispatch_vit_attention_f16<64>(qkv, static_cast<_Float16*>(out16), n, N, heads, stream);
  return dispatch_vit_attention_f16<80>(qkv, static_cast<_Float16*>(out16), n, N, heads, stream);
}
