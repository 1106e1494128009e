// Multi-head attention of a ViT block (ViTPose's backbone: softmax(q k^T hd^-0.5) v per head, no class token, no mask) for sequences
// of up to 192 tokens and heads of 64 or 80 channels, on the f16 matrix pipe: ONE kernel, vit_attention_kernel<HD, NT, SPLIT>, in the
// network's two precisions (vitpose.cpp).  q, k, v arrive as the fp32 rows the qkv product wrote ([n N][3 C], a row = q | k | v, each
// (heads, hd)) and are rounded to f16 on their way to the matrix pipe.
//
// Arithmetic, split form (SPLIT; as seq_attention_mfma.hip).  Every operand is split into (hi, lo) f16 planes, x = xh + xl 2^-11:
// q.k = sum qh kh + 2^-11 sum (qh kl + ql kh), the two sums in separate fp32 accumulators of v_mfma_f32_32x32x16_f16 - three products
// per step.  P is split like every other operand, and the result leaves pre-split - [16 f16 hi | 16 f16 lo*2^11] per 16 channels in the
// bytes of the fp32 row - as the A operand of `proj` (gemm_split_f16.hip).
// Arithmetic, single-product form (!SPLIT; vitpose.cpp's precision 1).  q, k, v are rounded once with r16 (common.hpp: nearest even,
// |x| < 2^-14 flushed to zero); S^T = K Q^T in ONE fp32 accumulator; s = q.k hd^-0.5; p~ = exp(s - max); the output is
// (r16(p~) . r16(v)) / sum(p~), the sum over the UNROUNDED fp32 p~, rounded once with r16 and stored as plain f16 [n N][C] - the A
// operand of `proj` (gemm_f16.hip).  A finite result beyond f16's 65504 is reported like a non-finite one.  The lo planes and the cross
// accumulators are not part of this instantiation, neither as registers nor as LDS.
// Both compute transposed, S^T = K Q^T (rows = keys, columns = queries): a lane holds 16 of the 32 keys of a key tile for ONE query, so
// the softmax over keys is in-lane plus one exchange with lane ^ 32, and P^T in the accumulators already is the B operand (k = keys,
// n = queries) of out^T = V^T P^T.
//
// Softmax: the exact two-pass form.  The scores of a 32-query tile against ALL keys (NT <= 6 key tiles) stay in registers, 16 NT
// fp32 per lane (main + 2^-11 cross folded as soon as a key tile is done, so 96 and not 192 at N = 192); maximum, 2^x on log2-scaled
// scores, sum, then P V, normalised by 1 / sum once at the end.  A streaming softmax would need the running-maximum rescale of the
// output accumulators and buys nothing here: K and V of one (image, head) fit in LDS whole.
//
// Work split.  One workgroup of four waves per (image, head).  K of the head goes global -> registers -> LDS as rows of 16-channel
// groups, [key][hd/16][16 hi | 16 lo] in the split form and [key][hd/16][16 f16] in the other (row stride hd * 4 + 16 or hd * 2 + 16
// bytes, an odd number of 16-byte slots: the 16 rows of a ds_read_b128 service group fall on different banks);
// V goes to LDS TRANSPOSED, Vt[channel][key position] as one f16 image per plane, the key positions of a 32-key tile permuted into
// the register order of P^T (position 16 s + 8 hb + e holds key 16 s + 4 hb + (e & 3) + 8 (e >> 2)), so that the A operand of
// V^T P^T is one 16-byte LDS read per plane.  One barrier; then wave w takes the query tiles w, w + 4.  Q is the B operand of
// K Q^T - lane (query, k-half) needs 8 consecutive channels of its own row - and goes global -> registers directly.
// hd = 80 is five k-steps of 16 and three 32-channel output blocks of which the last is half used: its lanes 16..31 read a clamped
// channel row and store nothing (attention is 2.5 % of the network's arithmetic; the simpler of the two forms).
//
// Bounds.  Keys and queries at or beyond N read the image's row N - 1 (clamped, never another image's rows or memory past the
// tensor); such keys get a score of -inf and a zero V, such queries are not stored.  Nothing of an (image, head) depends on another
// image or on n: a result row has the same bits wherever its image sits.
// Every NT at its full tile and one past it, exact gathers and the fences: tests/test_gpu_vitpose_edges.py (split form) and
// tests/test_gpu_vitpose_f16_ops.py (single-product form).
#include "gemm_split_common.hpp"

namespace {

template <int HD, int NT, bool SPLIT>
struct VitAttnCfg {
  static constexpr int KS = HD / 16;               // k-steps of q.k
  static constexpr int DB = (HD + 31) / 32;        // 32-channel output blocks
  static constexpr int PLANES = SPLIT ? 2 : 1;
  static constexpr int KG = 32 * PLANES;           // a 16-channel group of a K row in LDS (bytes): 16 hi, then 16 lo in the split form
  static constexpr int KRS = KS * KG + 16;         // K row stride in LDS (bytes): an odd number of 16-byte slots
  static constexpr int VRS = NT * 64 + 16;         // Vt row stride (bytes): NT * 32 key positions of f16 + 16
  static constexpr int K_BYTES = NT * 32 * KRS;
  static constexpr int V_BYTES = HD * VRS;         // per plane
  static constexpr int LDS_BYTES = K_BYTES + PLANES * V_BYTES;
};

// position of key `w` (0..31) of a key tile inside the tile's 32 Vt columns
__device__ __forceinline__ int vt_pos(int w) {
  const int w16 = w & 15;
  return (w & 16) + ((w16 >> 2) & 1) * 8 + ((w16 >> 3) << 2) + (w16 & 3);
}

// the rounding of an operand's hi plane - its only plane in the single-product form (a COMPUTED x goes through pinned() first in both)
template <bool SPLIT>
__device__ __forceinline__ _Float16 hi16(float x) {
  if constexpr (SPLIT) return (_Float16)x;
  else return r16(x);
}

// out: the split form's planes in the bytes of the fp32 rows [n N][C], or plain f16 [n N][C].
// What only the split form has - the lo planes kl, Vl, ql, pl, ol and the cross accumulators s_cross, o_cross - is declared in both
// instantiations and read under SPLIT alone: in the other nothing depends on them (the accumulators' zeroing is dead) and they take no
// register and no LDS.  (Zeroing and folding are spelled with a constant condition, not `if constexpr`, on purpose: hipcc's register
// allocation follows the spelling, and with `if constexpr` there the split instantiations <64, 1> and <64, 4> take 4 and 12 VGPRs more.)
template <int HD, int NT, bool SPLIT>
__global__ __launch_bounds__(256, 1) void vit_attention_kernel(const float* __restrict__ qkv, void* __restrict__ out, int N, int heads,
                                                              unsigned* oflow) {
  using Cfg = VitAttnCfg<HD, NT, SPLIT>;
  constexpr int KS = Cfg::KS, DB = Cfg::DB, KG = Cfg::KG, KRS = Cfg::KRS, VRS = Cfg::VRS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const Ks = smem;
  unsigned char* const Vh = smem + Cfg::K_BYTES;
  unsigned char* const Vl = Vh + Cfg::V_BYTES;  // (the end of LDS in the single-product form)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hb = lane >> 5;
  const int img = (int)blockIdx.x / heads, head = (int)blockIdx.x - img * heads;
  const int C = heads * HD;
  const size_t row0 = (size_t)img * N;  // the image's first row
  const float* const base = qkv + row0 * (size_t)(3 * C) + head * HD;

  // ---- K -> rows of f16 groups, V -> the transposed image(s) ----
  constexpr int C4 = HD / 4;
  for (int i = tid; i < NT * 32 * C4; i += 256) {
    const int key = i / C4, c = 4 * (i - key * C4);
    const float* src = base + (size_t)min(key, N - 1) * (size_t)(3 * C) + c;
    const f32x4 kx = *reinterpret_cast<const f32x4*>(src + C);
    f32x4 vx = *reinterpret_cast<const f32x4*>(src + 2 * C);
    if (key >= N) vx = f32x4{0.f, 0.f, 0.f, 0.f};  // p = 0 there, and 0 * v must stay 0
    f16x4 kh, kl;
#pragma unroll
    for (int e = 0; e < 4; ++e) kh[e] = hi16<SPLIT>(kx[e]);
    if constexpr (SPLIT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) kl[e] = lo_plane(kx[e], kh[e]);
    }
    unsigned char* kp = Ks + key * KRS + (c >> 4) * KG + (c & 15) * 2;
    *reinterpret_cast<f16x4*>(kp) = kh;
    if constexpr (SPLIT) *reinterpret_cast<f16x4*>(kp + 32) = kl;
    const int pos = (key & ~31) + vt_pos(key & 31);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const _Float16 h = hi16<SPLIT>(vx[e]);
      *reinterpret_cast<_Float16*>(Vh + (c + e) * VRS + pos * 2) = h;
      if constexpr (SPLIT) *reinterpret_cast<_Float16*>(Vl + (c + e) * VRS + pos * 2) = lo_plane(vx[e], h);
    }
  }
  __syncthreads();

  // hd^-0.5 * log2(e): scores in log2 units, softmax on the hardware 2^x
  constexpr float scale = (HD == 64 ? 0.125f : 0.11180339887498948482f) * 1.44269504088896340736f;
  constexpr float two_m11 = 0.00048828125f;
  bool bad = false;
  const int nqt = (N + 31) >> 5;
  for (int qt = wave; qt < nqt; qt += 4) {
    const int query = qt * 32 + l31;
    // this lane's part of Q: row `query` (clamped), per k-step the 8 channels 16 ks + 8 hb + [0, 8)
    f16x8 qh[KS], ql[KS];
    {
      const float* qrow = base + (size_t)min(query, N - 1) * (size_t)(3 * C) + hb * 8;
      f32x4 qraw[2 * KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qraw[2 * ks] = *reinterpret_cast<const f32x4*>(qrow + ks * 16);
        qraw[2 * ks + 1] = *reinterpret_cast<const f32x4*>(qrow + ks * 16 + 4);
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const float v[8] = {qraw[2 * ks].x, qraw[2 * ks].y, qraw[2 * ks].z, qraw[2 * ks].w,
                            qraw[2 * ks + 1].x, qraw[2 * ks + 1].y, qraw[2 * ks + 1].z, qraw[2 * ks + 1].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) qh[ks][e] = hi16<SPLIT>(v[e]);
        if constexpr (SPLIT) {
#pragma unroll
          for (int e = 0; e < 8; ++e) ql[ks][e] = lo_plane(v[e], qh[ks][e]);
        }
      }
    }
    // ---- pass 1: S^T = K Q^T for every key tile; register r of tile kt is key 32 kt + 4 hb + (r & 3) + 8 (r >> 2) ----
    float sc[NT][16];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      const unsigned char* pk = Ks + (kt * 32 + l31) * KRS + hb * 16;
      f32x16 s_main, s_cross;
#pragma unroll
      for (int r = 0; r < 16; ++r) s_main[r] = s_cross[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x8 kh = *reinterpret_cast<const f16x8*>(pk + ks * KG);
        s_main = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], s_main, 0, 0, 0);
        if constexpr (SPLIT) {
          const f16x8 kl = *reinterpret_cast<const f16x8*>(pk + ks * KG + 32);
          s_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], s_cross, 0, 0, 0);
          s_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], s_cross, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + 4 * hb + (r & 3) + 8 * (r >> 2);
        const float sv = (SPLIT ? fmaf(s_cross[r], two_m11, s_main[r]) : s_main[r]) * scale;
        sc[kt][r] = key < N ? sv : -INFINITY;
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
    f32x16 o_main[DB], o_cross[DB];
#pragma unroll
    for (int blk = 0; blk < DB; ++blk)
#pragma unroll
      for (int r = 0; r < 16; ++r) o_main[blk][r] = o_cross[blk][r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f16x8 ph, pl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float pv32 = pinned(sc[kt][8 * s + e]);
          ph[e] = hi16<SPLIT>(pv32);
          if constexpr (SPLIT) pl[e] = lo_plane(pv32, ph[e]);
        }
#pragma unroll
        for (int blk = 0; blk < DB; ++blk) {
          const int ch = min(32 * blk + l31, HD - 1);
          const int off = ch * VRS + (kt * 32 + s * 16 + hb * 8) * 2;
          const f16x8 vh = *reinterpret_cast<const f16x8*>(Vh + off);
          o_main[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, ph, o_main[blk], 0, 0, 0);
          if constexpr (SPLIT) {
            const f16x8 vl = *reinterpret_cast<const f16x8*>(Vl + off);
            o_cross[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, pl, o_cross[blk], 0, 0, 0);
            o_cross[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, ph, o_cross[blk], 0, 0, 0);
          }
        }
      }
    // register r of block blk is channel 32 blk + 4 hb + (r & 3) + 8 (r >> 2) of query l31: four consecutive channels per r >> 2, written
    // into the query's row: pre-split into this head's 16-channel groups in the bytes of the fp32 row (2 C f16), or as C plain f16
    if (query < N) {
      _Float16* const orow = static_cast<_Float16*>(out) + (row0 + query) * (size_t)C * (SPLIT ? 2 : 1);
#pragma unroll
      for (int blk = 0; blk < DB; ++blk)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int ch0 = 32 * blk + 8 * rq + 4 * hb;  // (a multiple of 4; a group of four lies inside the head or outside it)
          if (ch0 < HD) {
            f16x4 oh, ol;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = pinned((SPLIT ? fmaf(o_cross[blk][4 * rq + e], two_m11, o_main[blk][4 * rq + e]) : o_main[blk][4 * rq + e]) * inv);
              bad = bad || nonfinite(v);
              oh[e] = hi16<SPLIT>(v);
              if constexpr (SPLIT) ol[e] = lo_plane(v, oh[e]);
              else bad = bad || __builtin_amdgcn_classh(oh[e], 0x207);  // a finite value beyond f16's 65504
            }
            if constexpr (SPLIT) {
              const int cg = head * HD + ch0;
              _Float16* p = orow + (cg >> 4) * 32 + (cg & 15);
              *reinterpret_cast<f16x4*>(p) = oh;
              *reinterpret_cast<f16x4*>(p + 16) = ol;
            } else {
              *reinterpret_cast<f16x4*>(orow + head * HD + ch0) = oh;
            }
          }
        }
    }
  }
  report_nonfinite(oflow, bad);
}

// the form's name in error texts and launch labels
template <bool SPLIT>
constexpr const char* vit_attention_name = SPLIT ? "vit_attention_split_f16" : "vit_attention_f16";

template <int HD, int NT, bool SPLIT>
int launch_vit_attention(const float* qkv, void* out, int n, int N, int heads, hipStream_t stream) {
  using Cfg = VitAttnCfg<HD, NT, SPLIT>;
  static std::atomic<unsigned long long> done{0};
  PMCE_TRY(pmce_opt_in_lds(reinterpret_cast<const void*>(&vit_attention_kernel<HD, NT, SPLIT>), Cfg::LDS_BYTES, done, vit_attention_name<SPLIT>));
  hipLaunchKernelGGL((vit_attention_kernel<HD, NT, SPLIT>), dim3((unsigned)(n * heads)), dim3(256), Cfg::LDS_BYTES, stream, qkv, out, N, heads,
                     pmce_overflow_sink());
  return pmce_check_launch(vit_attention_name<SPLIT>);
}

template <int HD, bool SPLIT>
int dispatch_vit_attention(const float* qkv, void* out, int n, int N, int heads, hipStream_t stream) {
  switch ((N + 31) / 32) {
    case 1: return launch_vit_attention<HD, 1, SPLIT>(qkv, out, n, N, heads, stream);
    case 2: return launch_vit_attention<HD, 2, SPLIT>(qkv, out, n, N, heads, stream);
    case 3: return launch_vit_attention<HD, 3, SPLIT>(qkv, out, n, N, heads, stream);
    case 4: return launch_vit_attention<HD, 4, SPLIT>(qkv, out, n, N, heads, stream);
    case 5: return launch_vit_attention<HD, 5, SPLIT>(qkv, out, n, N, heads, stream);
    default: return launch_vit_attention<HD, 6, SPLIT>(qkv, out, n, N, heads, stream);
  }
}

// the argument checks and the HD choice of both entries
template <bool SPLIT>
int vit_attention(const float* qkv, void* out, int n, int N, int C, int heads, hipStream_t stream) {
  constexpr const char* who = vit_attention_name<SPLIT>;
  PMCE_REQUIRE(qkv && out, "%s: null pointer", who);
  PMCE_REQUIRE(n >= 1 && (long long)n * heads < (1ll << 31), "%s: n must be at least 1 and n * heads below 2^31 (got n=%d)", who, n);
  PMCE_REQUIRE(N >= 1 && N <= 192, "%s: N must be in 1..192 (got N=%d)", who, N);
  PMCE_REQUIRE(heads >= 1 && C >= 1 && C % heads == 0 && (C / heads == 64 || C / heads == 80), "%s: C / heads must be 64 or 80 (got C=%d heads=%d)", who,
               C, heads);
  PMCE_REQUIRE(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(out)) & 15) == 0, "%s: qkv and the result must be 16-byte aligned", who);
  if (C / heads == 64) return dispatch_vit_attention<64, SPLIT>(qkv, out, n, N, heads, stream);
  return dispatch_vit_attention<80, SPLIT>(qkv, out, n, N, heads, stream);
}

}  // namespace

extern "C" int pmce_vit_attention_supported(int N, int C, int heads) {
  if (N < 1 || N > 192 || heads < 1 || C < 1 || C % heads != 0) return 0;
  const int hd = C / heads;
  return hd == 64 || hd == 80 ? 1 : 0;
}

extern "C" int pmce_vit_attention_split_f16(const float* qkv, float* out_planes, int n, int N, int C, int heads, hipStream_t stream) {
  return vit_attention<true>(qkv, out_planes, n, N, C, heads, stream);
}

extern "C" int pmce_vit_attention_f16(const float* qkv, void* out16, int n, int N, int C, int heads, hipStream_t stream) {
  return vit_attention<false>(qkv, out16, n, N, C, heads, stream);
}
