// Single-product f16 "NT" GEMM for gfx950:  C[m,n] = epi( sum_k A16[m,k] * W16[n,k] + bias[n] )  (+ R[m,n]).
//
// The opt-in half-precision mode of ViTPose's blocks (vitpose.cpp, precision 1): ONE v_mfma_f32_32x32x16_f16 product with fp32
// accumulation where gemm_split_f16.hip spends three on an exact two-term split.  A16 is plain f16 [M][lda] - what
// pmce_layernorm_rows_f16, pmce_vit_attention_f16 and this kernel's own f16 output write, every value rounded by r16 (common.hpp:
// nearest even, |x| < 2^-14 flushed to zero).  W16 is packed once by pmce_gemm_pack_f16: r16(W[n] * 2^s(n)) with the per-row power of two
// pmce_gemm_pack_split_f16 chooses (the row's max |w| lifted into [2^14, 2^15)) and wscale[n] = 2^-s(n) beside it, in the blocked
// layout [ceil(N/64)][K/32][64 rows][32 f16].  No operand relies on f16 sub-normals.
//
// Kernel.  The SINGLE instantiations of gemm_split_kernel (gemm_split_kernel.hpp: a 32-wide k-tile of f16 is a 64-byte row - the size of a
// 16-wide k-tile of the split planes - so ring, DMA, tile walk and fp32 epilogues are the split form's; per pair of 64-byte rows TWO
// matrix instructions, k = [0,16) then [16,32) of the tile, replace three).  This file holds the launcher, the tile choice with this
// form's measured handicaps, the weight packer and the C entry points.
// Arithmetic per element is the same in every tile shape and at every position: a row of C has the same bits whatever M is.
// Epilogue, all fp32: scale by 2^-s, exact GELU (gelu_erf, the split kernel's), residual (R may be C itself: a lane reads an element of
// R before it writes that element of C, and nobody else touches it), then fp32 stores - or one r16 and f16 stores (fc1 -> fc2).
// Rows past M and columns past N: their operand rows are clamped to row M - 1 / N - 1 (never read past the tensors), never stored.
#include <atomic>

#include "gemm_split_kernel.hpp"

namespace {

// ---- launch ---------------------------------------------------------------------------------------------------------------
std::atomic<int> g_f16_tile{-1};   // pmce_gemm_f16_set_tuning: -1 = automatic
std::atomic<int> g_f16_grid{0};    // > 0: at most that many workgroups (a multiple of 8): tests make a workgroup walk many tiles

// gemm_split_kernel<..., APACK = true (64-byte f16 rows), OPACK = O16 (the f16 result), RS = false, KSUB = 1, LNEP = false, SINGLE = true>
template <int TM, int TN, int ACT, bool RES, bool O16>
int f16_launch_one(const SplitParams& p, int grid, hipStream_t stream) {
  constexpr int LDS = SplitCfg<TM, TN, true>::LDS_BYTES;
  static std::atomic<unsigned long long> done{0};
  PMCE_TRY(pmce_opt_in_lds(reinterpret_cast<const void*>(&gemm_split_kernel<TM, TN, ACT, RES, true, O16, false, 1, false, true>), LDS, done,
                           "gemm_nt_f16"));
  hipLaunchKernelGGL((gemm_split_kernel<TM, TN, ACT, RES, true, O16, false, 1, false, true>), dim3(grid), dim3(256), LDS, stream, p);
  return PMCE_OK;
}

template <int TM, int TN>
int f16_launch_cfg(SplitParams& p, int act, bool o16, hipStream_t stream) {
  using Cfg = SplitCfg<TM, TN, true>;
  p.ntm = (p.M + Cfg::BM - 1) / Cfg::BM;
  p.ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
  const int g = persistent_grid((long long)p.ntm * p.ntn, Cfg::LDS_BYTES, g_f16_grid.load(std::memory_order_relaxed));
  const bool res = p.R != nullptr;
  if (o16) return act == 1 ? f16_launch_one<TM, TN, 1, false, true>(p, g, stream) : f16_launch_one<TM, TN, 0, false, true>(p, g, stream);
  if (act == 1) return res ? f16_launch_one<TM, TN, 1, true, false>(p, g, stream) : f16_launch_one<TM, TN, 1, false, false>(p, g, stream);
  return res ? f16_launch_one<TM, TN, 0, true, false>(p, g, stream) : f16_launch_one<TM, TN, 0, false, false>(p, g, stream);
}

// Tile choice (cheapest_tile).  The handicaps are MEASURED (scripts/bench_vitpose.py, `products_ms_per_launch_by_forced_tile`: ViTPose-H's
// four products at M = 12288 with each shape forced, time per tile area on the busiest CU relative to 128 x 256): 128 x 128 costs
// 1.22 / 1.15 / 1.19 / 1.23 x (qkv / proj / fc1 / fc2), 64 x 128 costs 1.50 / 1.35 / 1.57 / 1.59 x - more than the split form's 1.12 and 1.3,
// as its 1.5 x LDS bytes per matrix instruction suggest.  The means are used.  128 x 256 is the fastest shape for all four products.
const GemmTile kF16Tiles[3] = {{128, 256, 1.0}, {128, 128, 1.20}, {64, 128, 1.50}};
int pick_f16_tile(int M, int N) {
  const int forced = g_f16_tile.load(std::memory_order_relaxed);
  return forced >= 0 && forced < 3 ? forced : cheapest_tile(kF16Tiles, M, N);
}

}  // namespace

// tile: 0 = 128x256, 1 = 128x128, 2 = 64x128, anything else = automatic; max_workgroups > 0 caps the persistent grid (rounded up to 8)
extern "C" int pmce_gemm_f16_set_tuning(int tile, int max_workgroups) {
  g_f16_tile.store(tile, std::memory_order_relaxed);
  g_f16_grid.store(max_workgroups > 0 ? max_workgroups : 0, std::memory_order_relaxed);
  return PMCE_OK;
}

extern "C" int pmce_gemm_nt_f16(const void* A16, const void* W16, const float* wscale, const float* bias, const float* R, void* C, int M, int N,
                                int K, long long lda, long long ldc, int act, int c_f16, unsigned* overflow_word, hipStream_t stream) {
  PMCE_REQUIRE(A16 && W16 && wscale && C, "gemm_nt_f16: null pointer");
  PMCE_REQUIRE(M >= 1, "gemm_nt_f16: M must be at least 1 (got M=%d)", M);
  PMCE_REQUIRE(N >= 32 && N % 32 == 0, "gemm_nt_f16: N must be a positive multiple of 32 (got N=%d)", N);
  PMCE_REQUIRE(K >= 32 && K % 32 == 0, "gemm_nt_f16: K must be a positive multiple of 32 (got K=%d)", K);
  PMCE_REQUIRE(act == 0 || act == 1, "gemm_nt_f16: act must be 0 or 1 (got %d)", act);
  PMCE_REQUIRE(c_f16 == 0 || c_f16 == 1, "gemm_nt_f16: c_f16 must be 0 or 1 (got %d)", c_f16);
  PMCE_REQUIRE(lda >= K && lda % 8 == 0, "gemm_nt_f16: lda must be a multiple of 8 and at least K (got lda=%lld K=%d)", lda, K);
  PMCE_REQUIRE(ldc >= N && (!c_f16 || ldc % 2 == 0), "gemm_nt_f16: ldc must be at least N, and even for an f16 result (got ldc=%lld N=%d)", ldc, N);
  PMCE_REQUIRE(!(c_f16 && R), "gemm_nt_f16: an f16 result takes no residual");
  const uintptr_t all = reinterpret_cast<uintptr_t>(A16) | reinterpret_cast<uintptr_t>(W16) | reinterpret_cast<uintptr_t>(wscale) |
                        reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(R) | reinterpret_cast<uintptr_t>(C);
  PMCE_REQUIRE((all & 15) == 0, "gemm_nt_f16: every buffer must be 16-byte aligned (the OR of the addresses ends in 0x%x)", (unsigned)(all & 15));
  PMCE_REQUIRE((long long)M * lda * 2 < (1ll << 32) && ((long long)N + 63) / 64 * 64 * K * 2 < (1ll << 32) && (long long)M * ldc < (1ll << 30),
               "gemm_nt_f16: an operand spans 4 GiB or more (split the batch)");
  PMCE_REQUIRE(ldc < (1ll << 21), "gemm_nt_f16: ldc=%lld (the tile epilogue addresses a 256-row window of C / R with 32-bit byte offsets)", ldc);
  SplitParams p = {};  // (no row scales, row map, clock probe or LayerNorm epilogue in this form; lda and ldc count f16 / result elements)
  p.A = static_cast<const float*>(A16); p.W = static_cast<const float*>(W16); p.wblk = 1; p.wscale = wscale; p.bias = bias; p.R = R;
  p.C = static_cast<float*>(C);
  p.M = M; p.N = N; p.K = K; p.lda = (unsigned)lda; p.ldc = (unsigned)ldc;
  p.oflow = overflow_word ? overflow_word : pmce_overflow_sink();
  switch (pick_f16_tile(M, N)) {
    case 0: PMCE_TRY((f16_launch_cfg<2, 4>(p, act, c_f16 != 0, stream))); break;
    case 1: PMCE_TRY((f16_launch_cfg<2, 2>(p, act, c_f16 != 0, stream))); break;
    default: PMCE_TRY((f16_launch_cfg<1, 2>(p, act, c_f16 != 0, stream))); break;
  }
  return pmce_check_launch("gemm_nt_f16");
}

// ---- weight packing ---------------------------------------------------------------------------------------------------------
// W[N][ldw] fp32 -> W16 blocked [ceil(N/64)][K/32][64][32] f16 of r16(W[n] * 2^s(n)) (ceil(N/64)*64*K f16 of storage; rows past N are
// not written and never contribute) and wscale[N] = 2^-s(n): s(n) exactly as split_pack_kernel chooses it.  One wave per row.
__global__ __launch_bounds__(256) void f16_pack_kernel(const float* __restrict__ W, int N, int K, int ldw, _Float16* __restrict__ Wp,
                                                       float* __restrict__ wscale) {
  const int lane = threadIdx.x & 63;
  for (long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); n < N; n += (long long)gridDim.x * 4) {
    const float* __restrict__ row = W + n * ldw;
    float m = 0.f;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(row[k]));
    m = wave_max(m);
    float up = 1.f, down = 1.f;
    if (m > 0.f) row_pow2(m, up, down);
    if (lane == 0) wscale[n] = down;
    _Float16* __restrict__ out = Wp + ((n >> 6) * (long long)(K / 32) * 64 + (n & 63)) * 32;
    for (int k = lane; k < K; k += 64) out[(long long)(k / 32) * (64 * 32) + (k % 32)] = r16(row[k] * up);
  }
}

extern "C" long long pmce_gemm_packed_f16_halves(int N, int K) { return N > 0 && K > 0 ? ((long long)N + 63) / 64 * 64 * K : 0; }

extern "C" int pmce_gemm_pack_f16(const float* W, int N, int K, int ldw, void* W16, float* wscale, hipStream_t stream) {
  PMCE_REQUIRE(W && W16 && wscale, "gemm_pack_f16: null pointer");
  PMCE_REQUIRE(N >= 1, "gemm_pack_f16: N must be at least 1 (got N=%d)", N);
  PMCE_REQUIRE(K >= 32 && K % 32 == 0, "gemm_pack_f16: K must be a positive multiple of 32 (got K=%d)", K);
  PMCE_REQUIRE(ldw >= K, "gemm_pack_f16: ldw must be at least K (got ldw=%d K=%d)", ldw, K);
  const int blocks = (N + 3) / 4 < 4096 ? (N + 3) / 4 : 4096;
  hipLaunchKernelGGL(f16_pack_kernel, dim3(blocks), dim3(256), 0, stream, W, N, K, ldw, static_cast<_Float16*>(W16), wscale);
  return pmce_check_launch("gemm_pack_f16");
}
