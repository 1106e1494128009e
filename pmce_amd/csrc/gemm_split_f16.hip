// Three-product f16 "NT" GEMM for gfx950:  C[m,n] = epi( sum_k A[m,k] * W[n,k] + bias[n] )  (+ R[m,n]),  fp32 in memory.
//
// The pose lifter's Linear layers (reference PoseEstimation.py:13-29 via timm Attention/Mlp, and imgfeat_embed,
// PoseEstimation.py:80) are 25 of the path's 30 large products and 70 % of its time on the fp32 matrix pipe
// (v_mfma_f32_32x32x2_f32: 157 TFLOP/s).  The f16 pipe is 16x faster (v_mfma_f32_32x32x16_f16: 2.5 PFLOP/s) and
// accumulates in fp32, so an fp32 product costs three f16 products at fp32 accuracy:
//     a = ahi + alo * 2^-11,  w * 2^s = whi + wlo            (hi = rne16(x), lo = rne16(x - hi); 22 mantissa bits each)
//     a * w * 2^s  =  ahi whi + ahi wlo + alo (whi 2^-11)  +  O(2^-22)
// (the dropped lo*lo term and the planes' own rounding sit below the fp32 product's accumulation error: measured against an
// fp64 product the result is CLOSER than the fp32 pipe's, tests/test_gpu_ops.py; on operands whose planes are known integers the three
// products have ONE fp32 value and every tile shape, path and epilogue form is held to it bit for bit, tests/test_gpu_gemm_split_exact.py
// with tests/gemm_split_ref.py).  2^s - a power of two per OUTPUT ROW of W
// (round 3; per tensor before), chosen by pmce_gemm_pack_split_f16 - lifts the row's max|w| to [2^14, 2^15) so that wlo and
// whi 2^-11 are normal f16 numbers for every weight within 2^-17 of the row's largest: an outlier row cannot starve the other
// rows' lo planes.  alo carries 2^11 so that it is normal wherever ahi is.  No operand relies on f16 sub-normals.
//
// Kernel (gemm_split_kernel.hpp; the same template's SINGLE instantiations are gemm_f16.hip's product): 256 threads = 2x2 waves, wave tile (32 TM) x (32 TN), block tile (64 TM) x (64 TN), k-tile 16.
//  * W is PACKED once: per row and 16-wide k-tile, 16 f16 hi then 16 f16 lo (64 bytes - the size of a 16-wide fp32 k-tile of
//    A, so both operands move as 64-byte rows).  A stays fp32 in memory (or arrives packed the same way, APACK) and is split in
//    registers between its ds_read and the matrix pipe.
//  * Tiles go global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds), 16 rows x 64 B per wave instruction, into a ring of
//    NS = 3 or 4 stages; the 16-byte chunks of a row are XOR-swizzled with (row >> 2) & 3 on the DMA's source address and on
//    the ds_read address (conflict-free ds_read_b128).  A k-iteration is 24 (TN = 4) or 12 matrix instructions per wave -
//    0.3 us - far less than a loaded L2 / HBM round trip, hence NS - 1 k-tiles in flight and ONE barrier per iteration:
//        wait(k-tile it landed) ; barrier ; issue DMA of k-tile it+NS-1 into the stage read in iteration it-1 ; compute.
//    The stream of k-tiles runs across tile boundaries (the next tile's first k-tiles fly under this tile's last ones).
//    The tile's bias slice rides in with its first k-tile (one more DMA instruction of wave 0) and becomes the accumulators'
//    initial value: the k-loop has no compiler-counted vector-memory operation whose wait would drain the ring.
//  * PERSISTENT workgroups, two per CU, walk an XCD-local chunk of the tile order (as gemm_f32.hip); the epilogue (scale by
//    2^-s, GELU, residual, stores) runs straight from the accumulators while the CU's other workgroup keeps the pipe busy.
#include <atomic>

#include "gemm_split_kernel.hpp"

// ---- launch ---------------------------------------------------------------------------------------------------------------
static std::atomic<int> g_split_tile{-1};  // pmce_gemm_split_set_tuning (tests sweep the tile shapes through it); -1 = automatic
extern "C" int pmce_gemm_split_set_tuning(int tile) {
  g_split_tile.store(tile, std::memory_order_relaxed);
  return PMCE_OK;
}

template <int TM, int TN, int ACT, bool RES, bool APACK, bool OPACK = false, bool RS = false, int KSUB = 1, bool LNEP = false>
static int launch_one(const SplitParams& p, int grid, hipStream_t stream) {
  using Cfg = SplitCfg<TM, TN>;
  static std::atomic<unsigned long long> done{0};
  // + two slices of BM row scales (RS) / the LayerNorm epilogue's exchange slots (LNEP)
  constexpr int LDS = (KSUB == 1 ? Cfg::LDS_BYTES : 3 * KSUB * Cfg::STAGE_FLOATS * 4 + 4096) + (RS || LNEP ? 2048 : 0);
  PMCE_TRY(pmce_opt_in_lds(reinterpret_cast<const void*>(&gemm_split_kernel<TM, TN, ACT, RES, APACK, OPACK, RS, KSUB, LNEP>), LDS, done,
                           "gemm_split_f16"));
  hipLaunchKernelGGL((gemm_split_kernel<TM, TN, ACT, RES, APACK, OPACK, RS, KSUB, LNEP>), dim3(grid), dim3(256), LDS, stream, p);
  return PMCE_OK;
}
// the 64x128 tile with two k-tiles per stage (small grids): the operand / epilogue combinations the model's products use
template <int KSUB>
static int launch_small_k32(SplitParams& p, int act, bool apack, bool opack, hipStream_t stream) {
  using Cfg = SplitCfg<1, 2>;
  p.ntm = (p.M + Cfg::BM - 1) / Cfg::BM;
  p.ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
  int g = p.ntm * p.ntn;
  if (g > 512) g = 512;
  g = capped_grid(g, pmce_gemm_workgroup_cap());  // (pmce_gemm_set_max_workgroups' cap)
  const bool res = p.R != nullptr;
  if (p.rscale) return launch_one<1, 2, 0, false, true, false, true, KSUB>(p, g, stream);
  if (opack) return launch_one<1, 2, 1, false, true, true, false, KSUB>(p, g, stream);
  if (apack) return res ? launch_one<1, 2, 0, true, true, false, false, KSUB>(p, g, stream)
                        : launch_one<1, 2, 0, false, true, false, false, KSUB>(p, g, stream);
  return launch_one<1, 2, 0, false, false, false, false, KSUB>(p, g, stream);
}
static bool small_k32_form_exists(int act, bool apack, bool opack, bool res, bool rs) {
  if (rs || opack) return true;
  if (apack) return act == 0;
  return act == 0 && !res;
}
template <int TM, int TN>
static int launch_cfg(SplitParams& p, int act, bool apack, bool opack, hipStream_t stream) {
  using Cfg = SplitCfg<TM, TN>;
  p.ntm = (p.M + Cfg::BM - 1) / Cfg::BM;
  p.ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
  const int g = persistent_grid((long long)p.ntm * p.ntn, Cfg::LDS_BYTES, pmce_gemm_workgroup_cap());
  const bool res = p.R != nullptr;
  if (p.rscale) return launch_one<TM, TN, 0, false, true, false, true>(p, g, stream);  // raw-input products: packed, row-scaled A
  if (opack) return launch_one<TM, TN, 1, false, true, true>(p, g, stream);  // fc1 of the lifter: GELU, packed in, packed out
  if (apack) {
    if (act == 1) return res ? launch_one<TM, TN, 1, true, true>(p, g, stream) : launch_one<TM, TN, 1, false, true>(p, g, stream);
    return res ? launch_one<TM, TN, 0, true, true>(p, g, stream) : launch_one<TM, TN, 0, false, true>(p, g, stream);
  }
  if (act == 1) return res ? launch_one<TM, TN, 1, true, false>(p, g, stream) : launch_one<TM, TN, 1, false, false>(p, g, stream);
  return res ? launch_one<TM, TN, 0, true, false>(p, g, stream) : launch_one<TM, TN, 0, false, false>(p, g, stream);
}

// Tile choice (large grids: cheapest_tile with this form's handicaps)
static const GemmTile kSplitTiles[3] = {{128, 256, 1.0}, {128, 128, 1.12}, {64, 128, 1.3}};
static int pick_split_tile(int M, int N) {
  const int forced = g_split_tile.load(std::memory_order_relaxed);
  if (forced >= 0 && forced < 3) return forced;
  // Small grids (fewer 128x256 tiles than CUs): the launch is ONE round of workgroups, each bound by its own serial chain per
  // k-tile (wait -> barrier -> DMA issue -> fragment reads -> 24 / 12 / 6 dependent matrix instructions per wave): 0.9 / 0.66 / 0.43 us
  // per iteration for the three shapes whatever the number of tiles (profiles/r04_c_*: the AdaLN product's 24 workgroups iterate as
  // fast as the GRU projection's 216).  Take the shape with the shortest chain whose tiles still run in one round (two workgroups per
  // CU interleave, three of the smallest shape fit).
  if ((long long)((M + 127) / 128) * ((N + 255) / 256) < 256) {
    static const double t_iter[3] = {0.9, 0.66, 0.43};
    static const int slots[3] = {512, 512, 768};
    int best = 0;
    double best_cost = 1e300;
    for (int i = 0; i < 3; ++i) {
      const GemmTile& t = kSplitTiles[i];
      const long long tiles = (long long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
      const double cost = (double)((tiles + slots[i] - 1) / slots[i]) * t_iter[i];
      if (cost < best_cost - 1e-12) { best_cost = cost; best = i; }
    }
    return best;
  }
  return cheapest_tile(kSplitTiles, M, N);
}

// Which kernel takes the product under the current tuning - the ONE decision, read by gemm_split_any's launch and by pmce_gemm_split_path.
enum SplitPath { kPathTile0 = 0, kPathTile1 = 1, kPathTile2 = 2, kPathTwoKTiles = 3, kPathSmall64 = 4, kPathSmall128 = 5 };
static int split_path(int M, int N, int K, int act, bool apack, bool opack, bool res, bool rs) {
  const int tile = pick_split_tile(M, N);
  const bool automatic = g_split_tile.load(std::memory_order_relaxed) < 0;
  if (tile == 2 && automatic) {
    // at most one round of 64 x 128 tiles: the small-grid kernel (gemm_split_small.hip: eight waves per tile, a deep ring, no tile stream)
    const int nwn = pmce_gemm_split_small_nwn(M, N, K, act, apack, opack, res, rs);
    if (nwn != 0) return nwn == 2 ? kPathSmall64 : kPathSmall128;
    if (K % 32 == 0 && K >= 128 && (long long)((M + 63) / 64) * ((N + 127) / 128) <= 512 && small_k32_form_exists(act, apack, opack, res, rs))
      return kPathTwoKTiles;  // small grid: two k-tiles per trip
  }
  return tile;
}
// 0 / 1 / 2: the persistent kernel's 128x256 / 128x128 / 64x128 tile; 3: 64x128 with two k-tiles per stage; 4 / 5: the small-grid kernel's
// 64x64 / 64x128 tile; PMCE_ERR_ARG: a product pmce_gemm_nt_split_f16 refuses for its sizes.  A query: it launches nothing.
extern "C" int pmce_gemm_split_path(int M, int N, int K, int act, int a_packed, int c_packed, int has_residual, int row_scaled) {
  PMCE_REQUIRE(M > 0 && N > 0 && K >= 32 && K % 16 == 0, "gemm_split_path: need M,N>0, K>=32 and K%%16==0 (got M=%d N=%d K=%d)", M, N, K);
  PMCE_REQUIRE(act == 0 || act == 1, "gemm_split_path: act must be 0 or 1");
  PMCE_REQUIRE(!row_scaled || K >= 128, "gemm_split_path: a row-scaled A needs K >= 128");
  return split_path(M, N, K, act, (a_packed || row_scaled) != 0, c_packed != 0, has_residual != 0, row_scaled != 0);
}

static int gemm_split_any(const float* A, const float* Wp, const float* wscale, const float* bias, const float* R, float* C, int M,
                          int N, int K, long long lda, long long ldc, int act, int a_packed, int c_packed, int c_div,
                          long long c_lo, long long c_hi, hipStream_t stream, const float* rscale = nullptr, int w_blocked = 0) {
  PMCE_REQUIRE(A && Wp && wscale && C, "gemm_split: null pointer");
  PMCE_REQUIRE(M > 0 && N > 0 && K >= 32 && K % 16 == 0, "gemm_split: need M,N>0, K>=32 and K%%16==0 (got M=%d N=%d K=%d)", M, N, K);
  PMCE_REQUIRE(act == 0 || act == 1, "gemm_split: act must be 0 or 1");
  PMCE_REQUIRE(lda >= K && lda % 4 == 0 && ldc >= N, "gemm_split: lda=%lld (>=K, multiple of 4) / ldc=%lld (>=N)", lda, ldc);
  PMCE_REQUIRE(!a_packed || lda == K, "gemm_split: a packed A has lda == K");
  PMCE_REQUIRE((long long)M * lda * 4 < (1ll << 32) && ((long long)N + 63) / 64 * 64 * K * 4 < (1ll << 32) && (long long)M * ldc < (1ll << 32),
               "gemm_split: an operand spans 4 GiB or more (split the batch)");
  PMCE_REQUIRE(ldc < (1ll << 21), "gemm_split: ldc=%lld (the tile epilogue addresses a 256-row window of C / R with 32-bit byte offsets)", ldc);
  PMCE_REQUIRE(c_div == 0 || R == nullptr, "gemm_split: a C row map cannot be combined with a residual");
  PMCE_REQUIRE(!c_packed || (a_packed && act == 1 && R == nullptr && c_div == 0 && N % 32 == 0 && ldc == N),
               "gemm_split: a packed result is supported for the packed-A + GELU form with N %% 32 == 0 and ldc == N");
  PMCE_REQUIRE(!rscale || (a_packed && !c_packed && act == 0 && R == nullptr && K >= 128),
               "gemm_split: a row-scaled A is a packed A with K >= 128; no activation, residual or packed result");
  // (K >= 128 is the RS epilogue's invariant: it reads the tile's row-scale slice from LDS at the END of the tile, while the DMA cursor runs
  // NS - 1 <= 3 stages ahead across tile boundaries - a tile must span at least NS - 1 stages (K / (16 KSUB) >= 3 with KSUB <= 2), or tile t + 2's
  // slice would land on tile t's scales before its epilogue.  ADVICE r04.)
  SplitParams p;
  p.A = A; p.W = Wp; p.wscale = wscale; p.bias = bias; p.R = R; p.C = C; p.rscale = rscale; p.wblk = w_blocked;
  p.M = M; p.N = N; p.K = K; p.lda = (unsigned)lda; p.ldc = (unsigned)ldc;
  p.c_div = c_div; p.c_lo = c_lo; p.c_hi = c_hi;
  p.ln1_w = p.ln1_b = p.ln2_w = p.ln2_b = nullptr; p.ln1_eps = p.ln2_eps = 0.f; p.out1 = p.out2 = nullptr;
  p.oflow = pmce_overflow_sink();
  p.clk = pmce_clock_sink();  // (thread-local: set while an entry point of a model with a clock probe runs)
  switch (split_path(M, N, K, act, a_packed != 0, c_packed != 0, R != nullptr, rscale != nullptr)) {
    case kPathSmall64:
      PMCE_TRY(pmce_gemm_split_small_launch(p, 2, a_packed != 0, c_packed != 0, stream));
      return pmce_check_launch("gemm_nt_split_f16 (small grid)");
    case kPathSmall128:
      PMCE_TRY(pmce_gemm_split_small_launch(p, 4, a_packed != 0, c_packed != 0, stream));
      return pmce_check_launch("gemm_nt_split_f16 (small grid)");
    case kPathTwoKTiles:
      PMCE_TRY(launch_small_k32<2>(p, act, a_packed != 0, c_packed != 0, stream));
      return pmce_check_launch("gemm_nt_split_f16 (64x128, two k-tiles per stage)");
    case kPathTile0: PMCE_TRY((launch_cfg<2, 4>(p, act, a_packed != 0, c_packed != 0, stream))); break;
    case kPathTile1: PMCE_TRY((launch_cfg<2, 2>(p, act, a_packed != 0, c_packed != 0, stream))); break;
    default: PMCE_TRY((launch_cfg<1, 2>(p, act, a_packed != 0, c_packed != 0, stream))); break;
  }
  return pmce_check_launch("gemm_nt_split_f16");
}

// The product's one entry point.  rscale != null -> A is row-scaled (Ap / rscale from pmce_split_rows_scaled_f16: raw inputs of any finite
// fp32 magnitude; C[m][n] = 2^e(m) 2^-s(n) (Ahi Whi + Ahi Wlo + Alo Whi) + bias[n]); c_div > 0 -> mapped output rows (ldc == N then);
// w_blocked: the weight's layout (pmce_gemm_pack_split_f16's `blocked`; 1 is what the model's launch sequences pass).
extern "C" int pmce_gemm_nt_split_f16(const float* A, const float* rscale, const float* Wp, int w_blocked, const float* wscale,
                                      const float* bias, const float* R, float* C, int M, int N, int K, long long lda, long long ldc,
                                      int act, int a_packed, int c_packed, int c_div, long long c_lo, long long c_hi, hipStream_t stream) {
  PMCE_REQUIRE(c_div >= 0 && (c_div == 0 || ldc == N), "gemm_split_blk: a row map needs ldc == N");
  return gemm_split_any(A, Wp, wscale, bias, R, C, M, N, K, lda, ldc, act, rscale ? 1 : a_packed, c_packed, c_div, c_lo, c_hi, stream,
                        rscale, w_blocked ? 1 : 0);
}

// A product with N = 256 and a residual whose result feeds a LayerNorm chain (the proj and fc2 products of a C = 256 lifter block,
// reference PoseEstimation.py:26-28,84-85,91-92,101-106): with x = Ap W^T + bias + R,
//   y1 = ln1_w ? LN(x; ln1_w, ln1_b, ln1_eps) : x ;   out1 = y1 (fp32 [M,256], may alias R; may be null)
//   out2 = LN(y1; ln2_w, ln2_b, ln2_eps) written PRE-SPLIT (the next product's A; may be null)
// - pmce_gemm_nt_split_f16 followed by pmce_ln_chain_f32(out2_split = 1) in one launch (64 x 256 tiles: a workgroup owns whole
// rows).  Ap pre-split [M,K]; W packed (w_blocked: the blocked layout); statistics two-pass in fp32 like pmce_ln_chain (a different
// summation order: the results agree to the last bits, not bit for bit).
extern "C" int pmce_gemm_nt_split_f16_ln(const float* Ap, const float* Wp, int w_blocked, const float* wscale, const float* bias,
                                         const float* R, int M, int K, const float* ln1_w, const float* ln1_b, float ln1_eps, float* out1,
                                         const float* ln2_w, const float* ln2_b, float ln2_eps, float* out2, hipStream_t stream) {
  PMCE_REQUIRE(Ap && Wp && wscale && R && (out1 || out2), "gemm_split_ln: null pointer");
  PMCE_REQUIRE(M > 0 && K >= 32 && K % 16 == 0, "gemm_split_ln: need M>0, K>=32 and K%%16==0 (got M=%d K=%d)", M, K);
  PMCE_REQUIRE((!ln1_w) == (!ln1_b) && (!out2 || (ln2_w && ln2_b)), "gemm_split_ln: a LayerNorm needs weight and bias");
  PMCE_REQUIRE((long long)M * K * 4 < (1ll << 32) && (long long)M * 256 * 4 < (1ll << 32), "gemm_split_ln: an operand spans 4 GiB or more (split the batch)");
  SplitParams p;
  p.A = Ap; p.W = Wp; p.wscale = wscale; p.bias = bias; p.R = R; p.C = nullptr; p.rscale = nullptr; p.wblk = w_blocked;
  p.M = M; p.N = 256; p.K = K; p.lda = (unsigned)K; p.ldc = 256u;
  p.c_div = 0; p.c_lo = 0; p.c_hi = 0;
  p.oflow = pmce_overflow_sink();
  p.clk = pmce_clock_sink();
  p.ln1_w = ln1_w; p.ln1_b = ln1_b; p.ln1_eps = ln1_eps; p.out1 = out1;
  p.ln2_w = ln2_w; p.ln2_b = ln2_b; p.ln2_eps = ln2_eps; p.out2 = out2;
  p.ntm = (M + 63) / 64;
  p.ntn = 1;
  const int g = capped_grid(p.ntm > 512 ? 512 : p.ntm, pmce_gemm_workgroup_cap());
  // (two k-tiles per stage on small grids, as the plain 64 x 128 tile has them, were measured and change nothing here: at M = 272 the
  // launch is its prologue and the epilogue's dependent chain, not the 16 trips of its k-loop)
  PMCE_TRY((launch_one<1, 4, 0, true, true, false, false, 1, true>(p, g, stream)));
  return pmce_check_launch("gemm_nt_split_f16_ln");
}

// ---- operand packing ------------------------------------------------------------------------------------------------------
// W[N][ldw] fp32 -> Wp[N][K/16][2][16] f16 (N*K floats of storage) and wscale[N] = 2^-s(n), s(n) chosen per row so that the
// row's max|W| * 2^s lies in [2^14, 2^15): hi = rne16(W 2^s), lo = rne16(W 2^s - hi) - both normal f16 for every weight within
// 2^-17 of the row's largest (smaller ones lose bits that are 2^-28 of the row's largest product).  One wave per row.
__global__ __launch_bounds__(256) void split_pack_kernel(const float* __restrict__ W, int N, int K, int ldw, _Float16* __restrict__ Wp,
                                                         float* __restrict__ wscale, int blocked) {
  const int lane = threadIdx.x & 63;
  for (long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); n < N; n += (long long)gridDim.x * 4) {
    const float* __restrict__ row = W + n * ldw;
    float m = 0.f;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(row[k]));
    m = wave_max(m);
    float up = 1.f, down = 1.f;
    if (m > 0.f) row_pow2(m, up, down);
    if (lane == 0) wscale[n] = down;
    // row-major: 32 f16 per (row, k-tile), a row's k-tiles adjacent; blocked: [n / 64][k-tile][n % 64][32 f16]
    _Float16* __restrict__ out = blocked ? Wp + ((n >> 6) * (long long)(K / 16) * 64 + (n & 63)) * 32 : Wp + n * K * 2;
    const long long kt_stride = blocked ? 64 * 32 : 32;
    for (int k = lane; k < K; k += 64) {
      const float ws = row[k] * up;
      const _Float16 hi = (_Float16)ws;
      const _Float16 lo = (_Float16)(ws - (float)hi);
      out[(k / 16) * kt_stride + (k % 16)] = hi;
      out[(k / 16) * kt_stride + 16 + (k % 16)] = lo;
    }
  }
}
// blocked != 0: the same planes in the BLOCKED layout [ceil(N/64)][K/16][64][16 hi | 16 lo] (Wp: ceil(N/64)*64*K floats of storage; rows
// past N are not written and never contribute): what a tile fetches per k-tile is then contiguous 4 KB pieces.  A streamed weight (one
// that is read once per launch from HBM: the final product's 278 MB, the GRU and AdaLN projections) otherwise arrives as 64-byte pieces
// one weight row apart - a different DRAM page per piece.
extern "C" int pmce_gemm_pack_split_f16(const float* W, int N, int K, int ldw, float* Wp, float* wscale, int blocked, hipStream_t stream) {
  PMCE_REQUIRE(W && Wp && wscale, "gemm_pack_split_blk: null pointer");
  PMCE_REQUIRE(N > 0 && K > 0 && K % 16 == 0 && ldw >= K, "gemm_pack_split_blk: need N>0, K%%16==0, ldw>=K (N=%d K=%d ldw=%d)", N, K, ldw);
  const int blocks = (N + 3) / 4 < 4096 ? (N + 3) / 4 : 4096;
  hipLaunchKernelGGL(split_pack_kernel, dim3(blocks), dim3(256), 0, stream, W, N, K, ldw, reinterpret_cast<_Float16*>(Wp), wscale, blocked ? 1 : 0);
  return pmce_check_launch("gemm_pack_split_f16");
}

// A[M][lda] fp32 -> Ap[M][K/16][2][16] f16: hi = rne16(a), lo = rne16((a - hi) * 2^11)
__global__ void split_rows_kernel(const float* __restrict__ A, long long M, int K, long long lda, _Float16* __restrict__ Ap) {
  const long long total = M * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long m = i / K;
    const int k = (int)(i % K);
    const float a = A[m * lda + k];
    const _Float16 hi = (_Float16)a;
    const _Float16 lo = lo_plane_plain(a, hi);
    _Float16* row = Ap + (m * K + (k / 16) * 16) * 2;
    row[k % 16] = hi;
    row[16 + k % 16] = lo;
  }
}
extern "C" int pmce_split_rows_f16(const float* A, long long M, int K, long long lda, float* Ap, hipStream_t stream) {
  PMCE_REQUIRE(A && Ap && M > 0 && K > 0 && K % 16 == 0 && lda >= K, "split_rows: bad arguments");
  const long long total = M * K;
  const long long want = (total + 256 * 4 - 1) / (256 * 4);
  hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, stream, A, M, K, lda,
                     reinterpret_cast<_Float16*>(Ap));
  return pmce_check_launch("split_rows_f16");
}

// Raw input rows of ANY finite fp32 magnitude -> packed planes of A[m] * 2^-e(m) plus rscale[m] = 2^e(m): e(m) puts the row's
// max |a| into [2^14, 2^15) (exactly what pmce_gemm_pack_split_f16 does for a weight row), so neither a feature of 1e5 (beyond f16's
// 65504) nor one of 1e-7 (whose planes would be f16 sub-normals) loses anything: both planes are normal f16 numbers for every
// element within 2^-17 of its row's largest.  The reference's Linear accepts any fp32 row (PoseEstimation.py:80,
// CoevoDecoder.py:228); so does this.  Rows holding inf / nan keep scale 1 and propagate as non-finite results of their own row
// only, like the reference's.  One wave per row; K % 16 == 0.
__global__ __launch_bounds__(256) void split_rows_scaled_kernel(const float* __restrict__ A, long long M, int K, long long lda,
                                                                _Float16* __restrict__ Ap, float* __restrict__ rscale) {
  const int lane = threadIdx.x & 63;
  for (long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); m < M; m += (long long)gridDim.x * 4) {
    const float* __restrict__ row = A + m * lda;
    float mx = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
      mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    mx = wave_max(mx);  // (fmaxf drops NaNs: a row with a NaN and finite values is scaled by its finite maximum, the NaN stays a NaN)
    float down = 1.f, up = 1.f;  // (the row is multiplied DOWN by 2^(15 - e); an infinite maximum keeps scale 1)
    if (mx > 0.f && mx < 3.0e38f) row_pow2(mx, down, up);
    if (lane == 0) rscale[m] = up;
    _Float16* __restrict__ out = Ap + m * K * 2;
    for (int k = lane * 4; k < K; k += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
      const float a[4] = {pinned(v.x * down), pinned(v.y * down), pinned(v.z * down), pinned(v.w * down)};  // ONE fp32 value for both planes
      f16x4 hi, lo;
#pragma unroll
      for (int i = 0; i < 4; ++i) hi[i] = (_Float16)a[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) lo[i] = lo_plane_plain(a[i], hi[i]);
      _Float16* q = out + (k >> 4) * 32 + (k & 15);
      *reinterpret_cast<f16x4*>(q) = hi;
      *reinterpret_cast<f16x4*>(q + 16) = lo;
    }
  }
}
extern "C" int pmce_split_rows_scaled_f16(const float* A, long long M, int K, long long lda, float* Ap, float* rscale, hipStream_t stream) {
  PMCE_REQUIRE(A && Ap && rscale && M > 0 && K > 0 && K % 16 == 0 && lda >= K && lda % 4 == 0, "split_rows_scaled: bad arguments");
  const long long want = (M + 3) / 4;
  hipLaunchKernelGGL(split_rows_scaled_kernel, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, stream, A, M, K, lda,
                     reinterpret_cast<_Float16*>(Ap), rscale);
  return pmce_check_launch("split_rows_scaled_f16");
}
