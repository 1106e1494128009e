// Single-product f16 "NT" GEMM for gfx950:  C[m,n] = epi( sum_k A16[m,k] * W16[n,k] + bias[n] )  (+ R[m,n]).
//
// The opt-in half-precision mode of ViTPose's blocks (vitpose.cpp, precision 1): ONE v_mfma_f32_32x32x16_f16 product with fp32
// accumulation where gemm_split_f16.hip spends three on an exact two-term split.  A16 is plain f16 [M][lda] - what
// pmce_layernorm_rows_f16, pmce_vit_attention_f16 and this kernel's own f16 output write, every value rounded by r16 (common.hpp:
// nearest even, |x| < 2^-14 flushed to zero).  W16 is packed once by pmce_gemm_pack_f16: r16(W[n] * 2^s(n)) with the per-row power of two
// pmce_gemm_pack_split_f16 chooses (the row's max |w| lifted into [2^14, 2^15)) and wscale[n] = 2^-s(n) beside it, in the blocked
// layout [ceil(N/64)][K/32][64 rows][32 f16].  No operand relies on f16 sub-normals.
//
// Kernel.  A 32-wide k-tile of f16 is a 64-byte row - the size of a 16-wide k-tile of the split planes - so the machinery of
// gemm_split_f16.hip carries over: 256 threads = 2x2 waves, wave tile (32 TM) x (32 TN), LDS-DMA of 16 rows x 64 B per wave
// instruction into a ring of NS = 3 or 4 stages, 16-byte chunks XOR-swizzled with (row >> 2) & 3, one barrier per k-tile, the stream
// of k-tiles running across tile boundaries, the tile's bias and 2^-s slices riding in with its first k-tile (the bias, scaled like
// its row of W, is the accumulators' initial value), persistent workgroups on an XCD-local chunk of the grouped tile order.  Per pair
// of 64-byte rows TWO matrix instructions (k = [0,16) then [16,32) of the tile: k ascending) replace three.
// Arithmetic per element is the same in every tile shape and at every position: a row of C has the same bits whatever M is.
// Epilogue, all fp32: scale by 2^-s, exact GELU (gelu_erf, the split kernel's), residual (R may be C itself: a lane reads an element of
// R before it writes that element of C, and nobody else touches it), then fp32 stores - or one r16 and f16 stores (fc1 -> fc2).
// Rows past M and columns past N: their operand rows are clamped to row M - 1 / N - 1 (never read past the tensors), never stored.
#include <atomic>

#include "gemm_split_common.hpp"

namespace {

struct F16Params {
  const _Float16* A;    // [M][lda] f16
  const _Float16* W;    // blocked [ceil(N/64)][K/32][64][32] f16 of r16(W[n] * 2^s(n))
  const float* wscale;  // [N]: 2^-s(n)
  const float* bias;    // [N] or null
  const float* R;       // fp32 residual [M][ldc] or null; may be C
  void* C;              // fp32 [M][ldc], or f16 [M][ldc] (O16)
  int M, N, K;
  unsigned lda, ldc;    // elements
  int ntm, ntn;
  unsigned* oflow;
};

template <int TM, int TN>
struct F16Cfg {
  static constexpr int BM = 64 * TM, BN = 64 * TN;
  static constexpr int STAGE_FLOATS = (BM + BN) * 16;  // 64 bytes per row
  static constexpr int NS = STAGE_FLOATS * 4 * 4 <= 64 * 1024 ? 4 : 3;
  // + NS {bias, 2^-s} slice pairs.  The DMA cursor runs NS - 1 k-tiles ahead across tile boundaries and a tile may be ONE k-tile (K = 32):
  // the slices of NS tiles can be in LDS or on their way before the oldest is read, so each of them has a slot of its own.  (The split
  // kernel has two slots and needs two k-tiles per tile.)
  static constexpr int LDS_BYTES = NS * STAGE_FLOATS * 4 + NS * 2048;
  static constexpr int DPW = (BM + BN) / 64;  // DMA instructions per wave per k-tile (16 rows each)
};

template <int TM, int TN, int ACT, bool RES, bool O16>
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(F16Params p) {
  static_assert(!(O16 && RES), "the f16 result is fc1's: no residual");
  using Cfg = F16Cfg<TM, TN>;
  constexpr int BM = Cfg::BM, BN = Cfg::BN, WM = 32 * TM, WN = 32 * TN;
  constexpr int NS = Cfg::NS, SF = Cfg::STAGE_FLOATS, DPW = Cfg::DPW;
  constexpr int GA = BM / 16;  // 16-row groups of the A part of a stage (a multiple of 4: every wave's first GA/4 DMAs are A's)
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = lane & 31, hb = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;

  // ---- persistent workgroups on an XCD-local chunk of the grouped tile order (common.hpp: xcd_chunk, grouped_tile_coords; GROUP_M as the
  // split kernel's) ----
  const XcdChunk chunk = xcd_chunk(p.ntm * p.ntn);
  const int chunk_start = chunk.start, chunk_len = chunk.len, bx = chunk.bx, gx = chunk.gx;
  if (bx >= chunk_len) return;
  auto tile_coords = [&](int bid, int& mb, int& nb) { grouped_tile_coords<4, BM, BN>(bid, p.ntm, p.ntn, mb, nb); };
  const int my_tiles = (chunk_len - bx + gx - 1) / gx;
  const int nk = p.K / 32;  // stages per tile
  const int total = my_tiles * nk;

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.A), 0, 0xffffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(p.W), 0, 0xffffffff, 0x00020000);
  // bounded: lanes past bias[N-1] / wscale[N-1] read zeros (the tile's column offset is part of the LANE offset below: the range check
  // covers the lane offset, not the scalar one)
  const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? p.N * 4 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wscale), 0, p.N * 4, 0x00020000);

  // ---- DMA side.  Instruction q of a wave moves row group g = wave + 4 q of a stage: lane L -> row 16 g + (L >> 2), PHYSICAL
  // chunk L & 3, which holds logical chunk (L & 3) ^ ((row >> 2) & 3) = (L & 3) ^ ((L >> 4) & 3).  Offsets in bytes. ----
  const int drow = lane >> 2;
  const unsigned dchunk = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
  unsigned doff[DPW];
  auto set_ptrs = [&](int mb, int nb) {
#pragma unroll
    for (int q = 0; q < DPW; ++q) {
      const int g = wave + 4 * q;
      if (q < GA / 4)
        doff[q] = (unsigned)min(mb + 16 * g + drow, p.M - 1) * p.lda * 2u + dchunk;
      else {
        const unsigned r = (unsigned)min(nb + 16 * (g - GA) + drow, p.N - 1);
        doff[q] = (r >> 6) * (unsigned)(p.K / 32) * 4096u + (r & 63u) * 64u + dchunk;  // 64-row block, 64-byte rows
      }
    }
  };
  const unsigned lds0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) float*)lds;
  const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);
  auto issue = [&](int kt, int stage) {
    const unsigned stage_base = lds_wave + stage * (SF * 4);
    const int ko = kt * 64, kw = kt * 4096;  // bytes
#pragma unroll
    for (int q = 0; q < DPW; ++q) {
      const bool is_a = q < GA / 4;
      sdma16o(is_a ? rsrc_a : rsrc_w, doff[q], is_a ? ko : kw, stage_base, q * 4096);
    }
  };

  // issue-side cursor (runs NS-1 k-tiles ahead of the compute side, across tile boundaries)
  int i_li = bx, i_kt = 0, i_stage = 0, issued = 0, i_nb = 0, i_mb = 0, i_par = 0;
  tile_coords(chunk_start + i_li, i_mb, i_nb);
  set_ptrs(i_mb, i_nb);
  auto issue_next = [&]() {
    if (i_kt == 0) {  // the tile's bias and 2^-s slices: 64 lanes x 4 floats each
      const unsigned soff = (unsigned)i_nb * 4u + (unsigned)lane * 16u;
      if (p.bias && wave == 0) lds_dma16(rsrc_b, soff, 0, lds0 + NS * SF * 4 + i_par * 2048);
      if (wave == 1) lds_dma16(rsrc_s, soff, 0, lds0 + NS * SF * 4 + i_par * 2048 + 1024);
      i_par = i_par + 1 == NS ? 0 : i_par + 1;
    }
    issue(i_kt, i_stage);
    ++issued;
    i_stage = i_stage + 1 == NS ? 0 : i_stage + 1;
    if (++i_kt == nk) {
      i_kt = 0;
      i_li += gx;
      if (i_li < chunk_len) {
        tile_coords(chunk_start + i_li, i_mb, i_nb);
        set_ptrs(i_mb, i_nb);
      }
    }
  };
#pragma unroll
  for (int q = 0; q < NS - 1; ++q)
    if (issued < total) issue_next();

  float w_down[TN];  // 2^-s of this lane's column in each of the wave's TN 32-column blocks
  const int swz = (n0 >> 2) & 3;
  const int a_row = (wm * WM + n0) * 16, w_row = BM * 16 + (wn * WN + n0) * 16;  // floats inside a stage
  const int c0 = 4 * (hb ^ swz), c1 = 4 * ((2 + hb) ^ swz);                      // k = 8 hb + [0,8) and 16 + 8 hb + [0,8) of the k-tile

  f32x16 acc[TM][TN];
  int li = bx, kt = 0, stage = 0, c_par = 0;
  int m_base, n_base;
  tile_coords(chunk_start + li, m_base, n_base);

  for (int it = 0; it < total; ++it) {
    // k-tile `it` has landed when at most (younger batches) x DPW of this wave's DMAs are still in flight (in-order completion)
    const int younger = issued - it - 1;
    if (NS == 4 && younger >= 2) wait_vm<2 * DPW>();
    else if (younger >= 1) wait_vm<DPW>();
    else wait_vm<0>();
    __syncthreads();  // every wave's part of k-tile `it` is in LDS; every wave is done reading the stage of k-tile it-1
    if (issued < total) issue_next();

    if (kt == 0) {  // the bias slice (scaled like its row of W) is the accumulators' initial value
      const float* sB = lds + NS * SF + c_par * 512 + wn * WN + n0;
      c_par = c_par + 1 == NS ? 0 : c_par + 1;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        w_down[j] = sB[256 + j * 32];
        const float bv = p.bias ? sB[j * 32] * pow2_recip(w_down[j]) : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = bv;
      }
    }
    {
      const float* sA = lds + stage * SF;
      f16x8 a0[TM], a1[TM], w0[TN], w1[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        a0[i] = *reinterpret_cast<const f16x8*>(sA + a_row + i * 512 + c0);
        a1[i] = *reinterpret_cast<const f16x8*>(sA + a_row + i * 512 + c1);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        w0[j] = *reinterpret_cast<const f16x8*>(sA + w_row + j * 512 + c0);
        w1[j] = *reinterpret_cast<const f16x8*>(sA + w_row + j * 512 + c1);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[i], w0[j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[i], w1[j], acc[i][j], 0, 0, 0);
    }

    stage = stage + 1 == NS ? 0 : stage + 1;
    if (++kt == nk) {
      // ---- epilogue of the finished tile, straight from the accumulators ----
      kt = 0;
      bool bad = false;  // this lane produced a non-finite value, or (f16 result) one beyond f16's 65504
      if constexpr (O16) {
        // A lane holds ONE column of 16 rows.  Registers r, r + 1 (r even) are adjacent rows; adjacent lanes pair up so that every lane
        // stores one dword per two elements: even lanes {(row r, n), (row r, n + 1)}, odd lanes {(row r + 1, n - 1), (row r + 1, n)}.
        // Buffer-form stores bounded after row M - 1: the block's position is part of the lane offset, which is what the range check covers.
        const bool odd = lane & 1;
        const unsigned rows_left = (unsigned)min(p.M - m_base, BM);
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(static_cast<_Float16*>(p.C) + (size_t)m_base * p.ldc, 0,
                                                                                 rows_left * p.ldc * 2u, 0x00020000);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int cb = n_base + wn * WN + j * 32;
          if (cb >= p.N) continue;  // (N % 32 == 0: a 32-column block is all in or all out)
#pragma unroll
          for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
              f32x2 v = {pinned(acc[i][j][r] * w_down[j]), pinned(acc[i][j][r + 1] * w_down[j])};  // ONE fp32 product in every instantiation
              if (ACT == 1) v = gelu_erf2(v);
              typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
              const _Float16 h0 = r16(pinned(v.x)), h1 = r16(pinned(v.y));
              bad = bad || __builtin_amdgcn_classh(h0, 0x207) || __builtin_amdgcn_classh(h1, 0x207);
              const unsigned w = __builtin_bit_cast(unsigned, h2_t{h0, h1});
              const unsigned nbr = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xf, 0xf, true);  // lane ^ 1
              const unsigned outw = odd ? ((nbr >> 16) | (w & 0xffff0000u)) : ((w & 0xffffu) | (nbr << 16));
              const int row = wm * WM + i * 32 + 4 * hb + (r & 3) + 8 * (r >> 2) + (odd ? 1 : 0);
              const unsigned vo = ((unsigned)row * p.ldc + (unsigned)(cb + (n0 & ~1))) * 2u;
              __builtin_amdgcn_raw_buffer_store_b32(outw, rsrc_c, vo, 0, 0);  // write-back: the next product's A operand
            }
          }
        }
      } else {
        float* const Cf = static_cast<float*>(p.C);
        const bool full = (m_base + BM <= p.M) && (n_base + BN <= p.N);
        if (full) {
          // Full tile, buffer-form accesses (gemm_split_f16.hip): one set of 16 lane offsets serves every block and both R and C; the
          // residual of block b + 1 is requested before block b is stored.
          constexpr int NBLK = TM * TN;
          const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(Cf + (size_t)m_base * p.ldc, 0, 0xffffffff, 0x00020000);
          const __amdgpu_buffer_rsrc_t rsrc_r =
              __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? p.R + (size_t)m_base * p.ldc : Cf), 0, 0xffffffff, 0x00020000);
          unsigned voff[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) voff[r] = ((unsigned)(4 * hb + (r & 3) + 8 * (r >> 2)) * p.ldc + (unsigned)n0) * 4u;
          auto blk_off = [&](int b) __attribute__((always_inline)) {  // wave-uniform
            return ((unsigned)(wm * WM + (b % TM) * 32) * p.ldc + (unsigned)(n_base + wn * WN + (b / TM) * 32)) * 4u;
          };
          float rv[2][16];
          auto res_load = [&](int b, float (&dst)[16]) __attribute__((always_inline)) {
            const unsigned so = blk_off(b);
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_r, voff[r], so, 0));
          };
          if (RES) res_load(0, rv[0]);
#pragma unroll
          for (int b = 0; b < NBLK; ++b) {
            const int j = b / TM, i = b % TM;
            if (RES && b + 1 < NBLK) res_load(b + 1, rv[(b + 1) & 1]);
            const unsigned so = blk_off(b);
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
              f32x2 v = {pinned(acc[i][j][r] * w_down[j]), pinned(acc[i][j][r + 1] * w_down[j])};  // ONE fp32 product in every instantiation
              if (ACT == 1) v = gelu_erf2(v);
              if (RES) v += f32x2{rv[b & 1][r], rv[b & 1][r + 1]};
              const float vx = v.x, vy = v.y;
              bad = bad || nonfinite(vx) || nonfinite(vy);
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vx), rsrc_c, voff[r], so, 2);
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vy), rsrc_c, voff[r + 1], so, 2);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int n = n_base + wn * WN + j * 32 + n0;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
              const int mrow = m_base + wm * WM + i * 32 + 4 * hb;
              float* Cp = Cf + (size_t)mrow * p.ldc + n;
              const float* Rp = RES ? p.R + (size_t)mrow * p.ldc + n : nullptr;
#pragma unroll
              for (int r = 0; r < 16; r += 2) {  // the same arithmetic as the full-tile path (results do not depend on tile shape)
                f32x2 v = {pinned(acc[i][j][r] * w_down[j]), pinned(acc[i][j][r + 1] * w_down[j])};  // ONE fp32 product in every instantiation
                if (ACT == 1) v = gelu_erf2(v);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                  const int rr = ((r + e) & 3) + 8 * ((r + e) >> 2);
                  if (n < p.N && mrow + rr < p.M) {
                    float o = e ? v.y : v.x;
                    if (RES) o += Rp[(size_t)rr * p.ldc];
                    bad = bad || nonfinite(o);
                    Cp[(size_t)rr * p.ldc] = o;
                  }
                }
              }
            }
          }
        }
      }
      report_nonfinite(p.oflow, bad);
      li += gx;
      if (li < chunk_len) tile_coords(chunk_start + li, m_base, n_base);
    }
  }
}

// ---- launch ---------------------------------------------------------------------------------------------------------------
std::atomic<int> g_f16_tile{-1};   // pmce_gemm_f16_set_tuning: -1 = automatic
std::atomic<int> g_f16_grid{0};    // > 0: at most that many workgroups (a multiple of 8): tests make a workgroup walk many tiles

template <int TM, int TN, int ACT, bool RES, bool O16>
int f16_launch_one(const F16Params& p, int grid, hipStream_t stream) {
  using Cfg = F16Cfg<TM, TN>;
  static std::atomic<unsigned long long> done{0};
  PMCE_TRY(pmce_opt_in_lds(reinterpret_cast<const void*>(&gemm_f16_kernel<TM, TN, ACT, RES, O16>), Cfg::LDS_BYTES, done, "gemm_nt_f16"));
  hipLaunchKernelGGL((gemm_f16_kernel<TM, TN, ACT, RES, O16>), dim3(grid), dim3(256), Cfg::LDS_BYTES, stream, p);
  return PMCE_OK;
}

template <int TM, int TN>
int f16_launch_cfg(F16Params& p, int act, bool o16, hipStream_t stream) {
  using Cfg = F16Cfg<TM, TN>;
  p.ntm = (p.M + Cfg::BM - 1) / Cfg::BM;
  p.ntn = (p.N + Cfg::BN - 1) / Cfg::BN;
  const int per_cu = (160 * 1024) / Cfg::LDS_BYTES >= 3 ? 3 : 2;
  long long g = (long long)p.ntm * p.ntn;
  if (g > 256 * per_cu) g = 256 * per_cu;
  const int cap = g_f16_grid.load(std::memory_order_relaxed);
  if (cap > 0 && g > cap) g = cap;
  g = (g + 7) & ~7ll;
  const bool res = p.R != nullptr;
  if (o16) return act == 1 ? f16_launch_one<TM, TN, 1, false, true>(p, (int)g, stream) : f16_launch_one<TM, TN, 0, false, true>(p, (int)g, stream);
  if (act == 1) return res ? f16_launch_one<TM, TN, 1, true, false>(p, (int)g, stream) : f16_launch_one<TM, TN, 1, false, false>(p, (int)g, stream);
  return res ? f16_launch_one<TM, TN, 0, true, false>(p, (int)g, stream) : f16_launch_one<TM, TN, 0, false, false>(p, (int)g, stream);
}

// Tile choice, as gemm_split_f16.hip's for large grids: a launch takes as long as its busiest CU; `ovh` is the per-area handicap of the
// smaller wave tiles, MEASURED (scripts/bench_vitpose.py, `products_ms_per_launch_by_forced_tile`: ViTPose-H's four products at M = 12288
// with each shape forced, time per tile area on the busiest CU relative to 128 x 256): 128 x 128 costs 1.22 / 1.15 / 1.19 / 1.23 x
// (qkv / proj / fc1 / fc2), 64 x 128 costs 1.50 / 1.35 / 1.57 / 1.59 x - more than the split kernel's 1.12 and 1.3, as its 1.5 x LDS
// bytes per matrix instruction suggest.  The means are used.  128 x 256 is the fastest shape for all four products.
struct F16Tile { int bm, bn; double ovh; };
const F16Tile kF16Tiles[] = {{128, 256, 1.0}, {128, 128, 1.20}, {64, 128, 1.50}};
int pick_f16_tile(int M, int N) {
  const int forced = g_f16_tile.load(std::memory_order_relaxed);
  if (forced >= 0 && forced < 3) return forced;
  int best = 0;
  double best_cost = 1e300;
  for (int i = 0; i < 3; ++i) {
    const F16Tile& t = kF16Tiles[i];
    const long long tiles = (long long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
    const long long per_cu = ((tiles + 7) / 8 + 31) / 32;
    const double cost = (double)per_cu * t.bm * t.bn * t.ovh;
    if (cost < best_cost) { best_cost = cost; best = i; }
  }
  return best;
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
  F16Params p;
  p.A = static_cast<const _Float16*>(A16); p.W = static_cast<const _Float16*>(W16); p.wscale = wscale; p.bias = bias; p.R = R; p.C = C;
  p.M = M; p.N = N; p.K = K; p.lda = (unsigned)lda; p.ldc = (unsigned)ldc; p.ntm = p.ntn = 0;
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
    int e = 0;
    if (m > 0.f && m < 3.0e38f) frexpf(m, &e);  // m = f * 2^e, f in [0.5, 1)
    e = max(-110, min(e, 125));                  // keeps 2^(15-e) and 2^(e-15) normal fp32 numbers
    const float up = m > 0.f ? ldexpf(1.f, 15 - e) : 1.f, down = m > 0.f ? ldexpf(1.f, e - 15) : 1.f;
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
