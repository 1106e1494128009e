// The persistent tile kernel of the f16-pipe "NT" GEMMs, in its two forms (arithmetic, operand layout and pipeline: the header of
// gemm_split_f16.hip):
//   * the three-product split form (gemm_split_f16.hip: fp32 in memory, fp32 accuracy), SINGLE = false;
//   * the single-product form (gemm_f16.hip: ViTPose's opt-in f16 mode), SINGLE = true.
// Single-product form.  A is plain f16 [M][lda] and W is r16(W[n] * 2^s(n)) in the blocked layout with 32-wide k-tiles: a 32-wide k-tile of
// f16 is a 64-byte row - the size of a 16-wide k-tile of the split planes - so the DMA descriptors, the swizzle, the ring, the wait ladder,
// the fragment offsets (the hi / lo chunks are k = [0,16) / [16,32) of the tile), the bias seeding and the fp32 epilogues are the split
// form's.  What differs sits under `SINGLE` below and nowhere else: the operands' pitches and nk = K / 32; one {bias, 2^-s} slice slot per
// ring stage, because a tile may be ONE k-tile (K = 32) and the DMA cursor runs NS - 1 k-tiles ahead; the slice DMA's offset form; TWO matrix
// instructions per pair of rows (k ascending) instead of three; ONE pinned fp32 product acc * 2^-s in every epilogue, so that a row of C
// has the same bits in every tile shape; and, in OPACK's place ("the result is the next product's operand"), one r16 and f16 stores.
// RS, LNEP, KSUB = 2, the C row map and the clock probe do not exist in this form.
#pragma once
#include "gemm_split_common.hpp"

template <int TM, int TN, bool SINGLE = false>
struct SplitCfg {
  static constexpr int BM = 64 * TM, BN = 64 * TN;
  static constexpr int STAGE_FLOATS = (BM + BN) * 16;  // 64 bytes per row
#ifdef PMCE_SPLIT_NS3
  static constexpr int NS = 3;
#else
  static constexpr int NS = STAGE_FLOATS * 4 * 4 <= 64 * 1024 ? 4 : 3;
#endif
  // {bias, 2^-s} slice pairs.  Split form: two (this tile's, the next one's) - a tile is at least two k-tiles.  Single-product form: the DMA
  // cursor runs NS - 1 k-tiles ahead across tile boundaries and a tile may be ONE k-tile (K = 32), so the slices of NS tiles can be in LDS or
  // on their way before the oldest is read: each has a slot of its own.
  static constexpr int SLOTS = SINGLE ? NS : 2;
  static constexpr int LDS_BYTES = NS * STAGE_FLOATS * 4 + SLOTS * 2048;
  static constexpr int DPW = (BM + BN) / 64;  // DMA instructions per wave per k-tile (16 rows each)
};

// RS: A is packed AND row-scaled (raw inputs of any fp32 magnitude: imgfeat_embed, the GRU layer-0 input projection) - the
// accumulators start at zero and the epilogue computes acc * 2^-s(n) * 2^e(m) + bias[n].
// KSUB = 2 (round 4; the 64x128 tile on small grids): a stage holds TWO consecutive 16-wide k-tiles, each in the layout of a KSUB = 1
// stage, fetched together and multiplied behind ONE wait and ONE barrier.  A launch of a few hundred small tiles is bound by a
// workgroup's serial chain per k-tile (wait -> barrier -> DMA issue -> fragment reads -> 6 dependent matrix instructions per wave: 0.43 us
// whatever the grid, profiles/r04_c_*); two k-tiles per trip halve the trips.  Same arithmetic and k order: bit-identical results.
// LNEP (round 4; the N = 256 products of a C = 256 lifter block, proj and fc2): the tile is 64 x 256 - whole rows - and the epilogue is
// the LayerNorm chain that followed the product as a launch of its own (lifter.hip ln_chain: norm2 after proj; the shared post-norm
// and the next block's norm1 after fc2): the residual stream and the pre-split LN output leave the accumulators directly, the fp32
// row is never re-read.  Row statistics: two-pass (mean, then centred squares) like ln_chain; a row's 256 columns sit in the two
// column waves of its row half - 32 lanes x 4 blocks each - so a statistic is 3 in-lane adds, a 32-lane all-reduce (4 DPP rotations
// inside the rows of 16 + one swizzle across them; every lane ends with the same bits) and one exchange of 16 floats per lane half
// with the partner wave through LDS.
__device__ __forceinline__ float half32_allsum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));  // row_ror:2
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));  // row_ror:1
  v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401f));                     // lane ^ 16
  return v;
}

// SINGLE: the single-product form (this file's header).  A is then f16 in 64-byte rows (APACK) and OPACK means an f16 result.
template <int TM, int TN, int ACT, bool RES, bool APACK, bool OPACK = false, bool RS = false, int KSUB = 1, bool LNEP = false, bool SINGLE = false>
__global__ __launch_bounds__(256, 2) void gemm_split_kernel(SplitParams p) {
  static_assert(!RS || (APACK && !OPACK && !RES), "a row-scaled A is a packed A; no packed result, no residual");
  static_assert(!LNEP || (TM == 1 && TN == 4 && ACT == 0 && RES && !OPACK && !RS && KSUB == 1), "the LayerNorm epilogue: 64 x 256 tile, residual form");
  static_assert(!SINGLE || (APACK && !RS && KSUB == 1 && !LNEP), "the single-product form: f16 A; no row scales, one k-tile per stage, no LayerNorm epilogue");
  static_assert(!(SINGLE && OPACK && RES), "the f16 result is fc1's: no residual");
  using Cfg = SplitCfg<TM, TN, SINGLE>;
  constexpr int BM = Cfg::BM, BN = Cfg::BN, WM = 32 * TM, WN = 32 * TN;
  constexpr int KW = SINGLE ? 32 : 16;                            // elements of K in a 64-byte row: the k-tile's width
  constexpr int SUBF = Cfg::STAGE_FLOATS;                         // one k-tile of the stage
  constexpr int NS = KSUB == 1 ? Cfg::NS : 3, SF = KSUB * SUBF, DPW = KSUB * Cfg::DPW;
  static_assert(KSUB == 1 || KSUB == 2, "one or two k-tiles per stage (four measured: no further gain)");
  constexpr int GA = BM / 16;  // 16-row groups of the A part of a stage (a multiple of 4: every wave's first GA/4 DMAs are A's)
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = lane & 31, hb = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;

  // ---- persistent workgroups on an XCD-local chunk of the grouped tile order (common.hpp: xcd_chunk, grouped_tile_coords) ----
  const XcdChunk chunk = xcd_chunk(p.ntm * p.ntn);
  const int chunk_start = chunk.start, chunk_len = chunk.len, bx = chunk.bx, gx = chunk.gx;
  if (bx >= chunk_len) return;
  // GROUP_M = 4 (8 until round 6, as gemm_f32.hip has it; 4 measures 0.2-0.9 % faster on the lifter's products at C = 512 and, through what they
  // leave in the caches, 2.5 % on the ln_chain launches between them - equal at C = 256; 16 slower, 2 / 1 mixed: profiles/r06_p_*, r06_q_*)
  auto tile_coords = [&](int bid, int& mb, int& nb) { grouped_tile_coords<4, BM, BN>(bid, p.ntm, p.ntn, mb, nb); };
  // clock probe (bench.py: the shader clock the chip sustains under this kernel; MI355X runs it power-limited far below 2.4 GHz)
  const bool probe = !SINGLE && p.clk != nullptr && tid == 0;
  const long long pc0 = probe ? (long long)__builtin_readcyclecounter() : 0, pw0 = probe ? (long long)wall_clock64() : 0;
  const int my_tiles = (chunk_len - bx + gx - 1) / gx;
  const int nk = p.K / (KW * KSUB);  // stages per tile
  const int total = my_tiles * nk;
  // (Round 2 started every CU's second workgroup half a tile late so that the two would not reach their epilogues together, -8...-18 % then;
  // with today's kernel they drift apart on their own and the delay only cost: +1.1 % at C = 512 without it,
  // profiles/r04_j_gemm_start_skew_ab.txt.  Removed in round 5.)

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), 0, 0xffffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.W), 0, 0xffffffff, 0x00020000);
  // bounded, meant to return zeros to lanes past bias[N-1] / wscale[N-1].  The range check covers the LANE offset, not the scalar one, so this
  // holds for the form of the slice DMA that puts the tile's column offset into the lane offset (issue_next below)
  const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? p.N * 4 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wscale), 0, p.N * 4, 0x00020000);
  // RS: the tile's slice of row scales (bounded: rows past M - 1 read zeros; they are never stored)
  const __amdgpu_buffer_rsrc_t rsrc_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.rscale), 0, RS ? p.M * 4 : 0, 0x00020000);

  // ---- DMA side.  Instruction q of a wave moves row group g = wave + 4 q of a stage: lane L -> row 16 g + (L >> 2), PHYSICAL
  // chunk L & 3, which holds logical chunk (L & 3) ^ ((row >> 2) & 3) = (L & 3) ^ ((L >> 4) & 3). ----
  const int drow = lane >> 2;
  const unsigned dchunk = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * (SINGLE ? 16 : 4));  // floats; SINGLE: bytes
  constexpr int DPS = Cfg::DPW;  // DMA instructions per wave per 16-wide k-tile
  unsigned doff[DPS];
  auto set_ptrs = [&](int mb, int nb) {
#pragma unroll
    for (int q = 0; q < DPS; ++q) {
      const int g = wave + 4 * q;
      if (q < GA / 4)   // (== g < GA: GA is a multiple of 4, so a wave's first GA / 4 instructions are A's whatever the wave)
        doff[q] = SINGLE ? (unsigned)min(mb + 16 * g + drow, p.M - 1) * p.lda * 2u + dchunk  // f16 rows: lda * 2 bytes
                         : ((unsigned)min(mb + 16 * g + drow, p.M - 1) * p.lda + dchunk) * 4u;
      else {
        const unsigned r = (unsigned)min(nb + 16 * (g - GA) + drow, p.N - 1);
        // 64-row blocks of 64-byte rows (the single-product form's W always, K / 32 k-tiles of 4096 bytes), or row-major
        doff[q] = SINGLE   ? (r >> 6) * (unsigned)(p.K / 32) * 4096u + (r & 63u) * 64u + dchunk
                  : p.wblk ? ((r >> 6) * (unsigned)(p.K / 16) * 1024u + (r & 63u) * 16u + dchunk) * 4u
                           : (r * (unsigned)p.K + dchunk) * 4u;
      }
    }
  };
  const unsigned lds0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) float*)lds;
  const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);
  const int kstep_w = (SINGLE || p.wblk) ? 4096 : 64;  // bytes from one k-tile of a W row (block) to the next
  auto issue = [&](int kt, int stage) {
    const unsigned stage_base = lds_wave + stage * (SF * 4);   // ONE scalar per k-tile: the instruction's slot is added as an immediate
#pragma unroll
    for (int sub = 0; sub < KSUB; ++sub) {
      const int ko = (kt * KSUB + sub) * 64, kw = (kt * KSUB + sub) * kstep_w;  // bytes
#pragma unroll
      for (int q = 0; q < DPS; ++q) {
        const bool is_a = q < GA / 4;   // compile-time: no run-time choice of descriptor and offset per instruction
        sdma16o(is_a ? rsrc_a : rsrc_w, doff[q], is_a ? ko : kw, stage_base + sub * (SUBF * 4), q * 4096);
      }
    }
  };

  // issue-side cursor (runs NS-1 k-tiles ahead of the compute side, across tile boundaries)
  int i_li = bx, i_kt = 0, i_stage = 0, issued = 0, i_nb = 0, i_mb = 0, i_par = 0;
  tile_coords(chunk_start + i_li, i_mb, i_nb);
  set_ptrs(i_mb, i_nb);
  auto issue_next = [&]() {
    if (i_kt == 0) {  // the tile's bias and 2^-s slices: 64 lanes x 4 floats each
      // The two forms place the tile's column offset differently.  Single-product: in the LANE offset, which is what the descriptors' range
      // check covers - lanes past column N - 1 of the last tile read zeros.  Split: in the SCALAR offset, which the check ignores - such lanes
      // may read past the array's end (their columns are never stored).  The lane form is the bounded one; the split kernels keep theirs
      // until a change of its own, because it changes their code.
      if constexpr (SINGLE) {
        const unsigned soff = (unsigned)i_nb * 4u + (unsigned)lane * 16u;
        if (p.bias && wave == 0) lds_dma16(rsrc_b, soff, 0, lds0 + NS * SF * 4 + i_par * 2048);
        if (wave == 1) lds_dma16(rsrc_s, soff, 0, lds0 + NS * SF * 4 + i_par * 2048 + 1024);
      } else {
        if (p.bias && wave == 0) lds_dma16(rsrc_b, (unsigned)lane * 16u, i_nb * 4, lds0 + NS * SF * 4 + i_par * 2048);
        if (wave == 1) lds_dma16(rsrc_s, (unsigned)lane * 16u, i_nb * 4, lds0 + NS * SF * 4 + i_par * 2048 + 1024);
      }
      if constexpr (RS)  // and its BM row scales (behind the two slice pairs)
        if (wave == 2) lds_dma16(rsrc_rs, (unsigned)lane * 16u, i_mb * 4, lds0 + NS * SF * 4 + 4096 + i_par * 1024);
      if constexpr (SINGLE) i_par = i_par + 1 == NS ? 0 : i_par + 1;
      else i_par ^= 1;
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
  float b_late[TN];  // RS: the bias of this lane's columns, added after the row scaling
  const int swz = (n0 >> 2) & 3;
  const int a_row = (wm * WM + n0) * 16, w_row = BM * 16 + (wn * WN + n0) * 16;  // floats inside a stage
  // chunk offsets (floats) of this lane's operand fragments
  const int ca0 = 4 * ((2 * hb) ^ swz), ca1 = 4 * ((2 * hb + 1) ^ swz);  // fp32 A: k = 8 hb + [0,4), + [4,8)
  const int ch = 4 * (hb ^ swz), cl = 4 * ((2 + hb) ^ swz);              // packed: hi / lo plane, k = 8 hb + [0,8)

  f32x16 acc[TM][TN];
  int li = bx, kt = 0, stage = 0, c_par = 0;
  int m_base, n_base;
  tile_coords(chunk_start + li, m_base, n_base);

  for (int it = 0; it < total; ++it) {
    // k-tile `it` has landed when at most (younger batches) x DPW of this wave's DMAs are still in flight (in-order
    // completion; anything else outstanding only makes the wait stricter)
    const int younger = issued - it - 1;
    if (NS == 4 && younger >= 2) wait_vm<2 * DPW>();
    else if (younger >= 1) wait_vm<DPW>();
    else wait_vm<0>();
    __syncthreads();  // every wave's part of k-tile `it` is in LDS; every wave is done reading the stage of k-tile it-1
    if (issued < total) issue_next();

    if (kt == 0) {  // the bias slice (scaled like its row of W) is the accumulators' initial value
      const float* sB = lds + NS * SF + c_par * 512 + wn * WN + n0;
      if constexpr (SINGLE) c_par = c_par + 1 == NS ? 0 : c_par + 1;
      else c_par ^= 1;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        w_down[j] = sB[256 + j * 32];
        if constexpr (RS) b_late[j] = p.bias ? sB[j * 32] : 0.f;
        const float bv = (p.bias && !RS) ? sB[j * 32] * pow2_recip(w_down[j]) : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = bv;
      }
    }
#pragma unroll
    for (int sub = 0; sub < KSUB; ++sub) {
    const float* sA = lds + stage * SF + sub * SUBF;
    f16x8 ahi[TM], alo[TM], whi[TN], wlo[TN], wh2[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if constexpr (APACK) {
        ahi[i] = *reinterpret_cast<const f16x8*>(sA + a_row + i * 512 + ch);
        alo[i] = *reinterpret_cast<const f16x8*>(sA + a_row + i * 512 + cl);
      } else {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(sA + a_row + i * 512 + ca0);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(sA + a_row + i * 512 + ca1);
        split8(x0, x1, ahi[i], alo[i]);
      }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      whi[j] = *reinterpret_cast<const f16x8*>(sA + w_row + j * 512 + ch);
      wlo[j] = *reinterpret_cast<const f16x8*>(sA + w_row + j * 512 + cl);
      if constexpr (!SINGLE) wh2[j] = whi[j] * (_Float16)0.00048828125f;  // 2^-11: undoes the scale of alo
    }
    // (single-product form: "hi" and "lo" are k = [0,16) and [16,32) of the k-tile - two instructions, k ascending)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[i], whi[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(SINGLE ? alo[i] : ahi[i], wlo[j], acc[i][j], 0, 0, 0);
    if constexpr (!SINGLE) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo[i], wh2[j], acc[i][j], 0, 0, 0);
    }
    }

    stage = stage + 1 == NS ? 0 : stage + 1;
    if (++kt == nk) {
      // ---- epilogue of the finished tile, straight from the accumulators ----
      kt = 0;
      bool bad = false;  // this lane produced a non-finite value (an operand beyond the f16 range, or fp32 overflow)
      if constexpr (LNEP) {
        // rows of this lane: m_base + 32 wm + 4 hb + (r & 3) + 8 (r >> 2); columns 128 wn + 32 j + n0 (n_base = 0, N = ldc = 256)
        float* sX = lds + NS * SF + 1024;  // exchange slots [pass][wm][wn][hb][16]
        const int rows_left = min(p.M - m_base, BM);
        const unsigned row_bytes = 256u * 4u;
        const __amdgpu_buffer_rsrc_t rsrc_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.R + (size_t)m_base * 256), 0,
                                                                                 (unsigned)rows_left * row_bytes, 0x00020000);
        unsigned lane_off = (unsigned)(wm * 32 + 4 * hb) * row_bytes + (unsigned)(wn * 128 + n0) * 4u;
        asm volatile("" : "+v"(lane_off));  // (keeps the 16 + 64 offsets derived from it out of the k-loop's registers: made here, per tile)
        auto voff = [&](int r) __attribute__((always_inline)) { return lane_off + (unsigned)((r & 3) + 8 * (r >> 2)) * row_bytes; };
        // x = product * 2^-s + R (the bias came in through the accumulators); rows past M read zeros and are never stored
        {  // (the residual of block j + 1 is requested before block j is used: two 16-register sets, as in the plain epilogue)
          float rv[2][16];
          auto res_load = [&](int j, float (&dst)[16]) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc_r, voff(r), j * 128, 0));
          };
          res_load(0, rv[0]);
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            if (j + 1 < TN) res_load(j + 1, rv[(j + 1) & 1]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float v = acc[0][j][r] * w_down[j] + rv[j & 1][r];
              bad = bad || nonfinite(v);
              acc[0][j][r] = v;
            }
          }
        }
        int pass = 0;
        // sum over the row of f(element) for this lane's 16 rows: both column waves end with the same 16 totals
        auto row_totals = [&](float (&t)[16]) __attribute__((always_inline)) {
#pragma unroll
          for (int r = 0; r < 16; ++r) t[r] = half32_allsum(t[r]);
          float* slot = sX + (((pass * 2 + wm) * 2 + wn) * 2 + hb) * 16;
          if (n0 == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(slot + 4 * q) = f32x4{t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]};
          }
          __syncthreads();
          const float* other = sX + (((pass * 2 + wm) * 2 + (wn ^ 1)) * 2 + hb) * 16;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 o = *reinterpret_cast<const f32x4*>(other + 4 * q);
            t[4 * q] += o.x; t[4 * q + 1] += o.y; t[4 * q + 2] += o.z; t[4 * q + 3] += o.w;
          }
          ++pass;
        };
        // acc <- LN(acc; w, b, eps) over the 256 columns of each row
        auto layer_norm = [&](const float* __restrict__ w, const float* __restrict__ b, float eps) __attribute__((always_inline)) {
          float t[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) t[r] = (acc[0][0][r] + acc[0][1][r]) + (acc[0][2][r] + acc[0][3][r]);
          row_totals(t);
          float mean[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) mean[r] = t[r] * (1.0f / 256.0f);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float q2 = 0.f;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
              const float d = acc[0][j][r] - mean[r];
              acc[0][j][r] = d;
              q2 = fmaf(d, d, q2);
            }
            t[r] = q2;
          }
          row_totals(t);
#pragma unroll
          for (int r = 0; r < 16; ++r) t[r] = 1.0f / sqrtf(t[r] * (1.0f / 256.0f) + eps);
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const float wv = w[wn * 128 + j * 32 + n0], bv = b[wn * 128 + j * 32 + n0];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][j][r] = fmaf(acc[0][j][r] * t[r], wv, bv);
          }
        };
        if (p.ln1_w) layer_norm(p.ln1_w, p.ln1_b, p.ln1_eps);
        if (p.out1) {
          const __amdgpu_buffer_rsrc_t rsrc_o = __builtin_amdgcn_make_buffer_rsrc(p.out1 + (size_t)m_base * 256, 0, (unsigned)rows_left * row_bytes, 0x00020000);
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float y = acc[0][j][r];  // (a bit_cast applied to the vector component itself reads component 0 every time)
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), rsrc_o, voff(r), j * 128, 2);
            }
        }
        if (p.out2) {
          layer_norm(p.ln2_w, p.ln2_b, p.ln2_eps);
          // pre-split [row][K/16][16 hi | 16 lo*2^11] f16 in the bytes of the fp32 row, as the OPACK epilogue writes it
          const bool odd = lane & 1;
          const unsigned psel = split_perm_sel(lane);
          const int colf = (n0 >> 4) * 32 + (odd ? 16 + ((n0 - 1) & 15) : (n0 & 15));
          unsigned lane_pk = (unsigned)(wm * 32 + 4 * hb) * row_bytes + (unsigned)(wn * 128) * 4u + (unsigned)colf * 2u;
          asm volatile("" : "+v"(lane_pk));
          const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(p.out2 + (size_t)m_base * 256, 0, (unsigned)rows_left * row_bytes, 0x00020000);
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const unsigned outw = split_pack_exchange(pinned(acc[0][j][r]), psel, bad);
              const unsigned vo = lane_pk + (unsigned)((r & 3) + 8 * (r >> 2)) * row_bytes + (unsigned)(j * 32) * 4u;
              __builtin_amdgcn_raw_buffer_store_b32(outw, rsrc_x, vo, 0, 0);  // write-back: the next product's A operand (as ln_chain's out2)
            }
        }
        report_nonfinite(p.oflow, bad);
        li += gx;
        if (li < chunk_len) tile_coords(chunk_start + li, m_base, n_base);
        continue;
      }
      if constexpr (RS) {
        // Row-scaled A: C[m][n] = acc * 2^-s(n) * 2^e(m) + bias[n].  2^e of the tile's rows landed with the tile's first k-tile
        // (c_par has moved on to the next tile's parity since).  Row-major over the accumulators - one row scale at a time serves
        // the TN column blocks - so the epilogue holds no table of scales in registers.
        const float* sR = lds + NS * SF + 1024 + (c_par ^ 1) * 256 + wm * WM + 4 * hb;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rr = (r & 3) + 8 * (r >> 2);
            const int mm = m_base + wm * WM + i * 32 + 4 * hb + rr;
            const float up = sR[i * 32 + rr];
            if (mm < p.M) {
              float* crow = p.c_div > 0 ? p.C + (long long)(mm % p.c_div) * p.c_lo + (long long)(mm / p.c_div) * p.c_hi
                                        : p.C + (size_t)mm * p.ldc;
#pragma unroll
              for (int j = 0; j < TN; ++j) {
                const int n = n_base + wn * WN + j * 32 + n0;
                const float v = fmaf(acc[i][j][r] * w_down[j], up, b_late[j]);
                bad = bad || nonfinite(v);
                if (n < p.N) __builtin_nontemporal_store(v, crow + n);
              }
            }
          }
        report_nonfinite(p.oflow, bad);
        li += gx;
        if (li < chunk_len) tile_coords(chunk_start + li, m_base, n_base);
        continue;
      }
      if constexpr (OPACK && SINGLE) {
        // The result is the f16 A operand of the next product (fc1 -> fc2): one r16 per element.  A lane holds ONE column of 16 rows.
        // Registers r, r + 1 (r even) are adjacent rows; adjacent lanes pair up so that every lane stores one dword per two elements: even
        // lanes {(row r, n), (row r, n + 1)}, odd lanes {(row r + 1, n - 1), (row r + 1, n)}.  Buffer-form stores bounded after row M - 1: the
        // block's position is part of the lane offset, which is what the range check covers.
        const bool odd = lane & 1;
        const unsigned rows_left = (unsigned)min(p.M - m_base, BM);
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<_Float16*>(p.C) + (size_t)m_base * p.ldc, 0,
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
              bad = bad || __builtin_amdgcn_classh(h0, 0x207) || __builtin_amdgcn_classh(h1, 0x207);  // also a finite value beyond f16's 65504
              const unsigned w = __builtin_bit_cast(unsigned, h2_t{h0, h1});
              const unsigned nbr = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xf, 0xf, true);  // lane ^ 1
              const unsigned outw = odd ? ((nbr >> 16) | (w & 0xffff0000u)) : ((w & 0xffffu) | (nbr << 16));
              const int row = wm * WM + i * 32 + 4 * hb + (r & 3) + 8 * (r >> 2) + (odd ? 1 : 0);
              const unsigned vo = ((unsigned)row * p.ldc + (unsigned)(cb + (n0 & ~1))) * 2u;
              __builtin_amdgcn_raw_buffer_store_b32(outw, rsrc_c, vo, 0, 0);  // write-back: the next product's A operand
            }
          }
        }
        report_nonfinite(p.oflow, bad);
        li += gx;
        if (li < chunk_len) tile_coords(chunk_start + li, m_base, n_base);
        continue;
      } else if constexpr (OPACK) {
        // The result is itself the A operand of the next product (fc1 -> fc2): written pre-split, [row][K/16][16 hi | 16 lo*2^11]
        // f16 in the bytes of the fp32 row.  A lane holds ONE column of 16 rows; adjacent lanes pair up (DPP quad_perm) so that
        // every lane still stores one dword per element: even lanes {hi(n), hi(n+1)}, odd lanes {lo(n-1), lo(n)}.
        const bool odd = lane & 1;
        const unsigned psel = split_perm_sel(lane);
        const int colf = (n0 >> 4) * 32 + (odd ? 16 + ((n0 - 1) & 15) : (n0 & 15));  // f16 index inside the 32-column group
        // Buffer-form stores: 16 lane offsets (row r of a 32x32 block + this lane's f16 pair) serve every block; the block's position
        // is added to the lane offset (NOT passed as the scalar offset: the range check that drops the rows beyond M covers the
        // lane offset only), and the descriptor ends after row M - 1.
        const unsigned rows_left = (unsigned)min(p.M - m_base, BM);
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(p.C + (size_t)m_base * p.ldc, 0, rows_left * (unsigned)p.ldc * 4u, 0x00020000);
        unsigned voff[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) voff[r] = (unsigned)(4 * hb + (r & 3) + 8 * (r >> 2)) * (unsigned)p.ldc * 4u + (unsigned)colf * 2u;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int cb = n_base + wn * WN + j * 32;
          if (cb >= p.N) continue;  // (N % 32 == 0: a 32-column block is all in or all out)
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const unsigned so = ((unsigned)(wm * WM + i * 32) * (unsigned)p.ldc + (unsigned)cb) * 4u;  // wave-uniform
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
              f32x2 v = {acc[i][j][r] * w_down[j], acc[i][j][r + 1] * w_down[j]};
              if (ACT == 1) v = gelu_erf2(v);
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const unsigned outw = split_pack_exchange(pinned(e ? v.y : v.x), psel, bad);
                __builtin_amdgcn_raw_buffer_store_b32(outw, rsrc_c, voff[r + e] + so, 0, 2);
              }
            }
          }
        }
        report_nonfinite(p.oflow, bad);
        li += gx;
        if (li < chunk_len) tile_coords(chunk_start + li, m_base, n_base);
        continue;
      }
      // (no row map in the single-product form)
      const bool full = (m_base + BM <= p.M) && (n_base + BN <= p.N) && (SINGLE || p.c_div == 0);
      if (!SINGLE && p.c_div > 0) {  // mapped rows (GRU layer-0 input projection: (b,t) rows -> time-major)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n_base + wn * WN + j * 32 + n0;
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int mm = m_base + wm * WM + i * 32 + 4 * hb + (r & 3) + 8 * (r >> 2);
              if (n < p.N && mm < p.M) {
                float v = acc[i][j][r] * w_down[j];
                if (ACT == 1) v = gelu_erf(v);
                bad = bad || nonfinite(v);
                p.C[(long long)(mm % p.c_div) * p.c_lo + (long long)(mm / p.c_div) * p.c_hi + n] = v;
              }
            }
        }
      } else if (full) {
        // Full tile, buffer-form accesses: ONE set of 16 lane offsets (row r of a 32x32 block, this lane's column) serves every
        // block of the tile and both R and C - the block's position goes into the scalar offset - instead of a 64-bit address pair
        // per row and block.  The residual of block b + 1 is requested BEFORE block b is stored (two 16-register sets): left to
        // itself every block starts with 16 dependent loads whose latency nothing hides - 8 exposed round trips per tile.
        constexpr int NBLK = TM * TN;
        const __amdgpu_buffer_rsrc_t rsrc_c = __builtin_amdgcn_make_buffer_rsrc(p.C + (size_t)m_base * p.ldc, 0, 0xffffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsrc_r =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(RES ? p.R + (size_t)m_base * p.ldc : p.C), 0, 0xffffffff, 0x00020000);
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
            f32x2 v = {acc[i][j][r] * w_down[j], acc[i][j][r + 1] * w_down[j]};
            if constexpr (SINGLE) v = f32x2{pinned(v.x), pinned(v.y)};  // ONE fp32 product in every instantiation (never fused with the residual add)
            if (ACT == 1) v = gelu_erf2(v);
            if (RES) v += f32x2{rv[b & 1][r], rv[b & 1][r + 1]};
            // aux 2 = nt: streaming stores measure 5-9 % faster than write-back ones here
            const float vx = v.x, vy = v.y;  // (a bit_cast applied to the vector component itself reads component 0 both times)
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
            float* __restrict__ Cp = p.C + (size_t)mrow * p.ldc + n;
            const float* __restrict__ Rp = RES ? p.R + (size_t)mrow * p.ldc + n : nullptr;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {  // the same arithmetic as the full-tile path (results do not depend on tile shape)
              f32x2 v = {acc[i][j][r] * w_down[j], acc[i][j][r + 1] * w_down[j]};
              if constexpr (SINGLE) v = f32x2{pinned(v.x), pinned(v.y)};
              if (ACT == 1) v = gelu_erf2(v);
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const int rr = ((r + e) & 3) + 8 * ((r + e) >> 2);
                if (n < p.N && mrow + rr < p.M) {
                  float o = e ? v.y : v.x;
                  if (RES) o += Rp[rr * p.ldc];
                  bad = bad || nonfinite(o);
                  Cp[rr * p.ldc] = o;
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
  if (probe) {
    atomicAdd(&p.clk[0], (unsigned long long)((long long)__builtin_readcyclecounter() - pc0));
    atomicAdd(&p.clk[1], (unsigned long long)((long long)wall_clock64() - pw0));
  }
}

// ---- host side shared by the two forms' launchers -------------------------------------------------------------------------
// The persistent grid: at most `cap` workgroups (a test aid; 0 = none), then a multiple of 8 (the XCD chunking) ...
static inline int capped_grid(long long g, int cap) {
  if (cap > 0 && g > cap) g = cap;
  return (int)((g + 7) & ~7ll);
}
// ... of a tile shape: one workgroup per tile up to the two or three per CU that its LDS allows
static inline int persistent_grid(long long tiles, int lds_bytes, int cap) {
  const int per_cu = (160 * 1024) / lds_bytes >= 3 ? 3 : 2;
  return capped_grid(tiles < 256 * per_cu ? tiles : 256 * per_cu, cap);
}
// Tile choice on large grids: a launch takes as long as its busiest CU (tiles are spread evenly over an XCD's 32 CUs, two or three
// workgroups per CU sharing one matrix pipe); `ovh` is the per-area handicap of the smaller wave tiles (operand traffic and vector work
// per matrix instruction), measured per kernel form.
struct GemmTile { int bm, bn; double ovh; };
static inline int cheapest_tile(const GemmTile (&tiles)[3], int M, int N) {
  int best = 0;
  double best_cost = 1e300;
  for (int i = 0; i < 3; ++i) {
    const GemmTile& t = tiles[i];
    const long long n = (long long)((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
    const long long per_cu = ((n + 7) / 8 + 31) / 32;
    const double cost = (double)per_cu * t.bm * t.bn * t.ovh;
    if (cost < best_cost) { best_cost = cost; best = i; }
  }
  return best;
}

// The packers' power of two for a row whose largest magnitude is m = f * 2^e, f in [0.5, 1): up = 2^(15 - e) lifts m into [2^14, 2^15) and
// down = 2^(e - 15) undoes it; e is clamped so that both are normal fp32 numbers.  (Whether a zero or non-finite row is scaled at all is the
// caller's rule.)
__device__ __forceinline__ void row_pow2(float m, float& up, float& down) {
  int e = 0;
  if (m > 0.f && m < 3.0e38f) frexpf(m, &e);
  e = max(-110, min(e, 125));
  up = ldexpf(1.f, 15 - e);
  down = ldexpf(1.f, e - 15);
}
