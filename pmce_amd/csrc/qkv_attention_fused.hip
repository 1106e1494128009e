// The qkv product and the attention of a TEMPORAL lifter block (C = 512: 8 heads of 64 channels; sequences of 16 frames) in one kernel,
// split-f16 mode: what pmce_gemm_nt_split_f16(XN -> QKV) followed by pmce_seq_attention_split_f16(QKV -> AO) compute, bit for bit, without
// the [M, 3C] fp32 tensor between them (428 MB written and 571 MB read back per block at B = 256, and a launch of 106-111 us behind a
// product of 316 us).  Compiled as part of seq_attention_mfma.hip (included at its end): the two share split8_fused and the softmax is
// the same formula, and tests/test_host_logic.py pins the set of objects that carry f16 matrix instructions.
//
// Work unit = 8 sequences (128 gathered rows of XN; a 16-row group is one sequence) x one head: the product [128 x 512] x [512 x 192]
// against the head's q, k and v rows of the packed weight - three 64-row blocks of the blocked layout, used as they lie.  Four waves
// stacked along M; a wave owns 32 rows = TWO whole sequences and all 192 columns: six 32x32 accumulator blocks (96 registers).
// B = 256, J = 17: 544 tiles x 8 heads = 4,352 units on 512 persistent workgroups (two per CU).  Units are independent: no flags, no
// atomics.  Each XCD walks its own contiguous chunk of tiles with all 8 heads, so a tile of XN is fetched from HBM once and the 3 MB
// weight stays in the XCD's L2.
//
// k-loop: gemm_split_kernel's (gemm_split_f16.hip) - LDS-DMA ring with the same XOR swizzle, counted vmcnt, one barrier per k-tile, the
// stream of k-tiles running across unit boundaries, the unit's bias and 2^-s slices riding in with its first k-tile, the three f16
// products per k-tile in the same order (hi hi, hi lo, lo hi*2^-11) into ONE accumulator per element.  14 ds_read_b128 per 18 matrix
// instructions and wave (the 128x256 tile: 12 per 24).
//
// Accumulator layouts, chosen so that nothing is transposed through LDS:
//   * q and k: the product with EXCHANGED operands (W fragment as A, activation fragment as B): lane (token, hb) holds channels
//     32 b + 4 hb + (r & 3) + 8 (r >> 2).  The matrix instruction gives the same bits either way round (tests/test_gpu_qkv_attention_fused.py
//     checks it on the hardware).  One v_permlane32_swap per register pair (r, r + 4) turns that into 8 CONSECUTIVE channels
//     16 ks + 8 hb + [0, 8) per lane - exactly the K (A operand) and Q (B operand) fragments of seq_attention_mfma's S^T = K Q^T.
//   * v: the product as the GEMM does it: lane = channel, register r = token 4 hb + (r & 3) + 8 (r >> 2) of sequence r >> 3 - the key
//     order of the A operand of out^T = V^T P^T.
// Attention: seq_attention_mfma's, operation for operation (split8_fused, hi.hi and cross accumulators, log2-scaled two-pass softmax
// in-lane + one lane ^ 32 exchange, P split once, 1 / sum at the end).  The wave's two sequences share one 32x32 score tile; a lane
// (= one query) SELECTS the 8 registers of its own sequence's keys (v_cndmask - the other 8, the cross-sequence scores, are dropped
// like keys >= N are masked there), and out^T is computed once per sequence (V^T of sequence 0, of sequence 1: 12 matrix instructions
// per head, as there) and selected per lane likewise.  Selecting - not multiplying by p = 0 - keeps a non-finite row from reaching the
// other sequence of its wave.  The softmax' exponent is fma(t, scale, -max) with max taken over the ROUNDED t * scale: what hipcc's
// contraction makes of seq_attention_mfma's source; spelled out here so that the two stay the same bits.
// The result leaves pre-split: the lane halves exchange their (hi, lo) dwords (v_permlane32_swap again) so that every lane stores 16
// contiguous bytes - hb = 0 the hi plane of 8 channels, hb = 1 the lo plane - 8 stores per lane and unit, no LDS staging.
//
// Budget.  LDS: ring of NS = 3 stages x (128 + 192) rows x 64 B = 60 KB + two {bias, 2^-s} slice pairs of 2 x 1 KB = 64 KB; two
// workgroups per CU = 128 of 160 KB (NS = 4: 84 KB, does not fit twice).  Registers: 96 accumulators + 8 (A fragments) + up to 72 (W
// fragments hi, lo, hi*2^-11 of six blocks) in the k-loop; in the attention 32 (q planes) + 32 (k) + 32 (scores) + the v accumulators, then 16 (v planes of one block) + 64 (out^T of both
// sequences, main and cross) while the product's accumulators die block by block: under the 256 of two waves per SIMD.
// (Compiled: 221 registers, no scratch.  The non-finite test is a wave-wide ballot per result: a lazily combined per-lane flag kept every
// tested value alive and spilled 72 registers, with scratch reloads in the k-loop whose waits drained the DMA ring.)
// Measured, B = 256 (profiles/qaf_*): 369 us per launch against 338 (qkv product) + 109 (attention) = 447 us; the operator alone 325 against
// 434 us; faster than the two launches from ~400 units on, slower below (the model switches at 512 units, model.cpp).
// Non-finite results set the overflow sink (a non-finite q, k or v - an operand beyond the f16 range included - always makes one).

namespace {

struct QkvAttnParams {
  const float* A;       // XN pre-split [rows][C/16][16 hi | 16 lo*2^11] f16
  const float* W;       // the qkv weight, packed BLOCKED [3C/64][C/16][64 rows][16 hi | 16 lo] f16 (q rows, k rows, v rows)
  const float* wscale;  // [3C] 2^-s per weight row
  const float* bias;    // [3C] or null
  float* out;           // AO pre-split [rows][C/16][16 hi | 16 lo*2^11] f16
  int nseq, ntiles, J;  // sequence s = (b, j) = (s / J, s % J); its frame t is row (b * 16 + t) * J + j
  unsigned* oflow;
};

struct QaCfg {
  static constexpr int C = 512, NTOK = 16, NK = C / 16;
  static constexpr int BM = 128, BN = 192, NS = 3;
  static constexpr int STAGE_FLOATS = (BM + BN) * 16;
  static constexpr int DPW = (BM + BN) / 64;  // DMA instructions per wave and k-tile (16 rows each): 2 of A, 3 of W
  static constexpr int LDS_BYTES = NS * STAGE_FLOATS * 4 + 4096;
};

__global__ __launch_bounds__(256, 2) void qkv_attention_fused_kernel(QkvAttnParams p) {
  using Cfg = QaCfg;
  constexpr int C = Cfg::C, NK = Cfg::NK, NS = Cfg::NS, SF = Cfg::STAGE_FLOATS, DPW = Cfg::DPW, BM = Cfg::BM;
  extern __shared__ __attribute__((aligned(16))) float lds_qa[];
  float* const lds = lds_qa;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = lane & 31, hb = lane >> 5;

  // ---- persistent workgroups; XCD x owns a contiguous chunk of tiles, unit v of the chunk = (tile v / 8, head v % 8) ----
  const XcdChunk chunk = xcd_chunk(p.ntiles);
  const int chunk_start = chunk.start, chunk_units = chunk.len * 8, bx = chunk.bx, gx = chunk.gx;
  if (bx >= chunk_units) return;
  const int my_units = (chunk_units - bx + gx - 1) / gx;
  const int total = my_units * NK;

  const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), 0, 0xffffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.W), 0, 0xffffffff, 0x00020000);

  // row of frame t of sequence seq (rows < 2^21: checked by the launcher)
  auto token_row = [&](int seq, int t) { const int b = seq / p.J; return (unsigned)((b * Cfg::NTOK + t) * p.J + (seq - b * p.J)); };

  // ---- DMA side, as gemm_split_kernel: instruction q of a wave moves row group g = wave + 4 q of a stage (groups 0..7: the tile's 8
  // sequences; 8..19: the head's q, k, v rows), lane L -> row 16 g + (L >> 2), physical chunk L & 3 = logical chunk (L & 3) ^ ((L >> 4) & 3) ----
  const int drow = lane >> 2;
  const unsigned dchunk = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 4);  // floats
  unsigned doff[DPW];
  unsigned slice_off = 0;  // this lane's 16 bytes of the unit's bias / 2^-s slice: 64 floats each of the q, k and v rows (lanes 48..63 repeat v's)
  auto set_ptrs = [&](int v) {
    const int tile = chunk_start + (v >> 3), head = v & 7;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int seq = min(tile * 8 + wave + 4 * q, p.nseq - 1);  // (a ragged tile repeats the last sequence; its copies are not stored)
      doff[q] = (token_row(seq, drow) * (unsigned)C + dchunk) * 4u;
    }
#pragma unroll
    for (int q = 2; q < DPW; ++q) {  // part q - 2 (q, k, v) of the weight: 64-row block (q - 2) * 8 + head, this wave's 16 rows of it
      const unsigned blk = (unsigned)((q - 2) * 8 + head), r = (unsigned)(16 * wave + drow);
      doff[q] = (blk * (unsigned)(NK * 1024) + r * 16u + dchunk) * 4u;
    }
    slice_off = (unsigned)((min(lane >> 4, 2) * C + head * 64 + (lane & 15) * 4) * 4);
  };
  const unsigned lds0 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) float*)lds;
  const unsigned lds_wave = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);
  auto issue = [&](int kt, int stage) {
    const unsigned stage_base = lds_wave + stage * (SF * 4);
#pragma unroll
    for (int q = 0; q < DPW; ++q) {
      const bool is_a = q < 2;
      sdma16o(is_a ? rsrc_a : rsrc_w, doff[q], is_a ? kt * 64 : kt * 4096, stage_base, q * 4096);
    }
  };

  // issue-side cursor (NS - 1 k-tiles ahead of the compute side, across unit boundaries)
  int i_v = bx, i_kt = 0, i_stage = 0, issued = 0, i_par = 0;
  set_ptrs(i_v);
  auto issue_next = [&]() {
    if (i_kt == 0) {  // the unit's bias and 2^-s slices (descriptors made here, once per unit: not held in scalar registers through the k-loop)
      if (wave == 0)  // bounded: without a bias every lane reads zeros
        lds_dma16(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? 3 * C * 4 : 0, 0x00020000), slice_off, 0,
                  lds0 + NS * SF * 4 + i_par * 2048);
      if (wave == 1)
        lds_dma16(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wscale), 0, 3 * C * 4, 0x00020000), slice_off, 0,
                  lds0 + NS * SF * 4 + i_par * 2048 + 1024);
      i_par ^= 1;
    }
    issue(i_kt, i_stage);
    ++issued;
    i_stage = i_stage + 1 == NS ? 0 : i_stage + 1;
    if (++i_kt == NK) {
      i_kt = 0;
      i_v += gx;
      if (i_v < chunk_units) set_ptrs(i_v);
    }
  };
#pragma unroll
  for (int q = 0; q < NS - 1; ++q)
    if (issued < total) issue_next();

  const int swz = (n0 >> 2) & 3;
  const int a_row = (wave * 32 + n0) * 16, w_row = BM * 16 + n0 * 16;  // floats inside a stage
  const int ch = 4 * (hb ^ swz), cl = 4 * ((2 + hb) ^ swz);             // hi / lo plane, k = 8 hb + [0, 8)

  // acc[0..1]: q channels [0, 32), [32, 64) of the head; acc[2..3]: k; (exchanged operands: lane = token)   acc[4..5]: v (lane = channel)
  f32x16 acc[6];
  float w_down_v[2];
  int c_v = bx, kt = 0, stage = 0, c_par = 0;
  constexpr float scale = 0.125f * 1.44269504088896340736f;  // hd^-0.5 * log2(e), as seq_attention_mfma
  constexpr float two_m11 = 0.00048828125f;
  const bool sb = (n0 & 16) != 0;  // this lane's token belongs to the wave's second sequence

  for (int it = 0; it < total; ++it) {
    // k-tile `it` has landed when at most (younger batches) x DPW of this wave's DMAs are still in flight (loads complete in order; the
    // previous unit's result stores and the slice DMAs only make the wait stricter)
    if (issued - it - 1 >= 1) wait_vm<DPW>();
    else wait_vm<0>();
    __syncthreads();  // every wave's part of k-tile `it` is in LDS; every wave is done reading the stage of k-tile it - 1
    if (issued < total) issue_next();

    if (kt == 0) {  // bias * 2^s is the accumulators' initial value, as in the GEMM
      const float* sB = lds + NS * SF + c_par * 512;
      c_par ^= 1;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(sB + j * 32 + 8 * rq + 4 * hb);
          const f32x4 s = *reinterpret_cast<const f32x4*>(sB + 256 + j * 32 + 8 * rq + 4 * hb);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[j][4 * rq + e] = b[e] * pow2_recip(s[e]);
        }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        w_down_v[j] = sB[256 + 128 + j * 32 + n0];
        const float bv = sB[128 + j * 32 + n0] * pow2_recip(w_down_v[j]);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[4 + j][r] = bv;
      }
    }
    {
      const float* sA = lds + stage * SF;
      const f16x8 ahi = *reinterpret_cast<const f16x8*>(sA + a_row + ch);
      const f16x8 alo = *reinterpret_cast<const f16x8*>(sA + a_row + cl);
      f16x8 whi[6], wlo[6], wh2[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        whi[j] = *reinterpret_cast<const f16x8*>(sA + w_row + j * 512 + ch);
        wlo[j] = *reinterpret_cast<const f16x8*>(sA + w_row + j * 512 + cl);
        wh2[j] = whi[j] * (_Float16)0.00048828125f;  // 2^-11: undoes the scale of alo
      }
#pragma unroll
      for (int j = 0; j < 6; ++j)
        acc[j] = j < 4 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(whi[j], ahi, acc[j], 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, whi[j], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 6; ++j)
        acc[j] = j < 4 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo[j], ahi, acc[j], 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, wlo[j], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 6; ++j)
        acc[j] = j < 4 ? __builtin_amdgcn_mfma_f32_32x32x16_f16(wh2[j], alo, acc[j], 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, wh2[j], acc[j], 0, 0, 0);
    }

    stage = stage + 1 == NS ? 0 : stage + 1;
    if (++kt == NK) {
      // ---- the unit's attention, straight from the accumulators ----
      kt = 0;
      unsigned long long bad = 0;  // a non-finite q, k or v (an operand beyond the f16 range included) always reaches a result: those are tested
      const float* sS = lds + NS * SF + (c_par ^ 1) * 512 + 256;  // the unit's 2^-s slice (c_par has moved on)
      // q, k: scale, exchange 4-channel groups between the lane halves, split.  Index ks = the head's 16-channel group.
      f16x8 qh[4], ql[4], kh[4], kl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float val[16];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const f32x4 s = *reinterpret_cast<const f32x4*>(sS + j * 32 + 8 * rq + 4 * hb);
#pragma unroll
          for (int e = 0; e < 4; ++e) val[4 * rq + e] = acc[j][4 * rq + e] * s[e];
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          // registers 8 g + e hold channel 16 g + 4 hb + e, registers 8 g + 4 + e channel 16 g + 8 + 4 hb + e: after the swap the first
          // set is channel 16 g + 8 hb + e and the second 16 g + 8 hb + 4 + e
          f32x4 x0, x1;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, val[8 * g + e]),
                                                             __builtin_bit_cast(unsigned, val[8 * g + 4 + e]), false, false);
            x0[e] = __builtin_bit_cast(float, (unsigned)sw[0]);
            x1[e] = __builtin_bit_cast(float, (unsigned)sw[1]);
          }
          const int ks = 2 * (j & 1) + g;
          if (j < 2) split8_fused(x0, x1, qh[ks], ql[ks]);
          else split8_fused(x0, x1, kh[ks], kl[ks]);
        }
        __builtin_amdgcn_sched_barrier(0);  // block by block: the planes take the accumulators' registers, nothing is held twice
      }
      // ---- S^T = K Q^T: rows = the 32 keys of both sequences, columns = the 32 queries ----
      f32x16 s_main, s_cross;
#pragma unroll
      for (int r = 0; r < 16; ++r) s_main[r] = s_cross[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s_main = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[ks], qh[ks], s_main, 0, 0, 0);
        s_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[ks], ql[ks], s_cross, 0, 0, 0);
        s_cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl[ks], qh[ks], s_cross, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- softmax over the 16 keys of this lane's query: register 8 sb + e is key 4 hb + (e & 3) + 8 (e >> 2) of its own sequence ----
      float t[8], pr[8];
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float sm = sb ? s_main[8 + e] : s_main[e];
        const float sc = sb ? s_cross[8 + e] : s_cross[e];
        t[e] = fmaf(sc, two_m11, sm);
        mx = fmaxf(mx, pinned(t[e] * scale));
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pr[e] = __builtin_amdgcn_exp2f(fmaf(t[e], scale, -mx));
        sum += pr[e];
      }
      sum += __shfl_xor(sum, 32);
      const float inv = 1.0f / sum;
      f16x8 ph, pl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float pv32 = pinned(pr[e]);
        ph[e] = (_Float16)pv32;
        pl[e] = lo_plane(pv32, ph[e]);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- out^T = V^T P^T per 32-channel block and sequence; the lane keeps its own sequence's; stored pre-split ----
      const int tile = chunk_start + (c_v >> 3), head = c_v & 7;
      const int seq = tile * 8 + wave * 2 + (n0 >> 4);
      float* const orow = p.out + (size_t)token_row(min(seq, p.nseq - 1), n0 & 15) * C + head * 64 + hb * 8;
      const bool live = seq < p.nseq;
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        // v of the block, per sequence: the 8 registers of a sequence are its keys in the order of P^T's registers
        f16x8 vh[2], vl[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float x[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            x[e] = pinned(acc[4 + blk][8 * s + e] * w_down_v[blk]);
            vh[s][e] = (_Float16)x[e];
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) vl[s][e] = lo_plane(x[e], vh[s][e]);
        }
        f32x16 om[2], oc[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
          for (int r = 0; r < 16; ++r) om[s][r] = oc[s][r] = 0.f;
          om[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[s], ph, om[s], 0, 0, 0);
          oc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[s], pl, oc[s], 0, 0, 0);
          oc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl[s], ph, oc[s], 0, 0, 0);
        }
        // register 4 rq + e is channel 32 blk + 8 rq + 4 hb + e of query n0
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          f16x4 oh, ol;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float m = sb ? om[1][4 * rq + e] : om[0][4 * rq + e];
            const float c = sb ? oc[1][4 * rq + e] : oc[0][4 * rq + e];
            const float v = pinned(fmaf(c, two_m11, m) * inv);
            bad |= __builtin_amdgcn_ballot_w64(nonfinite(v));  // (a wave-wide mask, evaluated here: a lazily combined flag keeps every v alive)
            oh[e] = (_Float16)v;
            ol[e] = lo_plane(v, oh[e]);
          }
          // hb = 0 keeps its hi pair and takes the partner's (channels + 4): 16 bytes of the hi plane; hb = 1 likewise the lo plane
          typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
          typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
          const u32x2 h2 = __builtin_bit_cast(u32x2, oh), l2 = __builtin_bit_cast(u32x2, ol);
          const auto s0 = __builtin_amdgcn_permlane32_swap(h2[0], l2[0], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(h2[1], l2[1], false, false);
          const u32x4 piece = {(unsigned)s0[0], (unsigned)s1[0], (unsigned)s0[1], (unsigned)s1[1]};
          // 16-channel group 2 blk + (rq >> 1) = 16 floats of the row; inside it hi at f16 8 (rq & 1), lo 16 f16 further (hb * 8 floats)
          if (live) *reinterpret_cast<u32x4*>(orow + (2 * blk + (rq >> 1)) * 16 + (rq & 1) * 4) = piece;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (p.oflow && bad != 0ull && lane == 0) *reinterpret_cast<volatile unsigned*>(p.oflow) = 1u;
      c_v += gx;
    }
  }
}

}  // namespace

extern "C" int pmce_qkv_attention_fused_split_f16(const float* xn_planes, const float* Wp, const float* wscale, const float* bias, float* out_planes,
                                                  int B, int J, int C, unsigned* overflow_word, hipStream_t stream) {
  using Cfg = QaCfg;
  PMCE_REQUIRE(xn_planes && Wp && wscale && out_planes && B > 0 && J > 0, "qkv_attention_fused_split_f16: bad arguments");
  PMCE_REQUIRE(C == Cfg::C, "qkv_attention_fused_split_f16: C must be 512 (got %d)", C);
  // the kernel addresses the rows of XN with 32-bit byte offsets
  PMCE_REQUIRE((long long)B * Cfg::NTOK * J * C * 4 < (1ll << 32), "qkv_attention_fused_split_f16: the operand spans 4 GiB or more (split the batch)");
  QkvAttnParams p;
  p.A = xn_planes; p.W = Wp; p.wscale = wscale; p.bias = bias; p.out = out_planes;
  p.nseq = B * J; p.ntiles = (p.nseq + 7) / 8; p.J = J;
  p.oflow = overflow_word ? overflow_word : pmce_overflow_sink();
  static std::atomic<unsigned long long> done{0};
  PMCE_TRY(pmce_opt_in_lds(reinterpret_cast<const void*>(&qkv_attention_fused_kernel), Cfg::LDS_BYTES, done, "qkv_attention_fused_split_f16"));
  const int units = p.ntiles * 8;  // (a multiple of 8, as the kernel's XCD arithmetic needs of the grid)
  const int grid = units < 512 ? units : 512;
  hipLaunchKernelGGL(qkv_attention_fused_kernel, dim3(grid), dim3(256), Cfg::LDS_BYTES, stream, p);
  return pmce_check_launch("qkv_attention_fused_split_f16");
}
