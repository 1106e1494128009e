// Shared pieces of the three-product f16 GEMM kernels (gemm_split_f16.hip: the persistent 4-wave tiles; gemm_split_small.hip: the
// small-grid form) and of the matrix-pipe attention.  Arithmetic and operand layout: see the header of gemm_split_f16.hip.
#pragma once
#include "common.hpp"

struct SplitParams {
  const float* A;       // fp32 [M][lda], or packed planes [M][K/16][16 hi | 16 lo*2^11] f16 (APACK)
  const float* W;       // packed planes [N][K/16][16 hi | 16 lo] f16 of W[n] * 2^s(n)
  int wblk;             // W is in the BLOCKED layout [N/64][K/16][64 rows][16 hi | 16 lo] (pmce_gemm_pack_split_f16, blocked): a tile's k-slice is
                        // contiguous 4 KB pieces instead of 64-byte pieces one weight row (K * 4 bytes) apart
  const float* wscale;  // [N]: 2^-s(n), one power of two per OUTPUT row of W (pmce_gemm_pack_split_f16)
  const float* bias;    // [N] or null
  const float* rscale;  // [M] or null: 2^e(m) per ROW of a packed A that was stored as A[m] * 2^-e(m) (pmce_split_rows_scaled_f16): the
                        // epilogue multiplies row m by it and adds the bias AFTER the scaling (RS instantiations)
  const float* R;       // residual [M][ldc] or null
  float* C;
  // (The single-product form, gemm_f16.hip, fills the same fields: A = f16 [M][lda], W = f16 blocked [ceil(N/64)][K/32][64][32], wblk = 1,
  // C = fp32 or f16 [M][ldc]; lda and ldc count elements of those types.)
  int M, N, K;
  unsigned lda, ldc;
  int ntm, ntn;
  int c_div;             // > 0: C row r lives at (r % c_div) * c_lo + (r / c_div) * c_hi (elements); never with R
  long long c_lo, c_hi;
  unsigned long long* clk;  // optional probe {shader clocks, 100 MHz ticks}: each workgroup's first wave adds its kernel residence (null = off)
  unsigned* oflow;  // device-visible word set to 1 when a result is not finite (an activation beyond f16's 65504, or fp32 overflow); may be null
  // LayerNorm epilogue (LNEP instantiation; N == 256 == the tile's width, so a workgroup owns whole rows): with x = the product + bias + R,
  //   y1 = ln1_w ? LN(x; ln1_w, ln1_b, ln1_eps) : x ;  out1 = y1 (fp32, if out1) ;  out2 = LN(y1; ln2_w, ln2_b, ln2_eps) pre-split (if out2)
  // - what pmce_ln_chain does to the product's result in a launch of its own.  C is not written.
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
  float ln1_eps, ln2_eps;
  float *out1, *out2;
};

// 1 / x for x = 2^e, e in [-126, 126], exactly: the exponent field mirrored around the bias
__device__ __forceinline__ float pow2_recip(float x) { return __uint_as_float(0x7f000000u - __float_as_uint(x)); }

// exponent field all ones: infinity or NaN
__device__ __forceinline__ bool nonfinite(float v) { return __builtin_amdgcn_class(v, 0x207); }  // signalling / quiet NaN, -inf, +inf (0x203, until round 6, lacked the -inf bit)
__device__ __forceinline__ void report_nonfinite(unsigned* sink, bool lane_saw_one) {
  if (sink && __builtin_amdgcn_ballot_w64(lane_saw_one) != 0ull && (threadIdx.x & 63) == 0) *reinterpret_cast<volatile unsigned*>(sink) = 1u;
}

// One element of a PRE-SPLIT result: x -> (hi, lo * 2^11) f16 in one dword, exchanged with the neighbour lane (lane ^ 1) so that even lanes store
// {hi(n), hi(n + 1)} and odd lanes {lo(n - 1), lo(n)} - the layout [16 hi | 16 lo] of a 16-column group.  perm_sel = split_perm_sel(lane).
// Round 6: 20 instead of 25 vector instructions per element beside the GELU (v_pack_b32_f16, v_perm_b32, the class test on the f16 itself) -
// the epilogue's vector work costs the CU's other workgroup matrix time.  The same bits as the shift / mask form it replaces.
__device__ __forceinline__ unsigned split_perm_sel(int lane) { return (lane & 1) ? 0x03020706u : 0x05040100u; }
__device__ __forceinline__ unsigned split_pack_exchange(float x, unsigned perm_sel, bool& bad) {
  typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
  const _Float16 h = (_Float16)x;
  bad = bad || __builtin_amdgcn_classh(h, 0x207);  // inf / nan: also a finite x beyond f16's 65504 - the next product could not read it
  const _Float16 l = lo_plane(x, h);  // the fused form: same bits as the plain one for every x whose hi is finite
  const unsigned w = __builtin_bit_cast(unsigned, h2_t{h, l});
  const unsigned nbr = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xf, 0xf, true);  // lane ^ 1
  return __builtin_amdgcn_perm(nbr, w, perm_sel);
}

// gemm_split_small.hip: the small-grid form (one 64 x 128 tile per workgroup, eight waves, at most one round of workgroups)
// pmce_gemm_split_small_nwn: 2 (the 64 x 64 tile), 4 (64 x 128) or 0 (no small-grid form for this product) - the ONE decision both the
// launch and pmce_gemm_split_path take.
int pmce_gemm_split_small_nwn(int M, int N, int K, int act, bool apack, bool opack, bool res, bool rs);
int pmce_gemm_split_small_launch(SplitParams& p, int nwn, bool apack, bool opack, hipStream_t stream);
