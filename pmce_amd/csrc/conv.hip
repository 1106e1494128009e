// The feature extractor's operators (reference lib/models/spin.py:18-143, the ResNet-50 backbone of the demo): an implicit-GEMM convolution
// on the f16 matrix pipe with the project's three-product split, the 3 x 3 / 2 max pool and the global average pool.  fp32 NHWC results.
//
//     out[m][n] = relu?( 2^-s(n) (Ahi Whi + Ahi Wlo + Alo Whi) + bias[n] + R[m][n]? )       m = (image, oy, ox), n = Cout, k = (ky, kx, cin)
//
// Weights: split ONCE (pmce_conv_pack_split_f16) from BatchNorm-folded fp32 OIHW weights into the blocked plane layout of the split GEMM,
// [ceil(Cout / 64)][Kp / 16][64 rows][16 hi | 16 lo] f16 of W[n] * 2^s(n), k in the order (ky, kx, cin), K = KH KW Cin padded with zero
// weights to Kp = a multiple of 32 (the stem: 147 -> 160) and the rows past Cout written as zeros; wscale[n] = 2^-s(n) lifts a row's
// largest |w| into [2^14, 2^15) exactly as pmce_gemm_pack_split_f16 does.
// Activations: fp32 in memory, addressed by four element strides (image, channel, row, column) - the stem reads the NCHW patches of
// pmce_crop_patches as they are, every later layer NHWC -, gathered into registers with the zero padding as a predicate of the load,
// split into (hi, lo * 2^11) while they are stored to LDS (lo_plane of common.hpp: a value beyond f16's range gives hi = inf, lo = -inf and
// a NaN / inf in every output that reads it, never a wrong finite number).
// Tile: 128 output pixels x 64 output channels per workgroup of four waves; a wave owns 32 pixels x the tile's 64 channels (one A fragment
// feeds two accumulators: the split of an activation is vector work, which costs matrix time on this chip, and is paid once per 6 matrix
// instructions).  A stage is two k-tiles of 16; two stages in LDS (48 KB: three workgroups per CU); the next stage's global loads are in
// flight in registers while the matrix instructions of the current one run; one barrier per stage.  The kernel is written for NT column
// sub-tiles per wave; a 128-wide tile (NT = 4, 64 KB, two workgroups per CU) was measured slower on every layer of the network - 7.17
// against 6.45 ms per batch of 64 over the 53 convolutions, profiles/extractor_bench.json's workload - and is not instantiated.
//   FAST (channel stride 1, Cin % 16 == 0, 16-byte aligned rows): a k-tile lies inside one tap and is 64 contiguous bytes per pixel:
//        one 16-byte load per thread and row, the tap arithmetic is scalar.
//   generic (the stem, Cin = 3): every element is its own predicated load; k -> (ky, kx, c) by division.  3 % of the network's work.
// Epilogue: v = 2^-s(n) acc + bias[n]; then act(v + R) (the bottleneck's order) or act(v) + R (darknet's shortcut), act = none, ReLU or
// leaky with a slope; the result's and the residual's rows have their own pitches, so both may be channel slices of wider NHWC buffers
// (the detector's concatenations are written in place).  pmce_conv2d_split_f16 is the case (ReLU or none, R first, pitch = Cout).
// Order of summation: an output element is ONE accumulator register that takes the k-tiles 0, 1, 2, ... in turn, three matrix
// instructions each in a fixed order, whatever the batch, the tile it falls into or its place in the tile: results are bit-identical
// whatever n is (tests/test_gpu_conv.py T2).
#include "gemm_split_common.hpp"

namespace {

struct ConvParams {
  const float* X;
  long long sn, sc, sy, sx;  // element strides of the input: image, channel, row, column
  int H, W, Cin, OH, OW, KH, KW, stride, pad;
  const float* Wp;      // packed planes (see above)
  const float* wscale;  // [Cout] 2^-s(n)
  const float* bias;    // [Cout] or null
  const float* R;       // residual, row m at R + m ldr, or null
  float* out;           // row m at out + m ldo
  long long ldo, ldr;   // row pitches in floats (>= Cout): a channel slice of a wider NHWC buffer
  int M, N, K, KT;      // M = n OH OW, N = Cout, K = KH KW Cin, KT = Kp / 16
  int ntn;              // column tiles
  int act;              // CONV_ACT_NONE / _RELU / _LEAKY
  float slope;          // of the leaky activation
  int res_after;        // 0: act(v + R) (ResNet's bottleneck); 1: act(v) + R (darknet's shortcut)
  unsigned* oflow;      // set to 1 when a result is not finite; may be null
};

constexpr int CONV_BM = 128;
constexpr int CONV_ACT_NONE = 0, CONV_ACT_RELU = 1, CONV_ACT_LEAKY = 2;

template <int NT, bool FAST>
__global__ __launch_bounds__(256) void conv_split_kernel(ConvParams p) {
  constexpr int BN = 32 * NT;
  constexpr int A_BYTES = CONV_BM * 64, SUB = A_BYTES + BN * 64, STAGE = 2 * SUB;  // one k-tile: [A rows of 64 B | W rows of 64 B]
  constexpr int WCH = NT;  // 16-byte weight chunks per thread and stage: 2 * BN * 4 / 256
  extern __shared__ __attribute__((aligned(16))) char conv_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = lane & 31, hb = lane >> 5;
  const int tn = blockIdx.x % p.ntn, tm = blockIdx.x / p.ntn;  // the column tiles of one row tile are neighbours: they share its A in L2
  const int m_base = tm * CONV_BM, n_base = tn * BN;

  // ---- gather side: thread (r = tid / 4, q = tid % 4) stages floats 4 q .. 4 q + 3 of the k-tile for the rows r and r + 64 ----
  const int gr = tid >> 2, gq = tid & 3;
  const float* gbase[2];
  int iy0[2], ix0[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int m = m_base + gr + 64 * u;
    const int mc = min(m, p.M - 1);
    const int img = mc / (p.OH * p.OW), rem = mc - img * (p.OH * p.OW);
    const int oy = rem / p.OW, ox = rem - oy * p.OW;
    gbase[u] = p.X + (long long)img * p.sn;
    iy0[u] = m < p.M ? oy * p.stride - p.pad : -(1 << 20);  // a row past M fails every bounds test: it stages zeros
    ix0[u] = ox * p.stride - p.pad;
  }
  auto load_a = [&](int kt, f32x4 (&v)[2]) {
    const int k0 = kt * 16;
    if constexpr (FAST) {
      const int tap = k0 / p.Cin, c0 = k0 - tap * p.Cin, ky = tap / p.KW, kx = tap - ky * p.KW;  // wave-uniform
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int iy = iy0[u] + ky, ix = ix0[u] + kx;
        const bool ok = k0 < p.K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) v[u] = *reinterpret_cast<const f32x4*>(gbase[u] + (long long)iy * p.sy + (long long)ix * p.sx + (c0 + 4 * gq));
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 4 * gq + e;
        const int tap = k / p.Cin, c = k - tap * p.Cin, ky = tap / p.KW, kx = tap - ky * p.KW;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int iy = iy0[u] + ky, ix = ix0[u] + kx;
          const bool ok = k < p.K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
          float x = 0.f;
          if (ok) x = gbase[u][(long long)iy * p.sy + (long long)ix * p.sx + (long long)c * p.sc];
          v[u][e] = x;
        }
      }
    }
  };
  // LDS image of a k-tile row: four 16-byte chunks {hi k 0-7, hi k 8-15, lo k 0-7, lo k 8-15}, chunk c at physical chunk c ^ ((row >> 2) & 3)
  auto store_a = [&](char* sub, const f32x4 (&v)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = gr + 64 * u, sw = (row >> 2) & 3;
      f16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) hi[e] = (_Float16)v[u][e];
#pragma unroll
      for (int e = 0; e < 4; ++e) lo[e] = lo_plane(v[u][e], hi[e]);
      char* rowp = sub + row * 64 + (gq & 1) * 8;
      *reinterpret_cast<f16x4*>(rowp + (((gq >> 1) ^ sw) << 4)) = hi;
      *reinterpret_cast<f16x4*>(rowp + (((2 + (gq >> 1)) ^ sw) << 4)) = lo;
    }
  };
  // weights: chunk i = tid + 256 j of the stage's 2 * BN * 4 chunks -> (k-tile s, row, chunk ch)
  const int nblocks = (p.N + 63) >> 6;
  auto load_w = [&](int st, f32x4 (&w)[WCH]) {
#pragma unroll
    for (int j = 0; j < WCH; ++j) {
      const int i = tid + 256 * j, s = i / (BN * 4), rc = i - s * (BN * 4), row = rc >> 2, ch = rc & 3;
      const int nb = (n_base + row) >> 6;
      w[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (nb < nblocks)
        w[j] = *reinterpret_cast<const f32x4*>(p.Wp + (((size_t)nb * p.KT + (2 * st + s)) * 64 + (row & 63)) * 16 + ch * 4);
    }
  };
  auto store_w = [&](char* stage, const f32x4 (&w)[WCH]) {
#pragma unroll
    for (int j = 0; j < WCH; ++j) {
      const int i = tid + 256 * j, s = i / (BN * 4), rc = i - s * (BN * 4), row = rc >> 2, ch = rc & 3;
      *reinterpret_cast<f32x4*>(stage + s * SUB + A_BYTES + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4)) = w[j];
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int nst = p.KT >> 1;
  f32x4 av[2][2], wv[WCH];
  load_a(0, av[0]);
  load_a(1, av[1]);
  load_w(0, wv);
  store_a(conv_lds, av[0]);
  store_a(conv_lds + SUB, av[1]);
  store_w(conv_lds, wv);
  __syncthreads();

  const int sw = (n0 >> 2) & 3;
  const int a_off = (32 * wave + n0) * 64, chi = (hb ^ sw) << 4, clo = ((2 + hb) ^ sw) << 4;
  for (int st = 0; st < nst; ++st) {
    const bool more = st + 1 < nst;
    if (more) {  // the next stage's loads fly while this one multiplies
      load_a(2 * st + 2, av[0]);
      load_a(2 * st + 3, av[1]);
      load_w(st + 1, wv);
    }
    const char* cur = conv_lds + (st & 1) * STAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const char* sub = cur + s * SUB;
      const f16x8 ahi = *reinterpret_cast<const f16x8*>(sub + a_off + chi);
      const f16x8 alo = *reinterpret_cast<const f16x8*>(sub + a_off + clo);
      f16x8 whi[NT], wlo[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const char* wr = sub + A_BYTES + (32 * j + n0) * 64;
        whi[j] = *reinterpret_cast<const f16x8*>(wr + chi);
        wlo[j] = *reinterpret_cast<const f16x8*>(wr + clo);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, whi[j], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, wlo[j], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const f16x8 wh2 = whi[j] * (_Float16)0.00048828125f;  // 2^-11: undoes the scale of alo
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, wh2, acc[j], 0, 0, 0);
      }
    }
    if (more) {  // the other stage was last read before the barrier that ended the previous trip
      char* nxt = conv_lds + ((st + 1) & 1) * STAGE;
      store_a(nxt, av[0]);
      store_a(nxt + SUB, av[1]);
      store_w(nxt, wv);
    }
    __syncthreads();
  }

  // ---- epilogue: register r of lane (n0, hb) is pixel 4 hb + (r & 3) + 8 (r >> 2) of the wave's 32, channel 32 j + n0 ----
  bool bad = false;
  const int m_lane = m_base + 32 * wave + 4 * hb;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n_base + 32 * j + n0;
    if (n < p.N) {
      const float w_down = p.wscale[n], b = p.bias ? p.bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m_lane + (r & 3) + 8 * (r >> 2);
        if (m < p.M) {
          float v = acc[j][r] * w_down;  // a power of two: exact
          v = v + b;
          const float res = p.R ? p.R[(size_t)m * p.ldr + n] : 0.f;
          if (p.R && !p.res_after) v = v + res;
          if (p.act == CONV_ACT_RELU) v = v < 0.f ? 0.f : v;  // (NaN stays NaN)
          if (p.act == CONV_ACT_LEAKY) v = v < 0.f ? v * p.slope : v;
          if (p.R && p.res_after) v = v + res;
          bad = bad || nonfinite(v);
          p.out[(size_t)m * p.ldo + n] = v;
        }
      }
    }
  }
  report_nonfinite(p.oflow, bad);
}

// One wave per packed row (the rows past Cout of the last block of 64 are zeros); k = (ky, kx, cin) from OIHW.
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ Wt, int Cout, int Cin, int KH, int KW, int Kp,
                                                        _Float16* __restrict__ Wp, float* __restrict__ wscale) {
  const int lane = threadIdx.x & 63;
  const int K = KH * KW * Cin, rows = ((Cout + 63) >> 6) << 6, taps = KH * KW;
  for (int n = blockIdx.x * 4 + (threadIdx.x >> 6); n < rows; n += gridDim.x * 4) {
    const float* __restrict__ row = Wt + (size_t)min(n, Cout - 1) * K;  // OIHW: [cin][ky][kx] inside a row
    float m = 0.f;
    if (n < Cout)
      for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(row[k]));
    m = wave_max(m);
    int e = 0;
    if (m > 0.f && m < 3.0e38f) frexpf(m, &e);  // m = f * 2^e, f in [0.5, 1)
    e = max(-110, min(e, 125));
    const float up = m > 0.f ? ldexpf(1.f, 15 - e) : 1.f, down = m > 0.f ? ldexpf(1.f, e - 15) : 1.f;
    if (lane == 0 && n < Cout) wscale[n] = down;
    _Float16* __restrict__ out = Wp + ((size_t)(n >> 6) * (Kp / 16) * 64 + (n & 63)) * 32;
    for (int k = lane; k < Kp; k += 64) {
      float ws = 0.f;
      if (n < Cout && k < K) {
        const int tap = k / Cin, c = k - tap * Cin;
        ws = row[(size_t)c * taps + tap] * up;
      }
      const _Float16 hi = (_Float16)ws;
      const _Float16 lo = (_Float16)(ws - (float)hi);
      out[(size_t)(k / 16) * (64 * 32) + (k % 16)] = hi;
      out[(size_t)(k / 16) * (64 * 32) + 16 + (k % 16)] = lo;
    }
  }
}

// 3 x 3 window, stride 2, pad 1 on NHWC fp32; a thread takes four channels of one output pixel.  The padding never wins (the window
// starts from -inf); a NaN in the window is the result, as nn.MaxPool2d gives it.
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int H, int W, int C,
                                                           int OH, int OW) {
  const int c4 = C >> 2;
  const long long total = (long long)n * OH * OW * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % c4);
    long long t = i / c4;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH), img = (int)(t / OH);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if ((unsigned)iy >= (unsigned)H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if ((unsigned)ix >= (unsigned)W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (((long long)img * H + iy) * W + ix) * C + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v[e] > m[e] || v[e] != v[e]) m[e] = v[e];
      }
    }
    *reinterpret_cast<f32x4*>(y + (((long long)img * OH + oy) * OW + ox) * C + 4 * c) = m;
  }
}

// Mean over the HW pixels of an NHWC image, per channel: one thread per (image, channel), the pixels in their order into ONE fp64 sum
// (no partial sums to combine: the same bits whatever n), rounded to fp32 once.
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int HW, int C) {
  const long long total = (long long)n * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long long img = i / C;
    const float* __restrict__ px = x + img * HW * C + c;
    double s = 0.0;
    for (int k = 0; k < HW; ++k) s += (double)px[(long long)k * C];
    y[i] = (float)(s / (double)HW);
  }
}

template <int NT, bool FAST>
int launch_conv(const ConvParams& p, hipStream_t stream) {
  constexpr int LDS = 2 * 2 * (CONV_BM * 64 + 32 * NT * 64);  // 48 KB: within the default limit
  const long long grid = (long long)((p.M + CONV_BM - 1) / CONV_BM) * p.ntn;
  hipLaunchKernelGGL((conv_split_kernel<NT, FAST>), dim3((unsigned)grid), dim3(256), LDS, stream, p);
  return pmce_check_launch("conv2d_split_f16");
}

}  // namespace

extern "C" long long pmce_conv_packed_floats(int Cout, int Cin, int KH, int KW) {
  if (Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || (long long)Cin * KH * KW > (1 << 24)) {
    pmce_set_error("conv_packed_floats: need Cout, Cin, KH, KW >= 1 and Cin KH KW <= 2^24 (got %d %d %d %d)", Cout, Cin, KH, KW);
    return 0;
  }
  const long long Kp = ((long long)Cin * KH * KW + 31) / 32 * 32;
  return (long long)((Cout + 63) / 64) * 64 * Kp;
}

extern "C" int pmce_conv_pack_split_f16(const float* W_oihw, int Cout, int Cin, int KH, int KW, float* Wp, float* wscale, hipStream_t stream) {
  PMCE_REQUIRE(W_oihw && Wp && wscale, "conv_pack_split_f16: null pointer");
  PMCE_REQUIRE(pmce_conv_packed_floats(Cout, Cin, KH, KW) > 0, "conv_pack_split_f16: bad shape (Cout=%d Cin=%d KH=%d KW=%d)", Cout, Cin, KH, KW);
  const int Kp = (Cin * KH * KW + 31) / 32 * 32, rows = (Cout + 63) / 64 * 64;
  const int blocks = rows / 4 < 4096 ? rows / 4 : 4096;
  hipLaunchKernelGGL(conv_pack_kernel, dim3(blocks), dim3(256), 0, stream, W_oihw, Cout, Cin, KH, KW, Kp, reinterpret_cast<_Float16*>(Wp), wscale);
  return pmce_check_launch("conv_pack_split_f16");
}

namespace {

// The one launcher behind both entries.
int conv2d_launch(const float* x, long long sn, long long sc, long long sy, long long sx, int n, int Cin, int H, int W, const float* Wp,
                  const float* wscale, const float* bias, const float* R, long long ldr, float* out, long long ldo, int Cout, int KH, int KW,
                  int stride, int pad, int act, float slope, int res_after, hipStream_t stream) {
  PMCE_REQUIRE(x && Wp && wscale && out, "conv2d_split_f16: null pointer");
  PMCE_REQUIRE(n >= 1 && Cin >= 1 && H >= 1 && W >= 1 && Cout >= 1 && KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0 && pad < KH && pad < KW,
               "conv2d_split_f16: need n, Cin, H, W, Cout, KH, KW, stride >= 1 and 0 <= pad < KH, KW (n=%d Cin=%d H=%d W=%d Cout=%d KH=%d KW=%d "
               "stride=%d pad=%d)", n, Cin, H, W, Cout, KH, KW, stride, pad);
  PMCE_REQUIRE(H + 2 * pad >= KH && W + 2 * pad >= KW, "conv2d_split_f16: the window (%d x %d) exceeds the padded input (%d x %d, pad %d)", KH, KW, H, W, pad);
  PMCE_REQUIRE(pmce_conv_packed_floats(Cout, Cin, KH, KW) > 0, "conv2d_split_f16: bad weight shape");
  PMCE_REQUIRE(sn >= 0 && sc >= 1 && sy >= 1 && sx >= 1, "conv2d_split_f16: strides must be positive");
  const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
  const long long M = (long long)n * OH * OW;
  // the largest element offset a load can form, and the output's extent, stay inside 2^40 elements; row indices are ints
  PMCE_REQUIRE(M < (1ll << 30) && (n - 1) * sn + (Cin - 1) * sc + (H - 1) * sy + (W - 1) * sx < (1ll << 40),
               "conv2d_split_f16: the problem is too large (M = %lld rows; split the batch)", M);
  PMCE_REQUIRE(ldo >= Cout && ldo < (1ll << 24) && (!R || (ldr >= Cout && ldr < (1ll << 24))),
               "conv2d_split_f16: the row pitches must be in Cout..2^24 (Cout=%d out pitch=%lld residual pitch=%lld)", Cout, ldo, ldr);
  ConvParams p{};
  p.X = x; p.sn = sn; p.sc = sc; p.sy = sy; p.sx = sx;
  p.H = H; p.W = W; p.Cin = Cin; p.OH = OH; p.OW = OW; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
  p.Wp = Wp; p.wscale = wscale; p.bias = bias; p.R = R; p.out = out; p.ldo = ldo; p.ldr = R ? ldr : 0;
  p.M = (int)M; p.N = Cout; p.K = Cin * KH * KW; p.KT = (p.K + 31) / 32 * 2;
  p.act = act; p.slope = slope; p.res_after = res_after;
  p.oflow = pmce_overflow_sink();
  const bool fast = sc == 1 && Cin % 16 == 0 && sn % 4 == 0 && sy % 4 == 0 && sx % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  p.ntn = (Cout + 63) / 64;  // one tile shape for every layer and every batch
  PMCE_REQUIRE((long long)((M + CONV_BM - 1) / CONV_BM) * p.ntn < (1ll << 31), "conv2d_split_f16: too many tiles");
  return fast ? launch_conv<2, true>(p, stream) : launch_conv<2, false>(p, stream);
}

}  // namespace

extern "C" int pmce_conv2d_split_f16(const float* x, long long sn, long long sc, long long sy, long long sx, int n, int Cin, int H, int W,
                                     const float* Wp, const float* wscale, const float* bias, const float* R, float* out, int Cout, int KH,
                                     int KW, int stride, int pad, int relu, hipStream_t stream) {
  return conv2d_launch(x, sn, sc, sy, sx, n, Cin, H, W, Wp, wscale, bias, R, Cout, out, Cout, Cout, KH, KW, stride, pad,
                       relu ? CONV_ACT_RELU : CONV_ACT_NONE, 0.f, 0, stream);
}

extern "C" int pmce_conv2d_act_split_f16(const float* x, long long sn, long long sc, long long sy, long long sx, int n, int Cin, int H, int W,
                                         const float* Wp, const float* wscale, const float* bias, const float* R, long long res_pitch,
                                         float* out, long long out_pitch, int Cout, int KH, int KW, int stride, int pad, int act, float slope,
                                         int res_after_act, hipStream_t stream) {
  PMCE_REQUIRE(act == CONV_ACT_NONE || act == CONV_ACT_RELU || act == CONV_ACT_LEAKY,
               "conv2d_act_split_f16: act must be 0 (none), 1 (ReLU) or 2 (leaky) (got %d)", act);
  PMCE_REQUIRE(act != CONV_ACT_LEAKY || (slope == slope && slope >= 0.f && slope <= 1.f),
               "conv2d_act_split_f16: the leaky slope must be in [0, 1] (got %g)", (double)slope);
  PMCE_REQUIRE(res_after_act == 0 || res_after_act == 1, "conv2d_act_split_f16: res_after_act must be 0 or 1 (got %d)", res_after_act);
  return conv2d_launch(x, sn, sc, sy, sx, n, Cin, H, W, Wp, wscale, bias, R, res_pitch, out, out_pitch, Cout, KH, KW, stride, pad, act,
                       act == CONV_ACT_LEAKY ? slope : 0.f, res_after_act, stream);
}

extern "C" int pmce_maxpool3x3s2_nhwc_f32(const float* x, float* y, int n, int H, int W, int C, hipStream_t stream) {
  PMCE_REQUIRE(x && y, "maxpool3x3s2: null pointer");
  PMCE_REQUIRE(n >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "maxpool3x3s2: need n, H, W >= 1 and C %% 4 == 0 (n=%d H=%d W=%d C=%d)", n, H, W, C);
  PMCE_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0, "maxpool3x3s2: buffers must be 16-byte aligned");
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const long long total = (long long)n * OH * OW * (C / 4);
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, x, y, n, H, W, C, OH, OW);
  return pmce_check_launch("maxpool3x3s2_nhwc_f32");
}

extern "C" int pmce_avgpool_nhwc_f32(const float* x, float* y, int n, int HW, int C, hipStream_t stream) {
  PMCE_REQUIRE(x && y, "avgpool: null pointer");
  PMCE_REQUIRE(n >= 1 && HW >= 1 && C >= 1, "avgpool: need n, HW, C >= 1 (n=%d HW=%d C=%d)", n, HW, C);
  const long long blocks = ((long long)n * C + 255) / 256;
  hipLaunchKernelGGL(avgpool_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, x, y, n, HW, C);
  return pmce_check_launch("avgpool_nhwc_f32");
}

// The single-product f16 mode: the same operators on f16 maps, ONE matrix product per k-tile (kernel, layouts and entries there).
#include "conv_f16.hpp"
