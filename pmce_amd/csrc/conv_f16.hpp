// The single-product f16 convolution (FeatureExtractor / YOLOv3 with precision="f16") and its small f16 companions: the 3 x 3 / 2 max
// pool, the global average, the nearest x2 upsample and the exact widening f16 -> fp32.  Included by conv.hip at its end: the two
// convolutions share one translation unit, one set of activation codes and the device-code census of the test suite.
//
//     out[m][n] = R16?( epilogue( 2^-s(n) * sum_k a16[m][k] * w16[n][k] + bias[n], R[m][n] ) )       m = (image, oy, ox), n = Cout, k = (ky, kx, cin)
//
// on v_mfma_f32_32x32x16_f16 with fp32 accumulation and ONE product per k-tile (conv.hip's kernel issues three and splits every
// activation into two planes on the way into LDS; this one does neither).
// Weights: packed ONCE (pmce_conv_pack_f16) from BatchNorm-folded fp32 OIHW weights into the blocked layout
//     [ceil(Cout / 64)][Kp / 32][64 rows][32 f16]        of r16(W[n] * 2^s(n)),
// k in the order (ky, kx, cin), K = KH KW Cin padded with zero weights to Kp = a multiple of 64 (one stage), the rows past Cout written
// as zeros; wscale[n] = 2^-s(n) lifts a row's largest |w| into [2^14, 2^15) exactly as pmce_conv_pack_split_f16 does.  A (block,
// k-tile) piece is 64 rows x 64 bytes = 4 KB, contiguous.
// Activations, two forms: f16 addressed by four element strides in halves (NHWC between layers: channel stride 1, the row pitch may be
// that of a wider buffer), taken as they are; or fp32 through four element strides (the stems: NCHW patches, letterboxed images), each
// value rounded by r16 (common.hpp: nearest even, |x| < 2^-14 -> 0, beyond the range -> inf) in the gather.  The zero padding is a
// predicate of the load.
// Tile: 128 output pixels x 64 output channels per workgroup of four waves, a wave owns 32 pixels x 64 channels.  A k-tile is 32 halves:
// the same 64-byte LDS row image and XOR swizzle as conv.hip's (16-byte chunk c of a row at physical chunk c ^ ((row >> 2) & 3)), chunk c
// = k 8 c .. 8 c + 7, and two matrix instructions per k-tile and column sub-tile (instruction u reads chunk 2 u + hb).  A stage is two
// k-tiles (K = 64); two stages in LDS (48 KB, as conv.hip's, for twice the K); the next stage's global loads are in flight in registers
// while the matrix instructions of the current one run; one barrier per stage.
//   FAST (f16, channel stride 1, Cin % 32 == 0, base and the other strides 16-byte aligned): a k-tile lies inside one tap and is 64
//        contiguous bytes per pixel: one 16-byte load per thread and row, the tap arithmetic is scalar.
//   generic (the stems; Cin % 32 != 0; a base or pitch that is not 16-byte aligned): every element is its own predicated load.
//   Both stage the same LDS image: the same bits for the same problem.
// Epilogue: conv.hip's - v = 2^-s(n) acc + bias[n]; then act(v + R) or act(v) + R - with an f16 residual of its own pitch, every step a
// separate fp32 rounding (contraction is off: the f16-output instantiation must round the very value the fp32-output one stores).  The
// result is fp32 (pitch in floats) or r16 of it (pitch in halves); a result that is not finite - a finite fp32 beyond f16's range
// included, where it is written as f16 - is reported to pmce_overflow_sink().  An f16 result whose column tile is whole and whose rows
// (and the residual's) are 16-byte aligned leaves through LDS: a lane owns one column for 16 rows, which as f16 is 2-byte stores of 64
// contiguous bytes per row, and the 56 x 56 layers are bound by exactly that traffic; the wave turns its patch round in the tile's LDS
// (free after the k-loop) and stores 16 bytes per lane, 128 contiguous bytes per row, reading the residual the same way.  Measured on
// the extractor's 2400 patches: 130 against 155 ms (layer1's conv3 0.078 against 0.138 ms per batch of 64); DESIGN.md 8.  Any other
// result (fp32, Cout % 64 != 0, an unaligned slice) takes the direct stores - to the same bits.
// Order of summation: an output element is ONE accumulator register that takes the k-tiles 0, 1, 2, ... in turn, two matrix
// instructions each in a fixed order, whatever the batch, the tile it falls into or its place in the tile: bit-identical whatever n is.
#pragma once

namespace {

struct ConvF16Params {
  const void* X;             // f16 or fp32 (the kernel's template argument)
  long long sn, sc, sy, sx;  // element strides of the input: image, channel, row, column
  int H, W, Cin, OH, OW, KH, KW, stride, pad;
  const _Float16* Wp;    // packed weights (see above)
  const float* wscale;   // [Cout] 2^-s(n)
  const float* bias;     // [Cout] or null
  const _Float16* R;     // residual, row m at R + m ldr, or null
  void* out;             // row m at out + m ldo, f16 or fp32 (the kernel's template argument)
  long long ldo, ldr;    // row pitches in elements (>= Cout)
  int M, N, K, KT;       // M = n OH OW, N = Cout, K = KH KW Cin, KT = Kp / 32
  int ntn;               // column tiles
  int act;               // CONV_ACT_NONE / _RELU / _LEAKY
  float slope;
  int res_after;         // 0: act(v + R); 1: act(v) + R
  int vec16;             // f16 result whose rows (and the residual's) take 16-byte accesses: the epilogue goes through LDS (see the kernel)
  unsigned* oflow;
};

constexpr int GATHER_FAST = 0, GATHER_F16 = 1, GATHER_F32 = 2;
constexpr int CONV16_NT = 2;  // column sub-tiles of 32 per wave: the 64-wide tile, the only one built (a 128-wide one was not measured: DESIGN.md 8)

template <int G, bool OUT16>
__global__ __launch_bounds__(256) void conv_f16_kernel(ConvF16Params p) {
#pragma clang fp contract(off)
  constexpr int NT = CONV16_NT, BN = 32 * NT;
  constexpr int A_BYTES = CONV_BM * 64, SUB = A_BYTES + BN * 64, STAGE = 2 * SUB;  // one k-tile: [A rows of 64 B | W rows of 64 B]
  constexpr int WCH = NT;  // 16-byte weight chunks per thread and stage: 2 * BN * 4 / 256
  extern __shared__ __attribute__((aligned(16))) char conv16_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = lane & 31, hb = lane >> 5;
  const int tn = blockIdx.x % p.ntn, tm = blockIdx.x / p.ntn;
  const int m_base = tm * CONV_BM, n_base = tn * BN;

  // ---- gather side: thread (r = tid / 4, q = tid % 4) stages halves 8 q .. 8 q + 7 of the k-tile for the rows r and r + 64 ----
  const int gr = tid >> 2, gq = tid & 3;
  long long goff[2];
  int iy0[2], ix0[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int m = m_base + gr + 64 * u;
    const int mc = min(m, p.M - 1);
    const int img = mc / (p.OH * p.OW), rem = mc - img * (p.OH * p.OW);
    const int oy = rem / p.OW, ox = rem - oy * p.OW;
    goff[u] = (long long)img * p.sn;
    iy0[u] = m < p.M ? oy * p.stride - p.pad : -(1 << 20);  // a row past M fails every bounds test: it stages zeros
    ix0[u] = ox * p.stride - p.pad;
  }
  auto load_a = [&](int kt, f16x8 (&v)[2]) {
    const int k0 = kt * 32;
    if constexpr (G == GATHER_FAST) {
      const int tap = k0 / p.Cin, c0 = k0 - tap * p.Cin, ky = tap / p.KW, kx = tap - ky * p.KW;  // wave-uniform
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int iy = iy0[u] + ky, ix = ix0[u] + kx;
        const bool ok = k0 < p.K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[u][e] = (_Float16)0.0f;
        if (ok)
          v[u] = *reinterpret_cast<const f16x8*>(static_cast<const _Float16*>(p.X) + goff[u] + (long long)iy * p.sy + (long long)ix * p.sx +
                                                 (c0 + 8 * gq));
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = k0 + 8 * gq + e;
        const int tap = k / p.Cin, c = k - tap * p.Cin, ky = tap / p.KW, kx = tap - ky * p.KW;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int iy = iy0[u] + ky, ix = ix0[u] + kx;
          const bool ok = k < p.K && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
          const long long off = goff[u] + (long long)iy * p.sy + (long long)ix * p.sx + (long long)c * p.sc;
          _Float16 x = (_Float16)0.0f;
          if constexpr (G == GATHER_F16) {
            if (ok) x = static_cast<const _Float16*>(p.X)[off];
          } else {
            if (ok) x = r16(static_cast<const float*>(p.X)[off]);
          }
          v[u][e] = x;
        }
      }
    }
  };
  // LDS image of a k-tile row: four 16-byte chunks {k 0-7, 8-15, 16-23, 24-31}, chunk c at physical chunk c ^ ((row >> 2) & 3)
  auto store_a = [&](char* sub, const f16x8 (&v)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = gr + 64 * u, sw = (row >> 2) & 3;
      *reinterpret_cast<f16x8*>(sub + row * 64 + ((gq ^ sw) << 4)) = v[u];
    }
  };
  // weights: chunk i = tid + 256 j of the stage's 2 * BN * 4 chunks -> (k-tile s, row, chunk ch)
  const int nblocks = (p.N + 63) >> 6;
  auto load_w = [&](int st, f16x8 (&w)[WCH]) {
#pragma unroll
    for (int j = 0; j < WCH; ++j) {
      const int i = tid + 256 * j, s = i / (BN * 4), rc = i - s * (BN * 4), row = rc >> 2, ch = rc & 3;
      const int nb = (n_base + row) >> 6;
#pragma unroll
      for (int e = 0; e < 8; ++e) w[j][e] = (_Float16)0.0f;
      if (nb < nblocks)
        w[j] = *reinterpret_cast<const f16x8*>(p.Wp + (((size_t)nb * p.KT + (2 * st + s)) * 64 + ((n_base + row) & 63)) * 32 + ch * 8);
    }
  };
  auto store_w = [&](char* stage, const f16x8 (&w)[WCH]) {
#pragma unroll
    for (int j = 0; j < WCH; ++j) {
      const int i = tid + 256 * j, s = i / (BN * 4), rc = i - s * (BN * 4), row = rc >> 2, ch = rc & 3;
      *reinterpret_cast<f16x8*>(stage + s * SUB + A_BYTES + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4)) = w[j];
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int nst = p.KT >> 1;
  f16x8 av[2][2], wv[WCH];
  load_a(0, av[0]);
  load_a(1, av[1]);
  load_w(0, wv);
  store_a(conv16_lds, av[0]);
  store_a(conv16_lds + SUB, av[1]);
  store_w(conv16_lds, wv);
  __syncthreads();

  const int sw = (n0 >> 2) & 3;
  const int a_off = (32 * wave + n0) * 64;
  for (int st = 0; st < nst; ++st) {
    const bool more = st + 1 < nst;
    if (more) {  // the next stage's loads fly while this one multiplies
      load_a(2 * st + 2, av[0]);
      load_a(2 * st + 3, av[1]);
      load_w(st + 1, wv);
    }
    const char* cur = conv16_lds + (st & 1) * STAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const char* sub = cur + s * SUB;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int ch = ((2 * u + hb) ^ sw) << 4;
        const f16x8 a = *reinterpret_cast<const f16x8*>(sub + a_off + ch);
        f16x8 w[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) w[j] = *reinterpret_cast<const f16x8*>(sub + A_BYTES + (32 * j + n0) * 64 + ch);
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, w[j], acc[j], 0, 0, 0);
      }
    }
    if (more) {  // the other stage was last read before the barrier that ended the previous trip
      char* nxt = conv16_lds + ((st + 1) & 1) * STAGE;
      store_a(nxt, av[0]);
      store_a(nxt + SUB, av[1]);
      store_w(nxt, wv);
    }
    __syncthreads();
  }

  // ---- epilogue: register r of lane (n0, hb) is pixel 4 hb + (r & 3) + 8 (r >> 2) of the wave's 32, channel 32 j + n0 ----
  bool bad = false;
  const int m_lane = m_base + 32 * wave + 4 * hb;
  if constexpr (OUT16) {
    if (p.vec16) {
      // A lane owns ONE column for 16 rows: written from the registers an f16 row would go out as 2-byte stores, 64 contiguous bytes per
      // row and instruction.  After the k-loop the tile's LDS is free, so the wave turns its 32 x BN patch round in it: v = 2^-s acc +
      // bias goes in as fp32 (the same fp32 value the direct form continues with), and comes out eight channels of a row per lane -
      // 16-byte residual loads, 16-byte stores, 128 contiguous bytes per row.  The same operations on every element: the same bits.
      constexpr int LDT = BN + 4;  // floats per patch row: 16-byte aligned rows a bank apart
      float* patch = reinterpret_cast<float*>(conv16_lds) + wave * (32 * LDT);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = n_base + 32 * j + n0;
        const float w_down = p.wscale[n], b = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[j][r] * w_down;  // a power of two: exact
          v = v + b;
          patch[(4 * hb + (r & 3) + 8 * (r >> 2)) * LDT + 32 * j + n0] = v;
        }
      }
      __syncthreads();
      _Float16* out16 = static_cast<_Float16*>(p.out);
#pragma unroll
      for (int i = 0; i < BN / 16; ++i) {
        const int c = lane + 64 * i, row = c / (BN / 8), c8 = c - row * (BN / 8);
        const int m = m_base + 32 * wave + row;
        if (m < p.M) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(patch + row * LDT + 8 * c8);
          const f32x4 v1 = *reinterpret_cast<const f32x4*>(patch + row * LDT + 8 * c8 + 4);
          f16x8 res;
#pragma unroll
          for (int e = 0; e < 8; ++e) res[e] = (_Float16)0.0f;
          if (p.R) res = *reinterpret_cast<const f16x8*>(p.R + (size_t)m * p.ldr + n_base + 8 * c8);
          f16x8 h;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float v = e < 4 ? v0[e & 3] : v1[e & 3];
            const float rs = (float)res[e];
            if (p.R && !p.res_after) v = v + rs;
            if (p.act == CONV_ACT_RELU) v = v < 0.f ? 0.f : v;
            if (p.act == CONV_ACT_LEAKY) v = v < 0.f ? v * p.slope : v;
            if (p.R && p.res_after) v = v + rs;
            h[e] = r16(pinned(v));
            bad = bad || __builtin_amdgcn_classh(h[e], 0x207);
          }
          *reinterpret_cast<f16x8*>(out16 + (size_t)m * p.ldo + n_base + 8 * c8) = h;
        }
      }
      report_nonfinite(p.oflow, bad);
      return;
    }
  }
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
          const float res = p.R ? (float)p.R[(size_t)m * p.ldr + n] : 0.f;
          if (p.R && !p.res_after) v = v + res;
          if (p.act == CONV_ACT_RELU) v = v < 0.f ? 0.f : v;  // (NaN stays NaN)
          if (p.act == CONV_ACT_LEAKY) v = v < 0.f ? v * p.slope : v;
          if (p.R && p.res_after) v = v + res;
          if constexpr (OUT16) {
            const _Float16 h = r16(pinned(v));
            bad = bad || __builtin_amdgcn_classh(h, 0x207);  // inf / NaN: also a finite v beyond f16's 65504
            static_cast<_Float16*>(p.out)[(size_t)m * p.ldo + n] = h;
          } else {
            bad = bad || nonfinite(v);
            static_cast<float*>(p.out)[(size_t)m * p.ldo + n] = v;
          }
        }
      }
    }
  }
  report_nonfinite(p.oflow, bad);
}

// One wave per packed row (the rows past Cout of the last block of 64 are zeros); k = (ky, kx, cin) from OIHW.
__global__ __launch_bounds__(256) void conv_pack_f16_kernel(const float* __restrict__ Wt, int Cout, int Cin, int KH, int KW, int Kp,
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
    _Float16* __restrict__ out = Wp + ((size_t)(n >> 6) * (Kp / 32) * 64 + (n & 63)) * 32;
    for (int k = lane; k < Kp; k += 64) {
      float ws = 0.f;
      if (n < Cout && k < K) {
        const int tap = k / Cin, c = k - tap * Cin;
        ws = row[(size_t)c * taps + tap] * up;
      }
      out[(size_t)(k / 32) * (64 * 32) + (k % 32)] = r16(ws);
    }
  }
}

// The f16 forms of conv.hip's max pool (a thread takes four channels of one output pixel: 8 bytes; exact, a NaN in the window wins) and
// average (the pixels in their order into ONE fp64 sum, rounded to fp32 once), and of yolo.hip's nearest x2 upsample (pitches in halves).
__global__ __launch_bounds__(256) void maxpool3x3s2_f16_kernel(const _Float16* __restrict__ x, _Float16* __restrict__ y, int n, int H, int W,
                                                               int C, int OH, int OW) {
  const int c4 = C >> 2;
  const long long total = (long long)n * OH * OW * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % c4);
    long long t = i / c4;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH), img = (int)(t / OH);
    const _Float16 ninf = (_Float16)(-INFINITY);
    f16x4 m = {ninf, ninf, ninf, ninf};
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = 2 * oy - 1 + ky;
      if ((unsigned)iy >= (unsigned)H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = 2 * ox - 1 + kx;
        if ((unsigned)ix >= (unsigned)W) continue;
        const f16x4 v = *reinterpret_cast<const f16x4*>(x + (((long long)img * H + iy) * W + ix) * C + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v[e] > m[e] || v[e] != v[e]) m[e] = v[e];
      }
    }
    *reinterpret_cast<f16x4*>(y + (((long long)img * OH + oy) * OW + ox) * C + 4 * c) = m;
  }
}

__global__ __launch_bounds__(256) void avgpool_f16_kernel(const _Float16* __restrict__ x, float* __restrict__ y, int n, int HW, int C) {
  const long long total = (long long)n * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long long img = i / C;
    const _Float16* __restrict__ px = x + img * HW * C + c;
    double s = 0.0;
    for (int k = 0; k < HW; ++k) s += (double)(float)px[(long long)k * C];
    y[i] = (float)(s / (double)HW);
  }
}

__global__ __launch_bounds__(256) void upsample2x_f16_kernel(const _Float16* __restrict__ x, long long ldx, _Float16* __restrict__ out,
                                                             long long ldo, int n, int H, int W, int C) {
  const int c4 = C >> 2, OW = 2 * W, OH = 2 * H;
  const long long total = (long long)n * OH * OW * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % c4);
    long long t = i / c4;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    const long long img = t / OH;
    const f16x4 v = *reinterpret_cast<const f16x4*>(x + ((img * H + (oy >> 1)) * W + (ox >> 1)) * ldx + 4 * c);
    *reinterpret_cast<f16x4*>(out + ((img * OH + oy) * OW + ox) * ldo + 4 * c) = v;
  }
}

__global__ __launch_bounds__(256) void widen_f16_kernel(const _Float16* __restrict__ x, float* __restrict__ y, long long count) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) y[i] = (float)x[i];
}

unsigned f16_grid_for(long long total) {
  const long long blocks = (total + 255) / 256;
  return (unsigned)(blocks < 65536 ? (blocks < 1 ? 1 : blocks) : 65536);
}

template <int G, bool OUT16>
int launch_conv_f16(const ConvF16Params& p, hipStream_t stream) {
  constexpr int LDS = 2 * 2 * (CONV_BM * 64 + 32 * CONV16_NT * 64);  // 48 KB: within the default limit
  const long long grid = (long long)((p.M + CONV_BM - 1) / CONV_BM) * p.ntn;
  hipLaunchKernelGGL((conv_f16_kernel<G, OUT16>), dim3((unsigned)grid), dim3(256), LDS, stream, p);
  return pmce_check_launch("conv2d_act_f16");
}

constexpr int CONV_DTYPE_F32 = 0, CONV_DTYPE_F16 = 1;

}  // namespace

extern "C" long long pmce_conv_packed_halves(int Cout, int Cin, int KH, int KW) {
  if (Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || (long long)Cin * KH * KW > (1 << 24)) {
    pmce_set_error("conv_packed_halves: need Cout, Cin, KH, KW >= 1 and Cin KH KW <= 2^24 (got %d %d %d %d)", Cout, Cin, KH, KW);
    return 0;
  }
  const long long Kp = ((long long)Cin * KH * KW + 63) / 64 * 64;
  return (long long)((Cout + 63) / 64) * 64 * Kp;
}

extern "C" int pmce_conv_pack_f16(const float* W_oihw, int Cout, int Cin, int KH, int KW, void* Wp, float* wscale, hipStream_t stream) {
  PMCE_REQUIRE(W_oihw && Wp && wscale, "conv_pack_f16: null pointer");
  PMCE_REQUIRE(pmce_conv_packed_halves(Cout, Cin, KH, KW) > 0, "conv_pack_f16: bad shape (Cout=%d Cin=%d KH=%d KW=%d)", Cout, Cin, KH, KW);
  const int Kp = (Cin * KH * KW + 63) / 64 * 64, rows = (Cout + 63) / 64 * 64;
  const int blocks = rows / 4 < 4096 ? rows / 4 : 4096;
  hipLaunchKernelGGL(conv_pack_f16_kernel, dim3(blocks), dim3(256), 0, stream, W_oihw, Cout, Cin, KH, KW, Kp, static_cast<_Float16*>(Wp), wscale);
  return pmce_check_launch("conv_pack_f16");
}

extern "C" int pmce_conv2d_act_f16(const void* x, int x_dtype, long long sn, long long sc, long long sy, long long sx, int n, int Cin, int H,
                                   int W, const void* Wp, const float* wscale, const float* bias, const void* R, long long res_pitch, void* out,
                                   long long out_pitch, int out_dtype, int Cout, int KH, int KW, int stride, int pad, int act, float slope,
                                   int res_after_act, hipStream_t stream) {
  PMCE_REQUIRE(x && Wp && wscale && out, "conv2d_act_f16: null pointer");
  PMCE_REQUIRE((x_dtype == CONV_DTYPE_F32 || x_dtype == CONV_DTYPE_F16) && (out_dtype == CONV_DTYPE_F32 || out_dtype == CONV_DTYPE_F16),
               "conv2d_act_f16: the dtype codes must be 0 (fp32) or 1 (f16) (got input %d, output %d)", x_dtype, out_dtype);
  PMCE_REQUIRE(act == CONV_ACT_NONE || act == CONV_ACT_RELU || act == CONV_ACT_LEAKY,
               "conv2d_act_f16: act must be 0 (none), 1 (ReLU) or 2 (leaky) (got %d)", act);
  PMCE_REQUIRE(act != CONV_ACT_LEAKY || (slope == slope && slope >= 0.f && slope <= 1.f),
               "conv2d_act_f16: the leaky slope must be in [0, 1] (got %g)", (double)slope);
  PMCE_REQUIRE(res_after_act == 0 || res_after_act == 1, "conv2d_act_f16: res_after_act must be 0 or 1 (got %d)", res_after_act);
  PMCE_REQUIRE(n >= 1 && Cin >= 1 && H >= 1 && W >= 1 && Cout >= 1 && KH >= 1 && KW >= 1 && stride >= 1 && pad >= 0 && pad < KH && pad < KW,
               "conv2d_act_f16: need n, Cin, H, W, Cout, KH, KW, stride >= 1 and 0 <= pad < KH, KW (n=%d Cin=%d H=%d W=%d Cout=%d KH=%d KW=%d "
               "stride=%d pad=%d)", n, Cin, H, W, Cout, KH, KW, stride, pad);
  PMCE_REQUIRE(H + 2 * pad >= KH && W + 2 * pad >= KW, "conv2d_act_f16: the window (%d x %d) exceeds the padded input (%d x %d, pad %d)", KH, KW, H, W, pad);
  PMCE_REQUIRE(pmce_conv_packed_halves(Cout, Cin, KH, KW) > 0, "conv2d_act_f16: bad weight shape");
  PMCE_REQUIRE(sn >= 0 && sc >= 1 && sy >= 1 && sx >= 1, "conv2d_act_f16: strides must be positive");
  const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
  const long long M = (long long)n * OH * OW;
  // the largest element offset a load can form, and the output's extent, stay inside 2^40 elements; row indices are ints
  PMCE_REQUIRE(M < (1ll << 30) && (n - 1) * sn + (Cin - 1) * sc + (H - 1) * sy + (W - 1) * sx < (1ll << 40),
               "conv2d_act_f16: the problem is too large (M = %lld rows; split the batch)", M);
  PMCE_REQUIRE(out_pitch >= Cout && out_pitch < (1ll << 24) && (!R || (res_pitch >= Cout && res_pitch < (1ll << 24))),
               "conv2d_act_f16: the row pitches must be in Cout..2^24 (Cout=%d out pitch=%lld residual pitch=%lld)", Cout, out_pitch, res_pitch);
  ConvF16Params p{};
  p.X = x; p.sn = sn; p.sc = sc; p.sy = sy; p.sx = sx;
  p.H = H; p.W = W; p.Cin = Cin; p.OH = OH; p.OW = OW; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
  p.Wp = static_cast<const _Float16*>(Wp); p.wscale = wscale; p.bias = bias; p.R = static_cast<const _Float16*>(R);
  p.out = out; p.ldo = out_pitch; p.ldr = R ? res_pitch : 0;
  p.M = (int)M; p.N = Cout; p.K = Cin * KH * KW; p.KT = (p.K + 63) / 64 * 2;
  p.act = act; p.slope = act == CONV_ACT_LEAKY ? slope : 0.f; p.res_after = res_after_act;
  p.oflow = pmce_overflow_sink();
  p.ntn = (Cout + 63) / 64;  // one tile shape for every layer and every batch
  PMCE_REQUIRE((long long)((M + CONV_BM - 1) / CONV_BM) * p.ntn < (1ll << 31), "conv2d_act_f16: too many tiles");
  // never an alignment requirement: whatever the 16-byte loads cannot read goes through the element loads, to the same bits
  const bool fast = x_dtype == CONV_DTYPE_F16 && sc == 1 && Cin % 32 == 0 && sn % 8 == 0 && sy % 8 == 0 && sx % 8 == 0 &&
                    (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const bool o16 = out_dtype == CONV_DTYPE_F16;
  p.vec16 = o16 && Cout % 64 == 0 && out_pitch % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
            (!R || (res_pitch % 8 == 0 && (reinterpret_cast<uintptr_t>(R) & 15) == 0));
  if (fast) return o16 ? launch_conv_f16<GATHER_FAST, true>(p, stream) : launch_conv_f16<GATHER_FAST, false>(p, stream);
  if (x_dtype == CONV_DTYPE_F16) return o16 ? launch_conv_f16<GATHER_F16, true>(p, stream) : launch_conv_f16<GATHER_F16, false>(p, stream);
  return o16 ? launch_conv_f16<GATHER_F32, true>(p, stream) : launch_conv_f16<GATHER_F32, false>(p, stream);
}

extern "C" int pmce_maxpool3x3s2_nhwc_f16(const void* x, void* y, int n, int H, int W, int C, hipStream_t stream) {
  PMCE_REQUIRE(x && y, "maxpool3x3s2_f16: null pointer");
  PMCE_REQUIRE(n >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "maxpool3x3s2_f16: need n, H, W >= 1 and C %% 4 == 0 (n=%d H=%d W=%d C=%d)", n, H, W, C);
  PMCE_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 7) == 0, "maxpool3x3s2_f16: buffers must be 8-byte aligned");
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(maxpool3x3s2_f16_kernel, dim3(f16_grid_for((long long)n * OH * OW * (C / 4))), dim3(256), 0, stream,
                     static_cast<const _Float16*>(x), static_cast<_Float16*>(y), n, H, W, C, OH, OW);
  return pmce_check_launch("maxpool3x3s2_nhwc_f16");
}

extern "C" int pmce_avgpool_nhwc_f16_f32(const void* x, float* y, int n, int HW, int C, hipStream_t stream) {
  PMCE_REQUIRE(x && y, "avgpool_f16: null pointer");
  PMCE_REQUIRE(n >= 1 && HW >= 1 && C >= 1, "avgpool_f16: need n, HW, C >= 1 (n=%d HW=%d C=%d)", n, HW, C);
  hipLaunchKernelGGL(avgpool_f16_kernel, dim3(f16_grid_for((long long)n * C)), dim3(256), 0, stream, static_cast<const _Float16*>(x), y, n, HW, C);
  return pmce_check_launch("avgpool_nhwc_f16_f32");
}

extern "C" int pmce_upsample2x_nhwc_f16(const void* x, long long in_pitch, void* out, long long out_pitch, int n, int H, int W, int C,
                                        hipStream_t stream) {
  PMCE_REQUIRE(x && out, "upsample2x_f16: null pointer");
  PMCE_REQUIRE(n >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && H <= 16384 && W <= 16384,
               "upsample2x_f16: need n, H, W >= 1 (H, W <= 16384) and C %% 4 == 0 (n=%d H=%d W=%d C=%d)", n, H, W, C);
  PMCE_REQUIRE(in_pitch >= C && out_pitch >= C && in_pitch % 4 == 0 && out_pitch % 4 == 0 && in_pitch < (1ll << 24) && out_pitch < (1ll << 24),
               "upsample2x_f16: the pitches must be multiples of 4 in C..2^24 (C=%d in=%lld out=%lld)", C, in_pitch, out_pitch);
  PMCE_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 7) == 0,
               "upsample2x_f16: the buffers (the slice's first channel included) must be 8-byte aligned");
  hipLaunchKernelGGL(upsample2x_f16_kernel, dim3(f16_grid_for((long long)n * 4 * H * W * (C / 4))), dim3(256), 0, stream,
                     static_cast<const _Float16*>(x), in_pitch, static_cast<_Float16*>(out), out_pitch, n, H, W, C);
  return pmce_check_launch("upsample2x_nhwc_f16");
}

extern "C" int pmce_widen_f16_f32(const void* x, float* y, long long count, hipStream_t stream) {
  PMCE_REQUIRE(x && y, "widen_f16_f32: null pointer");
  PMCE_REQUIRE(count >= 1 && count < (1ll << 40), "widen_f16_f32: count must be in 1..2^40 (got %lld)", count);
  hipLaunchKernelGGL(widen_f16_kernel, dim3(f16_grid_for(count)), dim3(256), 0, stream, static_cast<const _Float16*>(x), y, count);
  return pmce_check_launch("widen_f16_f32");
}
