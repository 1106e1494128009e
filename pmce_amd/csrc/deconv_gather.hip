// The second half of nn.ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) + eval-mode BatchNorm + ReLU (ViTPose's
// TopdownHeatmapSimpleHead).  The first half is one product on the split-f16 GEMM,
//     Y[n H W][16 Cout] = X[n H W][Cin] W'^T,      W'[(ky, kx, co)][ci] = W[ci][co][ky][kx] s[co]      (s = the BatchNorm scale),
// every input pixel's contribution to the 4 x 4 output pixels it touches.  This kernel gathers them:
//     out[n][oy][ox][co] = relu(sum Y[n][iy][ix][(ky, kx, co)] + b'[co])      over the (iy, ky), (ix, kx) with oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx
// - at most two (iy, ky) and two (ix, kx) per output pixel, fewer on the border -, summed in a fixed order: ky ascending, inside it
// kx ascending, the bias last.  One thread per output pixel and four channels; no atomics; a pixel depends on its own image only.
// The result is NHWC [n][2H][2W][Cout] fp32, or pre-split planes - the A operand of the next product.
#include "gemm_split_common.hpp"

namespace {

__global__ __launch_bounds__(256) void deconv4x4s2_gather_kernel(const float* __restrict__ Y, const float* __restrict__ bias, float* __restrict__ out,
                                                                 long long total, int H, int W, int Cout, int out_split) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int c4n = Cout >> 2;
  const int c = 4 * (int)(t % c4n);
  long long pix = t / c4n;  // (image, oy, ox)
  const int OW = 2 * W, OH = 2 * H;
  const int ox = (int)(pix % OW);
  pix /= OW;
  const int oy = (int)(pix % OH);
  const long long img = pix / OH;
  // ky = oy + 1 - 2 iy in 0..3: the smaller ky belongs to the larger iy
  const int iy_a = (oy + 1) >> 1, ky_a = oy + 1 - 2 * iy_a;
  const int ix_a = (ox + 1) >> 1, kx_a = ox + 1 - 2 * ix_a;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  bool first = true;
#pragma unroll
  for (int jy = 0; jy < 2; ++jy) {
    const int iy = iy_a - jy, ky = ky_a + 2 * jy;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int jx = 0; jx < 2; ++jx) {
      const int ix = ix_a - jx, kx = kx_a + 2 * jx;
      if (ix < 0 || ix >= W) continue;
      const f32x4 y = *reinterpret_cast<const f32x4*>(Y + ((img * H + iy) * W + ix) * (16ll * Cout) + (ky * 4 + kx) * Cout + c);
      acc = first ? y : f32x4{acc.x + y.x, acc.y + y.y, acc.z + y.z, acc.w + y.w};
      first = false;
    }
  }
  const f32x4 b = *reinterpret_cast<const f32x4*>(bias + c);
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float v = acc[e] + b[e];
    r[e] = v < 0.f ? 0.f : v;  // (a NaN stays a NaN)
  }
  float* orow = out + ((img * OH + oy) * OW + ox) * (long long)Cout;
  if (out_split) store4_split_f16(orow, c, r);
  else *reinterpret_cast<f32x4*>(orow + c) = r;
}

}  // namespace

extern "C" int pmce_deconv4x4s2_gather_f32(const float* Y, const float* bias, float* out, int n, int H, int W, int Cout, int out_split,
                                           hipStream_t stream) {
  PMCE_REQUIRE(Y && bias && out, "deconv4x4s2_gather: null pointer");
  PMCE_REQUIRE(n >= 1 && H >= 1 && W >= 1 && H <= 4096 && W <= 4096, "deconv4x4s2_gather: need n >= 1 and H, W in 1..4096 (got n=%d H=%d W=%d)", n, H, W);
  PMCE_REQUIRE(Cout >= 16 && Cout % 16 == 0 && Cout <= 65536, "deconv4x4s2_gather: Cout must be a multiple of 16 in 16..65536 (got Cout=%d)", Cout);
  PMCE_REQUIRE(((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
               "deconv4x4s2_gather: every buffer must be 16-byte aligned");
  const long long total = (long long)n * (2 * H) * (2 * W) * (Cout / 4);
  PMCE_REQUIRE((total + 255) / 256 < (1ll << 31), "deconv4x4s2_gather: too many output elements (n=%d)", n);
  hipLaunchKernelGGL(deconv4x4s2_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, Y, bias, out, total, H, W, Cout,
                     out_split);
  return pmce_check_launch("deconv4x4s2_gather");
}
