// Weak-perspective camera fit of the reference's demo, on device and batched over windows.
//
// What is restated (reference kasvii/PMCE):
//   * lib/models/project_net.py:6-16, OptimzeCamLayer: cam = (s, tx, ty), img_res = crop_size / 2,
//         pred[j][c] = (pose3d[j][c] + cam[1 + c]) * cam[0] * img_res + img_res            (c = 0, 1: the first two coordinates)
//   * main/run_demo.py:134-173, optimize_cam_param: per window a NEW torch.optim.Adam(lr = 0.1) on the SAME project_net (created once
//     per video, :245 - so a window starts from the previous window's camera), nn.L1Loss() against target[:, :17, :] (:156), 300 steps,
//     lr <- 0.05 after the step at j == 100, lr <- 0.001 after the step at j == 200 (:160-165).
//   * main/run_demo.py:49-67, convert_crop_cam_to_orig_img (== lib/utils/demo_utils.py:144-161 called with (x + w/2, y + h/2, h)).
//
// Without autograd, for one window with x[j][c] = scale * joints3d[j][c], R = crop_size / 2, N = 2 n_fit residuals:
//     r[j][c]  = (x[j][c] + t_c) s R + R - target[j][c]                 loss = sum |r| / N
//     dloss/ds = (R / N) sum_jc sign(r[j][c]) (x[j][c] + t_c)           sign(0) = 0, as torch's L1 backward
//     dloss/dt_c = (R / N) s sum_j sign(r[j][c])
// and Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay, moments zeroed per window), torch's single-tensor form:
//     m <- m + (g - m)(1 - b1)      v <- b2 v + (1 - b2) g g      cam <- cam - step_size_t m / (sqrt(v) / sqrt(bc2_t) + eps)
// with step_size_t = lr_t / (1 - b1^t) and bc2_t = 1 - b2^t.  The host computes the pair (step_size_t, sqrt(bc2_t)) per step in
// double, as torch does, and hands it over as a table [steps][2] of the compute type: no pow on the device, and the learning-rate
// schedule is the table's business.  The update is evaluated as
//     cam <- cam - (step_size_t sqrt(bc2_t)) m / (sqrt(v) + eps sqrt(bc2_t))
// which is the same quotient with ONE division per parameter instead of two (fp64 divisions are long sequences and everything here is
// one serial dependency chain).  fp64 reproduces the reference run in fp64 to rounding (tests: <= 1e-9 after 300 steps); in fp32 the loop
// is chaotic - a residual within an ulp of zero flips a sign term - and the result is held to what the reference's own fp32 run achieves.
//
// Mapping: one 64-lane wave owns one CHAIN of windows (seq_offsets[s] .. seq_offsets[s + 1] - 1; the first starts from init[s], each
// later one from its predecessor's result; a null table = every window its own chain).  Lane 2 j + c owns residual (j, c); lanes beyond
// 2 n_fit contribute zero.  Per step: the two sign sums are wave ballots + population counts (exact integers), the one floating-point sum
// is a DPP butterfly inside each row of 16 lanes followed by four lane reads added in a fixed order - no LDS, no atomics, and the same
// bits whatever the batch.  cam, m, v are wave-uniform registers.  In a chain the next window's <= 64 inputs are requested before the
// current window's loop starts and first touched after it.  Four waves per workgroup, nothing shared between them.  Results leave
// through vector stores of lane 0.
#include "common.hpp"

namespace {

constexpr int CAMFIT_MAX_FIT = 32;
constexpr int CAMFIT_WAVES = 4;

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float read_lane(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double read_lane(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// Sum over the 64 lanes, every lane active, in one fixed order: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
// leave every lane of a 16-lane row with that row's sum; the four row sums are read as scalars and added pairwise.
template <typename T>
__device__ __forceinline__ T wave_sum_fixed(T v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  return (read_lane(v, 0) + read_lane(v, 16)) + (read_lane(v, 32) + read_lane(v, 48));
}

template <typename T>
__device__ __forceinline__ T sqrt_ieee(T v);
template <>
__device__ __forceinline__ float sqrt_ieee<float>(float v) { return __fsqrt_rn(v); }
template <>
__device__ __forceinline__ double sqrt_ieee<double>(double v) { return __dsqrt_rn(v); }

template <typename T>
__device__ __forceinline__ void adam_update(T g, T& m, T& v, T& p, T a, T e) {
  m = m + (g - m) * T(1.0 - 0.9);
  v = T(0.999) * v + T(1.0 - 0.999) * g * g;
  p = p - a * m / (sqrt_ieee(v) + e);
}

template <typename T>
__global__ __launch_bounds__(64 * CAMFIT_WAVES) void camfit_kernel(const T* __restrict__ joints, const T* __restrict__ target,
                                                                   const T* __restrict__ init, const int* __restrict__ seq,
                                                                   const T* __restrict__ tab, T* __restrict__ cam_out,
                                                                   T* __restrict__ loss_out, const T* __restrict__ bbox,
                                                                   T* __restrict__ orig_cam, int S, int n_fit, int n_target, int steps,
                                                                   T scale, T R, T img_w, T img_h) {
  const int lane = threadIdx.x & 63;
  const int chain = blockIdx.x * CAMFIT_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (chain >= S) return;  // wave-uniform
  const int w0 = seq ? seq[chain] : chain;
  const int w1 = seq ? seq[chain + 1] : chain + 1;
  if (w0 >= w1) return;  // an empty chain owns no window
  const int j = lane >> 1, c = lane & 1;
  const bool act = lane < 2 * n_fit;
  const unsigned long long EVEN = 0x5555555555555555ull;
  const T inv_n = T(1) / T(2 * n_fit);
  const T Rn = R * inv_n;

  T s = init[3 * chain + 0], t0 = init[3 * chain + 1], t1 = init[3 * chain + 2];
  T x = act ? joints[((size_t)w0 * n_fit + j) * 3 + c] * scale : T(0);
  T tg = act ? target[((size_t)w0 * n_target + j) * 2 + c] : T(0);

  for (int w = w0; w < w1; ++w) {
    // the next window of the chain: requested now, first touched after the loop
    T nx = T(0), ntg = T(0);
    if (w + 1 < w1 && act) {
      nx = joints[((size_t)(w + 1) * n_fit + j) * 3 + c];
      ntg = target[((size_t)(w + 1) * n_target + j) * 2 + c];
    }
    T m0 = 0, m1 = 0, m2 = 0, v0 = 0, v1 = 0, v2 = 0;
    T st = tab[0], sb = tab[1];
    for (int t = 0; t < steps; ++t) {
      const int tn = min(t + 1, steps - 1);
      const T nst = tab[2 * tn], nsb = tab[2 * tn + 1];  // the next step's pair, a step ahead of its use
      const T a = x + (c ? t1 : t0);
      const T r = a * s * R + R - tg;
      const bool pos = act && r > T(0), neg = act && r < T(0);
      const T gs = wave_sum_fixed(pos ? a : (neg ? -a : T(0)));
      const unsigned long long bp = __ballot(pos), bn = __ballot(neg);
      const int c0 = __popcll(bp & EVEN) - __popcll(bn & EVEN);
      const int c1 = __popcll(bp & ~EVEN) - __popcll(bn & ~EVEN);
      const T sRn = s * Rn;
      const T g0 = gs * Rn, g1 = T(c0) * sRn, g2 = T(c1) * sRn;
      const T ua = st * sb, ue = T(1e-8) * sb;
      adam_update(g0, m0, v0, s, ua, ue);
      adam_update(g1, m1, v1, t0, ua, ue);
      adam_update(g2, m2, v2, t1, ua, ue);
      st = nst;
      sb = nsb;
    }
    // the loss at the returned camera: one more evaluation
    const T a = x + (c ? t1 : t0);
    const T r = a * s * R + R - tg;
    const T l = wave_sum_fixed(act ? (r < T(0) ? -r : r) : T(0)) * inv_n;
    if (lane == 0) {
      cam_out[3 * (size_t)w + 0] = s;
      cam_out[3 * (size_t)w + 1] = t0;
      cam_out[3 * (size_t)w + 2] = t1;
      loss_out[w] = l;
      if (bbox) {
        // run_demo.py:59-66, operation for operation
        const T bx = bbox[4 * (size_t)w + 0], by = bbox[4 * (size_t)w + 1], bw = bbox[4 * (size_t)w + 2], bh = bbox[4 * (size_t)w + 3];
        const T cx = bx + bw / T(2), cy = by + bh / T(2);
        const T hw = img_w / T(2), hh = img_h / T(2);
        const T sx = s * (T(1) / (img_w / bh));
        const T sy = s * (T(1) / (img_h / bh));
        orig_cam[4 * (size_t)w + 0] = sx;
        orig_cam[4 * (size_t)w + 1] = sy;
        orig_cam[4 * (size_t)w + 2] = ((cx - hw) / hw / sx) + t0;
        orig_cam[4 * (size_t)w + 3] = ((cy - hh) / hh / sy) + t1;
      }
    }
    x = nx * scale;
    tg = ntg;
  }
}

template <typename T>
int camfit_launch(const char* what, const T* joints3d, const T* target2d, const T* init, const int* seq_host, const int* seq_dev,
                  const T* step_table, T* cam, T* loss, const T* bbox, T* orig_cam, int W, int S, int n_fit, int n_target, int steps,
                  double scale, double crop_size, double img_w, double img_h, hipStream_t stream) {
  PMCE_REQUIRE(n_fit >= 1 && n_fit <= CAMFIT_MAX_FIT, "%s: n_fit must be in 1..32 (got %d)", what, n_fit);
  PMCE_REQUIRE(steps >= 1, "%s: steps must be >= 1 (got %d)", what, steps);
  PMCE_REQUIRE(n_target >= n_fit, "%s: target has %d rows, fewer than n_fit = %d", what, n_target, n_fit);
  PMCE_REQUIRE(W >= 1 && S >= 1, "%s: W and S must be >= 1 (got %d, %d)", what, W, S);
  PMCE_REQUIRE((seq_host == nullptr) == (seq_dev == nullptr), "%s: give seq_offsets on the host and on the device, or neither", what);
  if (seq_host) {
    PMCE_REQUIRE(seq_host[0] == 0 && seq_host[S] == W, "%s: seq_offsets must start at 0 and end at W = %d (got %d .. %d)", what, W,
                 seq_host[0], seq_host[S]);
    for (int i = 0; i < S; ++i)
      PMCE_REQUIRE(seq_host[i] <= seq_host[i + 1], "%s: seq_offsets must be monotone (entry %d: %d > %d)", what, i, seq_host[i],
                   seq_host[i + 1]);
  } else {
    PMCE_REQUIRE(S == W, "%s: without seq_offsets every window is its own chain: S must equal W (got %d, %d)", what, S, W);
  }
  const bool have_img = img_w > 0 && img_h > 0;
  PMCE_REQUIRE((bbox != nullptr) == have_img && (orig_cam != nullptr) == have_img,
               "%s: bbox, orig_cam and the image size go together (all or none)", what);
  PMCE_REQUIRE(crop_size > 0, "%s: crop_size must be positive", what);
  PMCE_REQUIRE(joints3d && target2d && init && step_table && cam && loss, "%s: null pointer", what);
  hipLaunchKernelGGL(camfit_kernel<T>, dim3((S + CAMFIT_WAVES - 1) / CAMFIT_WAVES), dim3(64 * CAMFIT_WAVES), 0, stream, joints3d,
                     target2d, init, seq_dev, step_table, cam, loss, bbox, orig_cam, S, n_fit, n_target, steps, (T)scale,
                     (T)(crop_size / 2), (T)img_w, (T)img_h);
  return pmce_check_launch(what);
}

}  // namespace

extern "C" int pmce_camfit_f32(const float* joints3d, const float* target2d, const float* init, const int* seq_offsets_host,
                               const int* seq_offsets, const float* step_table, float* cam, float* loss, const float* bbox,
                               float* orig_cam, int W, int S, int n_fit, int n_target, int steps, double scale, double crop_size,
                               double img_w, double img_h, hipStream_t stream) {
  return camfit_launch<float>("camfit_f32", joints3d, target2d, init, seq_offsets_host, seq_offsets, step_table, cam, loss, bbox,
                              orig_cam, W, S, n_fit, n_target, steps, scale, crop_size, img_w, img_h, stream);
}

extern "C" int pmce_camfit_f64(const double* joints3d, const double* target2d, const double* init, const int* seq_offsets_host,
                               const int* seq_offsets, const double* step_table, double* cam, double* loss, const double* bbox,
                               double* orig_cam, int W, int S, int n_fit, int n_target, int steps, double scale, double crop_size,
                               double img_w, double img_h, hipStream_t stream) {
  return camfit_launch<double>("camfit_f64", joints3d, target2d, init, seq_offsets_host, seq_offsets, step_table, cam, loss, bbox,
                               orig_cam, W, S, n_fit, n_target, steps, scale, crop_size, img_w, img_h, stream);
}
