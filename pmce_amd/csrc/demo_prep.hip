// The demo's per-window target preparation (reference main/run_demo.py:340-344), one launch for a table of windows.
//
// For window w with middle frame m (start + t_mid, or start when start == end: one frame repeated):
//   joints  = the J0 detected keypoints of frame m + pelvis + neck          (add_pelvis_and_neck, run_demo.py:116-128)
//   box     = get_bbox(joints)                                              (lib/coord_utils.py:45-63)
//   bbox    = process_bbox(box, aspect_ratio = 1, scale = box_scale)        (coord_utils.py:66-90, with its x + (w - 1) step)
//   target  = the rot = 0 affine of j2d_processing onto crop x crop pixels  (lib/aug_utils.py:51-64,140-173)
//   mid     = target / width * 2 - (1, height / width)                      (normalize_screen_coordinates of what j2d_processing
//                                                                            wrote back IN PLACE into the window's middle row)
// The reference computes the box in float32 (torch scalars in get_bbox, numpy float32 scalars in process_bbox): every operation below is
// the reference's, in its order, each rounded once (no contraction), so the box carries the reference's bits.  Its affine map is a float64
// solve (cv2.getAffineTransform); for rot = 0 the three point pairs reduce to  x' = (x - cx) * (crop / w) + crop / 2  (both axes scale by
// the WIDTH, aug_utils.py:150), evaluated here in float32.
#include "common.hpp"

namespace {

__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

constexpr int MAX_JOINTS = 64;  // one lane per joint

// One wavefront per window, lane j = joint j.
__global__ __launch_bounds__(256) void demo_targets_kernel(const float* __restrict__ kp, int kp_stride, const int* __restrict__ win,
                                                           float* __restrict__ bbox, float* __restrict__ target2d,
                                                           float* __restrict__ mid_pose2d, int* __restrict__ valid, int W, int L, int J0,
                                                           int t_mid, float img_w, float img_h, float crop, float box_scale, int lhip,
                                                           int rhip, int lsho, int rsho) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= W) return;
  const int J = J0 + 2;
  const int s0 = win[2 * w], e0 = win[2 * w + 1];
  const int m = min(max(s0 == e0 ? s0 : s0 + t_mid, 0), L - 1);
  const float* k = kp + (long long)m * J0 * kp_stride;
  float x = 0.f, y = 0.f;
  if (lane < J0) {
    x = k[lane * kp_stride];
    y = k[lane * kp_stride + 1];
  } else if (lane < J) {
    const int a = lane == J0 ? lhip : lsho, b = lane == J0 ? rhip : rsho;
    x = (k[a * kp_stride] + k[b * kp_stride]) * 0.5f;
    y = (k[a * kp_stride + 1] + k[b * kp_stride + 1]) * 0.5f;
  }
  const bool on = lane < J;
  // a non-finite keypoint has no box in the reference either (its comparisons are all false): the window is reported invalid
  const bool finite = __all(!on || (isfinite(x) && isfinite(y)));
  float xmin = wave_min_f(on ? x : INFINITY), xmax = wave_max_f(on ? x : -INFINITY);
  float ymin = wave_min_f(on ? y : INFINITY), ymax = wave_max_f(on ? y : -INFINITY);
  // get_bbox
  const float xc = (xmin + xmax) * 0.5f, wd = xmax - xmin;
  xmin = xc - 0.5f * wd;
  xmax = xc + 0.5f * wd;
  const float yc = (ymin + ymax) * 0.5f, ht = ymax - ymin;
  ymin = yc - 0.5f * ht;
  ymax = yc + 0.5f * ht;
  const float gx = xmin, gy = ymin, gw = xmax - xmin, gh = ymax - ymin;
  // process_bbox: sanitise, then the square box around the same centre, scaled
  const float x2 = gx + (gw - 1.0f), y2 = gy + (gh - 1.0f);
  const bool ok = finite && gw * gh > 0.f && x2 >= gx && y2 >= gy;
  float bw = x2 - gx, bh = y2 - gy;
  const float c_x = gx + bw * 0.5f, c_y = gy + bh * 0.5f;
  if (bw > bh) bh = bw;
  else if (bw < bh) bw = bh;
  const float qnan = __builtin_nanf("");
  const float ow = ok ? bw * box_scale : qnan, oh = ok ? bh * box_scale : qnan;
  const float ox = ok ? c_x - ow * 0.5f : qnan, oy = ok ? c_y - oh * 0.5f : qnan;
  if (lane == 0) {
    float* b = bbox + 4ll * w;
    b[0] = ox;
    b[1] = oy;
    b[2] = ow;
    b[3] = oh;
    valid[w] = ok ? 1 : 0;
  }
  if (on) {
    // get_center_scale + get_affine_transform(rot = 0): centre of the box, scale crop / box width on both axes
    const float cx = ox + ow * 0.5f, cy = oy + oh * 0.5f;
    const float sc = crop / ow, half = crop * 0.5f;
    const float tx = (x - cx) * sc + half, ty = (y - cy) * sc + half;
    const long long o = ((long long)w * J + lane) * 2;
    target2d[o] = tx;
    target2d[o + 1] = ty;
    // normalize_screen_coordinates of the crop coordinates - the association of pmce_prepare_pose2d_f32
    mid_pose2d[o] = tx / img_w * 2.0f - 1.0f;
    mid_pose2d[o + 1] = ty / img_w * 2.0f - img_h / img_w;
  }
}

// pose[w][t_mid][j][:] = mid[w][j][:] - the demo's in-place overwrite of the middle frame of assembled windows
__global__ __launch_bounds__(256) void demo_override_mid_kernel(float* __restrict__ pose, const float* __restrict__ mid, long long n,
                                                                int J2, int T, int t_mid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // over W * J * 2
  if (i >= n) return;
  const long long w = i / J2;
  pose[(w * T + t_mid) * J2 + i % J2] = mid[i];
}

}  // namespace

extern "C" int pmce_demo_targets_f32(const float* kp, int kp_stride, const int* win, float* bbox, float* target2d, float* mid_pose2d,
                                     int* valid, int W, int L, int J0, int t_mid, float img_w, float img_h, float crop_size,
                                     float box_scale, int lhip, int rhip, int lsho, int rsho, hipStream_t stream) {
  PMCE_REQUIRE(kp && win && bbox && target2d && mid_pose2d && valid, "demo_targets: null pointer");
  PMCE_REQUIRE(W > 0 && L > 0 && J0 > 0 && J0 + 2 <= MAX_JOINTS && kp_stride >= 2, "demo_targets: need W, L > 0, 1 <= J0 <= %d, kp_stride >= 2",
               MAX_JOINTS - 2);
  PMCE_REQUIRE(t_mid >= 0 && img_w > 0.f && img_h > 0.f && crop_size > 0.f && box_scale > 0.f, "demo_targets: bad size or scale");
  PMCE_REQUIRE(lhip >= 0 && lhip < J0 && rhip >= 0 && rhip < J0 && lsho >= 0 && lsho < J0 && rsho >= 0 && rsho < J0,
               "demo_targets: hip / shoulder index out of range");
  hipLaunchKernelGGL(demo_targets_kernel, dim3((unsigned)((W + 3) / 4)), dim3(256), 0, stream, kp, kp_stride, win, bbox, target2d,
                     mid_pose2d, valid, W, L, J0, t_mid, img_w, img_h, crop_size, box_scale, lhip, rhip, lsho, rsho);
  return pmce_check_launch("demo_targets");
}

extern "C" int pmce_demo_override_mid_f32(float* pose_windows, const float* mid_pose2d, int W, int T, int J, int t_mid,
                                          hipStream_t stream) {
  PMCE_REQUIRE(pose_windows && mid_pose2d && W > 0 && J > 0 && T > 0 && t_mid >= 0 && t_mid < T, "demo_override_mid: bad args");
  const long long n = (long long)W * J * 2;
  hipLaunchKernelGGL(demo_override_mid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, pose_windows, mid_pose2d, n,
                     J * 2, T, t_mid);
  return pmce_check_launch("demo_override_mid");
}
