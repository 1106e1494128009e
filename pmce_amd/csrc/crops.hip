// The demo's person crops (reference lib/utils/_dataset_demo.py:29-75 CropDataset), on frames that are already on the device.
//
//   pmce_crop_boxes    keypoints -> the per-frame box of get_all_bbox_params (lib/utils/smooth_bbox.py:36-103) and CropDataset's own lines
//                      (:48-50), the trim indices included.  fp64, one wavefront per frame, a lane per keypoint.  Not a hot path.
//   pmce_crop_patches  frames + boxes -> the S x S patches of get_single_image_crop_demo (lib/utils/_img_utils.py:53-101,219-251): the
//                      rot = 0 map of gen_trans_from_patch_cv in closed form, sampled by the fixed-point bilinear rule that OpenCV documents
//                      for warpAffine(INTER_LINEAR, BORDER_CONSTANT) on 8-bit images, then ToTensor + Normalize through a 3 x 256 table
//                      the host made with torch's own fp32 operations.  Integer arithmetic from the map's coefficients on: the same bits
//                      every run and whatever N.
//
// The patch kernel is bound by its fp32 output (602 KB per 224 x 224 patch).  A wavefront owns one output row at a time: its lanes take
// four adjacent x each, so that every plane row leaves as contiguous 16-byte stores, and everything that depends on the row alone (the
// source rows, their validity, the vertical fraction) is computed once per row and is wave-uniform.  What depends on the column alone
// (tap column, horizontal fraction) is computed once per lane and kept across the rows of the workgroup's band.  The 3-byte source pixels
// are unaligned and read with byte loads (served by L1 / L2: two source rows per output row, re-read by the neighbouring rows);
// DESIGN.md section 8 says what else was considered.  The sampling body is patch_sampler.hpp, shared with the 2D pose stage's patches
// (pose2d.hip).
#include "common.hpp"
#include "patch_sampler.hpp"

namespace {

using patch_sampler::MAX_SIDE;         // S
using patch_sampler::MAX_DIM;          // frame width / height
using patch_sampler::ROWS_PER_BLOCK;   // output rows of one workgroup: 8 per wave
using patch_sampler::in_reach;         // |v| <= 2^20 px

// ---------------------------------------------------------------------------------------------------------------------------------------
// boxes
// ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// kp_to_bbox_param of frame f, by the whole wave: (cx, cy, scale) and whether the frame is usable.  Every lane returns the same values.
__device__ __forceinline__ bool frame_param(const float* __restrict__ kp, int K, int f, double vis_thresh, int lane, double& cx, double& cy,
                                            double& scale) {
#pragma clang fp contract(off)
  const float* k = kp + (long long)f * K * 3;
  double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  bool any = false;
  for (int j = lane; j < K; j += 64) {
    if ((double)k[3 * j + 2] > vis_thresh) {
      const double x = (double)k[3 * j], y = (double)k[3 * j + 1];
      xmin = fmin(xmin, x);
      xmax = fmax(xmax, x);
      ymin = fmin(ymin, y);
      ymax = fmax(ymax, y);
      any = true;
    }
  }
  if (!__any(any)) return false;
  xmin = wave_min_d(xmin);
  xmax = wave_max_d(xmax);
  ymin = wave_min_d(ymin);
  ymax = wave_max_d(ymax);
  const double dx = xmax - xmin, dy = ymax - ymin;
  const double height = sqrt(dx * dx + dy * dy);
  if (!(height >= 0.5)) return false;          // person_height < 0.5 has no box; a NaN (a non-finite visible keypoint) has none here either
  cx = (xmin + xmax) / 2.0;
  cy = (ymin + ymax) / 2.0;
  scale = 150.0 / height;
  return true;
}

// One wavefront per frame.  An unusable frame walks to its nearest usable neighbours (recomputing their parameters: the gaps of a
// tracklet are short) and interpolates as np.linspace(prev, curr, n + 2)[1:-1] does.  Frame 0's wave finds the start of the span,
// frame N - 1's its end.
__global__ __launch_bounds__(256) void crop_boxes_kernel(const float* __restrict__ kp, int N, int K, double vis_thresh,
                                                         double* __restrict__ boxes, int* __restrict__ usable, int* __restrict__ span) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= N) return;
  double cx = 0, cy = 0, sc = 0;
  const bool ok = frame_param(kp, K, f, vis_thresh, lane, cx, cy, sc);
  int prev = f, next = f;
  bool inside = ok;
  if (!ok) {
    double pcx = 0, pcy = 0, psc = 0, ncx = 0, ncy = 0, nsc = 0;
    bool pok = false, nok = false;
    for (prev = f - 1; prev >= 0; --prev)
      if ((pok = frame_param(kp, K, prev, vis_thresh, lane, pcx, pcy, psc))) break;
    for (next = f + 1; next < N; ++next)
      if ((nok = frame_param(kp, K, next, vis_thresh, lane, ncx, ncy, nsc))) break;
    inside = pok && nok;
    if (inside) {
      const double div = (double)(next - prev), k = (double)(f - prev);      // n + 1 and the 1-based place inside the gap
      cx = pcx + k * ((ncx - pcx) / div);
      cy = pcy + k * ((ncy - pcy) / div);
      sc = psc + k * ((nsc - psc) / div);
    }
  }
  if (lane == 0) {
    const double qnan = __builtin_nan("");
    const double s = 150.0 / sc;               // _dataset_demo.py:49: the second division, kept
    double* b = boxes + 4ll * f;
    b[0] = inside ? cx : qnan;
    b[1] = inside ? cy : qnan;
    b[2] = inside ? s : qnan;
    b[3] = inside ? s : qnan;
    usable[f] = ok ? 1 : 0;
    // the span: (first usable, last usable + 1), or (-1, 0) without a usable frame
    if (f == 0) span[0] = ok ? 0 : (next < N ? next : -1);
    if (f == N - 1) span[1] = ok ? N : prev + 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// patches
// ---------------------------------------------------------------------------------------------------------------------------------------
// One axis of the inverse map, from the reference's text (gen_trans_from_patch_cv with rot = 0): the three source points are stored as
// float32, the 3-point solve is exact in closed form.  -> x_src = i * x_dst + t.
__device__ __forceinline__ void axis_map(double c, double size, double scale, int S, double& i, double& t) {
#pragma clang fp contract(off)
  const double c0 = (double)(float)c;
  const float half = (float)(size * scale * 0.5);
  const double d = (double)(float)(c + (double)half) - c0;
  const double hs = (double)S / 2.0;
  i = d / hs;
  t = c0 - hs * i;
}

// grid (N, bands of ROWS_PER_BLOCK rows).  table[3][256]: the normalised value of byte v in output channel c.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void crop_patches_kernel(const unsigned char* __restrict__ frames, int F, int H, int W,
                                                           const int* __restrict__ frame_index, const double* __restrict__ boxes, int N,
                                                           double scale, int S, int swap_rb, const float* __restrict__ table,
                                                           float* __restrict__ out_f32, unsigned char* __restrict__ out_u8,
                                                           int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ float lut[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) lut[i] = table[i];
  __syncthreads();
  const int n = blockIdx.x;
  const int y_begin = blockIdx.y * ROWS_PER_BLOCK, y_end = min(y_begin + ROWS_PER_BLOCK, S);

  const double bx = boxes[4ll * n], by = boxes[4ll * n + 1], bw = boxes[4ll * n + 2], bh = boxes[4ll * n + 3];
  const int fi = frame_index[n];
  int st = 0;
  double ix = 0, tx = 0, iy = 0, ty = 0;
  if (!(isfinite(bx) && isfinite(by) && isfinite(bw) && isfinite(bh)) || !(bw * scale > 0.0) || !(bh * scale > 0.0)) {
    st = 1;
  } else {
    axis_map(bx, bw, scale, S, ix, tx);
    axis_map(by, bh, scale, S, iy, ty);
    const double last = (double)(S - 1);
    if (!(in_reach(tx) && in_reach(ix * last + tx) && in_reach(ty) && in_reach(iy * last + ty))) st = 2;
  }
  if (st == 0 && (fi < 0 || fi >= F)) st = 3;       // reachable only through a device table (the host's is validated)
  if (blockIdx.y == 0 && threadIdx.x == 0) status[n] = st;
  const bool live = st == 0;

  const size_t plane = (size_t)S * S;
  float* of = out_f32 + (size_t)n * 3 * plane;
  unsigned char* ou = out_u8 ? out_u8 + (size_t)n * 3 * plane : nullptr;
  const unsigned char* frame = frames + (live ? (size_t)fi * H * W * 3 : 0);
  patch_sampler::sample_rows<ALIGNED, false>(frame, H, W, live, ix, tx, iy, ty, S, S, y_begin, y_end, swap_rb, lut, of, ou, nullptr,
                                             nullptr);
}

}  // namespace

extern "C" int pmce_crop_boxes(const float* keypoints, int N, int K, double vis_thresh, double* boxes, int* usable, int* span,
                               hipStream_t stream) {
  PMCE_REQUIRE(keypoints && boxes && usable && span, "crop_boxes: null pointer");
  PMCE_REQUIRE(N >= 1 && K >= 1, "crop_boxes: need N >= 1 frames of K >= 1 keypoints (got N = %d, K = %d)", N, K);
  PMCE_REQUIRE(vis_thresh == vis_thresh, "crop_boxes: vis_thresh is NaN");
  hipLaunchKernelGGL(crop_boxes_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, keypoints, N, K, vis_thresh, boxes, usable,
                     span);
  return pmce_check_launch("crop_boxes");
}

extern "C" int pmce_crop_patches(const unsigned char* frames, int n_frames, int height, int width, const int* frame_index_host,
                                 const int* frame_index, const double* boxes, int n_jobs, double scale, int side, int swap_rb,
                                 const float* norm_table, float* patch_f32, unsigned char* patch_u8, int* status, hipStream_t stream) {
  PMCE_REQUIRE(frames && frame_index && boxes && norm_table && patch_f32 && status, "crop_patches: null pointer");
  PMCE_REQUIRE(n_frames >= 1 && height >= 1 && height <= MAX_DIM && width >= 1 && width <= MAX_DIM,
               "crop_patches: need n_frames >= 1 and a frame of 1..%d x 1..%d (got %d frames of %d x %d)", MAX_DIM, MAX_DIM, n_frames,
               width, height);
  PMCE_REQUIRE(n_jobs >= 1, "crop_patches: need n_jobs >= 1 (got %d)", n_jobs);
  PMCE_REQUIRE(side >= 1 && side <= MAX_SIDE, "crop_patches: the patch side must be in 1..%d (got %d)", MAX_SIDE, side);
  PMCE_REQUIRE(scale == scale && scale - scale == 0.0, "crop_patches: scale must be finite");
  if (frame_index_host)
    for (int n = 0; n < n_jobs; ++n)
      PMCE_REQUIRE(frame_index_host[n] >= 0 && frame_index_host[n] < n_frames, "crop_patches: frame_index[%d] = %d, there are %d frames", n,
                   frame_index_host[n], n_frames);
  const dim3 grid((unsigned)n_jobs, (unsigned)((side + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
  if (side % 4 == 0)
    hipLaunchKernelGGL(crop_patches_kernel<true>, grid, dim3(256), 0, stream, frames, n_frames, height, width, frame_index, boxes, n_jobs,
                       scale, side, swap_rb ? 1 : 0, norm_table, patch_f32, patch_u8, status);
  else
    hipLaunchKernelGGL(crop_patches_kernel<false>, grid, dim3(256), 0, stream, frames, n_frames, height, width, frame_index, boxes, n_jobs,
                       scale, side, swap_rb ? 1 : 0, norm_table, patch_f32, patch_u8, status);
  return pmce_check_launch("crop_patches");
}
