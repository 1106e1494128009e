// The demo's 2D pose stage around the network (reference main/run_demo.py:264-286, inference_top_down_pose_model with the config
// pose_detector/ViTPose_huge_coco_256x192.py): tracker boxes to the network's patches, and its heatmaps to keypoints.  include/pmce_hip.h
// (the pose2d section) states every formula; they were written from mmpose 0.x's published text and OpenCV's documented warpAffine rule.
//
//   pmce_pose_patches  frames + boxes -> the Hp x Wp patches of TopDownAffine (use_udp, rotation 0): _box2cs and the UDP map with their
//                      float roundings spelled out, OpenCV's fp64 inversion of the float matrix, then the sampling body of the person
//                      crops (patch_sampler.hpp).  Optionally the x-mirrored patches of the flip test in the same launch.
//   pmce_pose_decode   heatmaps (+ the flipped set) -> keypoints: the flip average, the first maximum, DARK's Taylor step on the
//                      blurred log map (post_dark_udp, kernel 11) and transform_preds, in one launch.  One workgroup per image.  The
//                      blur is evaluated only where the step reads it: nine values per keypoint, from a 13-row x 3-column strip of the
//                      horizontal pass.  No atomics; an image's bits do not depend on the batch.
#include "common.hpp"
#include "patch_sampler.hpp"

namespace {

using patch_sampler::MAX_SIDE;
using patch_sampler::MAX_DIM;
using patch_sampler::ROWS_PER_BLOCK;
using patch_sampler::in_reach;

constexpr int MAX_K = 64;            // keypoints
constexpr int MAX_HEAT = 4096;       // heatmap width / height
constexpr int BLUR = 11, RAD = 5;    // modulate_kernel and its radius
constexpr int STRIP = 2 * RAD + 3;   // rows of the horizontal pass a keypoint needs: py - 6 .. py + 6
constexpr int THREADS = 256;

// ---------------------------------------------------------------------------------------------------------------------------------------
// patches
// ---------------------------------------------------------------------------------------------------------------------------------------
// One axis of TopDownAffine's UDP map, inverted as cv2.warpAffine does: m = (float)((S - 1) / wt), b = (float)(m' * (0.5 wt - c)).
__device__ __forceinline__ void udp_axis(float c, float wt, int S, float& m, float& b) {
#pragma clang fp contract(off)
  const double k = (double)(S - 1) / (double)wt;
  const float off = 0.5f * wt - c;
  m = (float)k;
  b = (float)(k * (double)off);
}

// grid (N, bands of ROWS_PER_BLOCK rows).  boxes[N][4] fp64: (x, y, w, h), or (cx, cy, w, h) with `centred`.
template <bool ALIGNED, bool MIRROR>
__global__ __launch_bounds__(256) void pose_patches_kernel(const unsigned char* __restrict__ frames, int F, int H, int W,
                                                           const int* __restrict__ frame_index, const double* __restrict__ boxes, int N,
                                                           int centred, float padding, int SH, int SW, int swap_rb,
                                                           const float* __restrict__ table, float* __restrict__ out_f32,
                                                           unsigned char* __restrict__ out_u8, float* __restrict__ centre_scale,
                                                           int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ float lut[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) lut[i] = table[i];
  __syncthreads();
  const int n = blockIdx.x;
  const int y_begin = blockIdx.y * ROWS_PER_BLOCK, y_end = min(y_begin + ROWS_PER_BLOCK, SH);

  double bx = boxes[4ll * n], by = boxes[4ll * n + 1], bw = boxes[4ll * n + 2], bh = boxes[4ll * n + 3];
  const int fi = frame_index[n];
  int st = 0;
  double ix = 0, tx = 0, iy = 0, ty = 0;
  float cx = 0.f, cy = 0.f, wt = 0.f, ht = 0.f;
  if (!(isfinite(bx) && isfinite(by) && isfinite(bw) && isfinite(bh)) || !(bw > 0.0) || !(bh > 0.0)) {
    st = 1;
  } else {
    if (centred) {
      bx = bx - 0.5 * bw;
      by = by - 0.5 * bh;
    }
    // _box2cs
    const double a = (double)SW / (double)SH;
    cx = (float)(bx + 0.5 * bw);
    cy = (float)(by + 0.5 * bh);
    if (bw > a * bh)
      bh = bw / a;
    else if (bw < a * bh)
      bw = bh * a;
    const float sx = (float)(bw / 200.0) * padding, sy = (float)(bh / 200.0) * padding;
    wt = sx * 200.0f;
    ht = sy * 200.0f;
    // the UDP map, then OpenCV's inversion of the float matrix in fp64
    float m00, m02, m11, m12;
    udp_axis(cx, wt, SW, m00, m02);
    udp_axis(cy, ht, SH, m11, m12);
    const double D = 1.0 / ((double)m00 * (double)m11);
    ix = (double)m11 * D;
    iy = (double)m00 * D;
    tx = -ix * (double)m02;
    ty = -iy * (double)m12;
    if (!(in_reach(tx) && in_reach(ix * (double)(SW - 1) + tx) && in_reach(ty) && in_reach(iy * (double)(SH - 1) + ty))) st = 2;
  }
  if (st == 0 && (fi < 0 || fi >= F)) st = 3;       // reachable only through a device table (the host's is validated)
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    status[n] = st;
    float* cs = centre_scale + 4ll * n;
    cs[0] = cx;
    cs[1] = cy;
    cs[2] = wt;
    cs[3] = ht;
  }
  const bool live = st == 0;

  const size_t patch = (size_t)3 * SH * SW;
  float* of = out_f32 + (size_t)n * patch;
  unsigned char* ou = out_u8 ? out_u8 + (size_t)n * patch : nullptr;
  float* of_m = MIRROR ? out_f32 + ((size_t)N + n) * patch : nullptr;
  unsigned char* ou_m = MIRROR && out_u8 ? out_u8 + ((size_t)N + n) * patch : nullptr;
  const unsigned char* frame = frames + (live ? (size_t)fi * H * W * 3 : 0);
  patch_sampler::sample_rows<ALIGNED, MIRROR>(frame, H, W, live, ix, tx, iy, ty, SH, SW, y_begin, y_end, swap_rb, lut, of, ou, of_m, ou_m);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// decoding
// ---------------------------------------------------------------------------------------------------------------------------------------
struct DecodeTables {
  float g[BLUR];                 // the blur's taps
  unsigned char perm[MAX_K];     // the flipped set's channel for channel k
};

// heat[k][y][x] through element strides; the image's base is already applied.
struct HeatView {
  const float* p;
  long long sk, sy, sx;
};

// A[k][y][x]: the plain heatmap, or its average with the flipped set's (channel perm[k], column Wh - 1 - x).
template <bool FLIP>
__device__ __forceinline__ float averaged(const HeatView& h, const HeatView& f, int k, int kf, int y, int x, int Wh) {
#pragma clang fp contract(off)
  const float v = h.p[k * h.sk + y * h.sy + x * h.sx];
  if (!FLIP) return v;
  const float w = f.p[kf * f.sk + y * f.sy + (long long)(Wh - 1 - x) * f.sx];
  return (v + w) * 0.5f;
}

// BORDER_REFLECT_101, for an index at most n - 1 outside [0, n); clamped besides, so that a strip row nobody reads stays in bounds
__device__ __forceinline__ int reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i > n - 1) i = 2 * (n - 1) - i;
  return min(max(i, 0), n - 1);
}
__device__ __forceinline__ int clampi(int i, int n) { return min(max(i, 0), n - 1); }

// grid (n images), 256 threads.
template <bool FLIP>
__global__ __launch_bounds__(THREADS) void pose_decode_kernel(HeatView heat, long long sn, HeatView flipped, long long fn, int K, int Hh,
                                                              int Wh, DecodeTables tab, const float* __restrict__ centre_scale,
                                                              const int* __restrict__ status, float* __restrict__ keypoints,
                                                              float* __restrict__ coords, int* __restrict__ argmax) {
#pragma clang fp contract(off)
  __shared__ float s_max[THREADS];
  __shared__ int s_idx[THREADS];
  __shared__ float s_score[MAX_K];
  __shared__ int s_pos[MAX_K];
  __shared__ float s_strip[MAX_K * STRIP * 3];      // [k][r][c]: the horizontal pass at row reflect(py - 6 + r), column clamp(px - 1 + c)
  __shared__ float s_log[MAX_K * 9];                // [k][dy + 1][dx + 1]

  const int img = blockIdx.x;
  const int tid = threadIdx.x;
  heat.p += (long long)img * sn;
  if (FLIP) flipped.p += (long long)img * fn;
  const int npix = Hh * Wh;

  // 1. the first maximum of A[k]: thread (k, j) walks the pixels j, j + P, ... in ascending order
  const int P = THREADS / K;                        // pixel lanes per keypoint; P * K threads work
  {
    const int k = tid % K, j = tid / K;
    float best = -INFINITY;
    int at = 0x7fffffff;
    if (j < P) {
      const int kf = tab.perm[k];
      for (int p = j; p < npix; p += P) {
        const float v = averaged<FLIP>(heat, flipped, k, kf, p / Wh, p % Wh, Wh);
        if (at == 0x7fffffff || v > best) {
          best = v;
          at = p;
        }
      }
    }
    s_max[tid] = best;
    s_idx[tid] = at;
  }
  __syncthreads();
  if (tid < K) {
    float best = s_max[tid];
    int at = s_idx[tid];                            // lane 0 of a keypoint always has a pixel: npix >= 36
    for (int j = 1; j < P; ++j) {
      const float v = s_max[j * K + tid];
      const int p = s_idx[j * K + tid];
      if (p != 0x7fffffff && (v > best || (v == best && p < at))) {
        best = v;
        at = p;
      }
    }
    s_score[tid] = best;
    s_pos[tid] = at;
  }
  __syncthreads();

  // 2. the horizontal pass on the strip of every refined keypoint
  for (int it = tid; it < K * STRIP * 3; it += THREADS) {
    const int k = it / (STRIP * 3), r = (it / 3) % STRIP, c = it % 3;
    if (!(s_score[k] > 0.0f)) continue;
    const int px = s_pos[k] % Wh, py = s_pos[k] / Wh;
    const int y = reflect101(py - (RAD + 1) + r, Hh), x = clampi(px - 1 + c, Wh);
    const int kf = tab.perm[k];
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < BLUR; ++i) acc = acc + tab.g[i] * averaged<FLIP>(heat, flipped, k, kf, y, reflect101(x + i - RAD, Wh), Wh);
    s_strip[it] = acc;
  }
  __syncthreads();
  // 3. the vertical pass and the log map at the nine points (edge replication = the clamped index)
  for (int it = tid; it < K * 9; it += THREADS) {
    const int k = it / 9, dy = (it / 3) % 3, c = it % 3;
    if (!(s_score[k] > 0.0f)) continue;
    const int py = s_pos[k] / Wh;
    const int r0 = clampi(py - 1 + dy, Hh) - RAD - (py - (RAD + 1));       // strip row of the first tap: 0, 1 or 2
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < BLUR; ++j) acc = acc + tab.g[j] * s_strip[(k * STRIP + r0 + j) * 3 + c];
    // the logarithm is taken in fp64 and rounded once: where the Hessian is nearly singular the step amplifies every ulp of L
    s_log[it] = (float)log((double)fminf(fmaxf(acc, 0.001f), 50.0f));
  }
  __syncthreads();
  // 4. the Taylor step and the way back to the image
  if (tid < K) {
    const int k = tid;
    const float score = s_score[k];
    const int px = s_pos[k] % Wh, py = s_pos[k] / Wh;
    float hx = -1.0f, hy = -1.0f;
    int ax = -1, ay = -1;
    if (score > 0.0f) {
      const float* L = s_log + k * 9;
      const float c = L[4];
      const float dx = 0.5f * (L[5] - L[3]), dy = 0.5f * (L[7] - L[1]);
      const float dxx = L[5] - 2.0f * c + L[3], dyy = L[7] - 2.0f * c + L[1];
      const float dxy = 0.5f * (L[8] - L[5] - L[7] + c + c - L[3] - L[1] + L[0]);
      const double eps = 1.1920928955078125e-07;    // 2^-23
      const double a = (double)dxx + eps, d = (double)dyy + eps, b = (double)dxy;
      const double det = a * d - b * b;
      const double ox = (d * (double)dx - b * (double)dy) / det, oy = (a * (double)dy - b * (double)dx) / det;
      hx = (float)((double)px - ox);
      hy = (float)((double)py - oy);
      ax = px;
      ay = py;
    }
    const long long o = (long long)img * K + k;
    if (coords) {
      coords[2 * o] = hx;
      coords[2 * o + 1] = hy;
    }
    if (argmax) {
      argmax[2 * o] = ax;
      argmax[2 * o + 1] = ay;
    }
    float* kp = keypoints + 3 * o;
    if (status && status[img] != 0) {
      kp[0] = 0.0f;
      kp[1] = 0.0f;
      kp[2] = 0.0f;
    } else {
      const float* cs = centre_scale + 4ll * img;
      const float cx = cs[0], cy = cs[1], wt = cs[2], ht = cs[3];
      const float kx = (float)((double)wt / (double)(Wh - 1)), ky = (float)((double)ht / (double)(Hh - 1));
      const float x1 = hx * kx, y1 = hy * ky;
      const float x2 = x1 + cx, y2 = y1 + cy;
      kp[0] = x2 - 0.5f * wt;
      kp[1] = y2 - 0.5f * ht;
      kp[2] = score;
    }
  }
}

}  // namespace

extern "C" int pmce_pose_patches(const unsigned char* frames, int n_frames, int height, int width, const int* frame_index_host,
                                 const int* frame_index, const double* boxes, int n_jobs, int centred, double padding, int patch_h,
                                 int patch_w, int swap_rb, int mirror, const float* norm_table, float* patch_f32,
                                 unsigned char* patch_u8, float* centre_scale, int* status, hipStream_t stream) {
  PMCE_REQUIRE(frames && frame_index && boxes && norm_table && patch_f32 && centre_scale && status, "pose_patches: null pointer");
  PMCE_REQUIRE(n_frames >= 1 && height >= 1 && height <= MAX_DIM && width >= 1 && width <= MAX_DIM,
               "pose_patches: need n_frames >= 1 and a frame of 1..%d x 1..%d (got %d frames of %d x %d)", MAX_DIM, MAX_DIM, n_frames,
               width, height);
  PMCE_REQUIRE(n_jobs >= 1 && n_jobs <= (1 << 30), "pose_patches: need n_jobs >= 1 (got %d)", n_jobs);
  PMCE_REQUIRE(patch_h >= 2 && patch_h <= MAX_SIDE && patch_w >= 2 && patch_w <= MAX_SIDE,
               "pose_patches: the patch must be 2..%d high and wide (got %d x %d)", MAX_SIDE, patch_h, patch_w);
  PMCE_REQUIRE(padding > 0.0 && padding - padding == 0.0, "pose_patches: padding must be finite and positive");
  if (frame_index_host)
    for (int n = 0; n < n_jobs; ++n)
      PMCE_REQUIRE(frame_index_host[n] >= 0 && frame_index_host[n] < n_frames, "pose_patches: frame_index[%d] = %d, there are %d frames", n,
                   frame_index_host[n], n_frames);
  const dim3 grid((unsigned)n_jobs, (unsigned)((patch_h + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
#define PMCE_POSE_PATCHES(A, M)                                                                                                        \
  hipLaunchKernelGGL((pose_patches_kernel<A, M>), grid, dim3(256), 0, stream, frames, n_frames, height, width, frame_index, boxes,    \
                     n_jobs, centred ? 1 : 0, (float)padding, patch_h, patch_w, swap_rb ? 1 : 0, norm_table, patch_f32, patch_u8,      \
                     centre_scale, status)
  if (patch_w % 4 == 0) {
    if (mirror)
      PMCE_POSE_PATCHES(true, true);
    else
      PMCE_POSE_PATCHES(true, false);
  } else {
    if (mirror)
      PMCE_POSE_PATCHES(false, true);
    else
      PMCE_POSE_PATCHES(false, false);
  }
#undef PMCE_POSE_PATCHES
  return pmce_check_launch("pose_patches");
}

extern "C" int pmce_pose_decode(const float* heat, long long sn, long long sk, long long sy, long long sx, const float* heat_flipped,
                                long long fn, long long fk, long long fy, long long fx, int n, int K, int heat_h, int heat_w,
                                const int* perm_host, const float* blur_host, const float* centre_scale, const int* status,
                                float* keypoints, float* coords, int* argmax, hipStream_t stream) {
  PMCE_REQUIRE(heat && blur_host && centre_scale && keypoints, "pose_decode: null pointer");
  PMCE_REQUIRE(n >= 1, "pose_decode: need n >= 1 images (got %d)", n);
  PMCE_REQUIRE(K >= 1 && K <= MAX_K, "pose_decode: K must be in 1..%d (got %d)", MAX_K, K);
  PMCE_REQUIRE(heat_h >= RAD + 1 && heat_h <= MAX_HEAT && heat_w >= RAD + 1 && heat_w <= MAX_HEAT,
               "pose_decode: the heatmaps must be %d..%d high and wide (got %d x %d)", RAD + 1, MAX_HEAT, heat_h, heat_w);
  PMCE_REQUIRE(!heat_flipped || perm_host, "pose_decode: a flipped set needs its channel permutation");
  DecodeTables tab;
  for (int i = 0; i < BLUR; ++i) tab.g[i] = blur_host[i];
  for (int k = 0; k < MAX_K; ++k) tab.perm[k] = (unsigned char)(k < K ? k : 0);
  if (heat_flipped)
    for (int k = 0; k < K; ++k) {
      PMCE_REQUIRE(perm_host[k] >= 0 && perm_host[k] < K, "pose_decode: perm[%d] = %d, there are %d keypoints", k, perm_host[k], K);
      tab.perm[k] = (unsigned char)perm_host[k];
    }
  const HeatView h{heat, sk, sy, sx}, f{heat_flipped, fk, fy, fx};
  if (heat_flipped)
    hipLaunchKernelGGL(pose_decode_kernel<true>, dim3((unsigned)n), dim3(THREADS), 0, stream, h, sn, f, fn, K, heat_h, heat_w, tab,
                       centre_scale, status, keypoints, coords, argmax);
  else
    hipLaunchKernelGGL(pose_decode_kernel<false>, dim3((unsigned)n), dim3(THREADS), 0, stream, h, sn, f, fn, K, heat_h, heat_w, tab,
                       centre_scale, status, keypoints, coords, argmax);
  return pmce_check_launch("pose_decode");
}
