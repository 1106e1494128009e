// The debug overlay of the demo, on device: the tracker's boxes and ids and the pose stage's 2D skeletons drawn on the frames
// (the rules are this project's own and all integer, so the picture is pinned to the byte).  A ROW is one person in
// one frame; its primitives, in drawing order: the four edges of its box (top, right, bottom, left), the label with its id, the limbs
// in the skeleton's order, the keypoints' discs.  The coverage rules are overlay_cover.hpp's.
//
// Two stages per chunk of frames, plain launches on the caller's stream:
//   raster   SLICES workgroups per (row, primitive): they walk the primitive's bounding box, clipped to the frame, and for every covered
//            pixel do ONE 32-bit atomic max of  (row << 2 | level) + 1  into the pixel's key.  Rows of a frame are drawn in the order
//            given, so the larger row index wins; inside a row every primitive has the person's colour except the label's digits, so three
//            levels order a row: 0 box, 1 label ground, 2 digits, 3 limbs and discs.  Max commutes: the winner does not depend on the
//            order of arrival, on the other frames and rows of the call, or on the chunking.
//   resolve  one lane per pixel of the chunk: a non-empty key names the winner; its colour is blended in once and the key is put back
//            to empty, so the buffer serves the next chunk without a clearing pass (the call clears it once, on entry).
#include "common.hpp"
#include "overlay_cover.hpp"

#include <algorithm>

namespace {

using namespace overlay_cover;

constexpr int MAX_DIM = 8192;
constexpr int THREADS = 256;
constexpr int SLICES = 8;  // workgroups that share a primitive's bounding box (grid.z): a limb across a 1080p frame is 2M pixel tests
constexpr int STATUS_SKIPPED = 1;  // a non-finite or empty box, a non-finite keypoint, an id out of range: that primitive (row) is skipped
constexpr int STATUS_GUARD = 2;    // a primitive with an endpoint beyond the guard band was dropped
constexpr int STATUS_FRAME = 4;    // frame_index outside the frames: the row drew nothing
constexpr int BOX_XYXY = 0, BOX_CXCYWH = 1, BOX_XYWH = 2;
constexpr int GLYPH_W = 5, GLYPH_H = 7, CELL_W = 6, CELL_H = 8;
constexpr long long ID_END = 1000000000ll;
constexpr int LEVEL_BOX = 0, LEVEL_LABEL = 1, LEVEL_TEXT = 2, LEVEL_POSE = 3;

struct DrawParams {
  int F, W, H, f0, f1;      // the frames, and the chunk [f0, f1) this launch draws
  int box_format, K, D, L;  // keypoints per row, their components (2 or 3), limbs
  double score_thresh;
  int thickness, radius, label_scale;
};

struct Corners {
  double x1, y1, x2, y2;
  bool ok;  // finite, w > 0 and h > 0
};

__device__ __forceinline__ Corners box_corners(const double* __restrict__ b, int format) {
#pragma clang fp contract(off)
  // Written as selects over the format.  v - 0.0 is v to the bit, so a corner that is given as it is passes through unchanged.
  const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
  const bool corners = format == BOX_XYXY, centred = format == BOX_CXCYWH;
  const double back_x = centred ? 0.5 * b2 : 0.0, back_y = centred ? 0.5 * b3 : 0.0;  // from (b0, b1) back to the top left corner
  const double on_x = centred ? 0.5 * b2 : b2, on_y = centred ? 0.5 * b3 : b3;        // ... and on to the bottom right one
  Corners c;
  c.x1 = b0 - back_x;
  c.y1 = b1 - back_y;
  c.x2 = corners ? b2 : b0 + on_x;
  c.y2 = corners ? b3 : b1 + on_y;
  const double w = corners ? b2 - b0 : b2, h = corners ? b3 - b1 : b3;
  c.ok = isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3) && w > 0.0 && h > 0.0;
  return c;
}

// 0: not drawn (its score is below the threshold), 1: drawn, 2: not finite
__device__ __forceinline__ int keypoint_state(const double* __restrict__ kp, int D, double score_thresh) {
  if (!(isfinite(kp[0]) && isfinite(kp[1]))) return 2;
  if (D < 3) return 1;
  if (!isfinite(kp[2])) return 2;
  return kp[2] >= score_thresh ? 1 : 0;
}

__device__ __forceinline__ int decimal_digits(long long id) {
  int n = 1;
  for (long long p = 10; p <= id; p *= 10) ++n;
  return n;
}

__global__ __launch_bounds__(THREADS) void overlay_raster_kernel(const int* __restrict__ frame_index, const double* __restrict__ boxes,
                                                                 const long long* __restrict__ ids, const double* __restrict__ keypoints,
                                                                 const int* __restrict__ skeleton, const unsigned char* __restrict__ font,
                                                                 int* __restrict__ status, unsigned* __restrict__ keys, int row0,
                                                                 DrawParams P) {
  const int row = row0 + blockIdx.y;
  const int prim = blockIdx.x;
  const bool lead = threadIdx.x == 0 && blockIdx.z == 0;
  const int first = blockIdx.z * THREADS + threadIdx.x, stride = THREADS * SLICES;  // this thread's pixels of the bounding box
  const int f = frame_index[row];
  if (f < 0 || f >= P.F) {
    if (lead && prim == 0 && P.f0 == 0) atomicOr(&status[row], STATUS_FRAME);
    return;
  }
  if (f < P.f0 || f >= P.f1) return;  // another chunk's row
  long long id = 0;
  if (ids) {
    id = ids[row];
    if (id < 0 || id >= ID_END) {
      if (lead && prim == 0) atomicOr(&status[row], STATUS_SKIPPED);
      return;
    }
  }
  unsigned* Kf = keys + (size_t)(f - P.f0) * P.W * P.H;
  const unsigned key0 = ((unsigned)row << 2) + 1u;
  int flags = 0;

  if (prim < 5) {
    // ---- the box: edges 0..3 and the label ------------------------------------------------------------------------------------------
    if (!boxes) return;
    const Corners c = box_corners(boxes + 4 * (size_t)row, P.box_format);
    if (!c.ok) {
      if (lead) atomicOr(&status[row], STATUS_SKIPPED);
      return;
    }
    if (prim < 4) {
      const double ex0 = (prim == 0 || prim == 3) ? c.x1 : c.x2, ey0 = prim < 2 ? c.y1 : c.y2;
      const double ex1 = prim < 2 ? c.x2 : c.x1, ey1 = (prim == 0 || prim == 3) ? c.y1 : c.y2;
      // top (x1,y1)->(x2,y1), right (x2,y1)->(x2,y2), bottom (x2,y2)->(x1,y2), left (x1,y2)->(x1,y1)
      if (beyond_guard(ex0) || beyond_guard(ey0) || beyond_guard(ex1) || beyond_guard(ey1)) {
        if (lead) atomicOr(&status[row], STATUS_GUARD);
        return;
      }
      const int ax = quantise(ex0), ay = quantise(ey0), bx = quantise(ex1), by = quantise(ey1);
      const int r = SUB_HALF * P.thickness;
      int x0, x1, y0, y1;
      centre_span(min(ax, bx) - r, max(ax, bx) + r, P.W, x0, x1);
      centre_span(min(ay, by) - r, max(ay, by) + r, P.H, y0, y1);
      if (x1 < x0 || y1 < y0) return;
      const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);
      for (int t = first; t < n; t += stride) {
        const int x = x0 + t % bw, y = y0 + t / bw;
        if (segment_covers(ax, ay, bx, by, pixel_centre(x), pixel_centre(y), P.thickness))
          atomicMax(Kf + (size_t)y * P.W + x, key0 + LEVEL_BOX);
      }
      return;
    }
    if (!ids) return;
    if (beyond_guard(c.x1) || beyond_guard(c.y1)) {
      if (lead) atomicOr(&status[row], STATUS_GUARD);
      return;
    }
    const int nd = decimal_digits(id), s = P.label_scale;
    const int lw = CELL_W * s * nd, lh = CELL_H * s;
    if (lw > P.W || lh > P.H) return;  // larger than the frame: no label
    const int X0 = min(max(quantise(c.x1) >> SUB_BITS, 0), P.W - lw);
    const int Y0 = min(max((quantise(c.y1) >> SUB_BITS) - lh, 0), P.H - lh);
    for (int t = first; t < lw * lh; t += stride) {
      const int u = t % lw, v = t / lw;
      const int cell = u / (CELL_W * s), gx = (u % (CELL_W * s)) / s - 1, gy = v / s - 1;  // the glyph sits at columns 1..5, rows 1..7
      long long q = id;
      for (int j = nd - 1; j > cell; --j) q /= 10;
      const int digit = (int)(q % 10);
      const bool ink = gx >= 0 && gx < GLYPH_W && gy >= 0 && gy < GLYPH_H && ((font[digit * GLYPH_H + gy] >> (GLYPH_W - 1 - gx)) & 1);
      atomicMax(Kf + (size_t)(Y0 + v) * P.W + (X0 + u), key0 + (ink ? LEVEL_TEXT : LEVEL_LABEL));
    }
    return;
  }

  // ---- the pose: limbs, then discs ------------------------------------------------------------------------------------------------------
  if (!keypoints) return;
  const double* kp = keypoints + (size_t)row * P.K * P.D;
  if (prim < 5 + P.L) {
    const int ia = skeleton[2 * (prim - 5)], ib = skeleton[2 * (prim - 5) + 1];
    if (ia < 0 || ia >= P.K || ib < 0 || ib >= P.K) return;  // (the host refuses such a table)
    const double* pa = kp + (size_t)ia * P.D;
    const double* pb = kp + (size_t)ib * P.D;
    const int sa = keypoint_state(pa, P.D, P.score_thresh), sb = keypoint_state(pb, P.D, P.score_thresh);
    if (sa == 2 || sb == 2) flags |= STATUS_SKIPPED;
    if (sa != 1 || sb != 1) {
      if (lead && flags) atomicOr(&status[row], flags);
      return;
    }
    if (beyond_guard(pa[0]) || beyond_guard(pa[1]) || beyond_guard(pb[0]) || beyond_guard(pb[1])) {
      if (lead) atomicOr(&status[row], STATUS_GUARD);
      return;
    }
    const int ax = quantise(pa[0]), ay = quantise(pa[1]), bx = quantise(pb[0]), by = quantise(pb[1]);
    const int r = SUB_HALF * P.thickness;
    int x0, x1, y0, y1;
    centre_span(min(ax, bx) - r, max(ax, bx) + r, P.W, x0, x1);
    centre_span(min(ay, by) - r, max(ay, by) + r, P.H, y0, y1);
    if (x1 < x0 || y1 < y0) return;
    const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);
    for (int t = first; t < n; t += stride) {
      const int x = x0 + t % bw, y = y0 + t / bw;
      if (segment_covers(ax, ay, bx, by, pixel_centre(x), pixel_centre(y), P.thickness))
        atomicMax(Kf + (size_t)y * P.W + x, key0 + LEVEL_POSE);
    }
    return;
  }
  const int k = prim - 5 - P.L;
  if (k >= P.K) return;
  const double* pk = kp + (size_t)k * P.D;
  const int sk = keypoint_state(pk, P.D, P.score_thresh);
  if (sk != 1) {
    if (lead && sk == 2) atomicOr(&status[row], STATUS_SKIPPED);
    return;
  }
  if (beyond_guard(pk[0]) || beyond_guard(pk[1])) {
    if (lead) atomicOr(&status[row], STATUS_GUARD);
    return;
  }
  const int kx = quantise(pk[0]), ky = quantise(pk[1]);
  const int r = SUB_ONE * P.radius;
  int x0, x1, y0, y1;
  centre_span(kx - r, kx + r, P.W, x0, x1);
  centre_span(ky - r, ky + r, P.H, y0, y1);
  if (x1 < x0 || y1 < y0) return;
  const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);
  for (int t = first; t < n; t += stride) {
    const int x = x0 + t % bw, y = y0 + t / bw;
    if (disc_covers(kx, ky, pixel_centre(x), pixel_centre(y), P.radius)) atomicMax(Kf + (size_t)y * P.W + x, key0 + LEVEL_POSE);
  }
}

__device__ __forceinline__ unsigned char blend(int alpha, int colour, int pixel) {
  return (unsigned char)((alpha * colour + (255 - alpha) * pixel + 127) / 255);
}

__global__ __launch_bounds__(THREADS) void overlay_resolve_kernel(unsigned char* __restrict__ frames, unsigned* __restrict__ keys,
                                                                  const long long* __restrict__ ids,
                                                                  const unsigned char* __restrict__ palette, int n_palette, int text0,
                                                                  int text1, int text2, int alpha, size_t pixel0, size_t n_pixels) {
  const size_t t = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (t >= n_pixels) return;
  const unsigned key = keys[t];
  if (key == 0u) return;
  keys[t] = 0u;
  const unsigned row = (key - 1u) >> 2, level = (key - 1u) & 3u;
  int c0 = text0, c1 = text1, c2 = text2;
  if (level != (unsigned)LEVEL_TEXT) {
    const unsigned char* col = palette + 3 * (ids ? (int)(ids[row] % n_palette) : 0);
    c0 = col[0], c1 = col[1], c2 = col[2];
  }
  unsigned char* px = frames + (pixel0 + t) * 3;
  px[0] = blend(alpha, c0, px[0]);
  px[1] = blend(alpha, c1, px[1]);
  px[2] = blend(alpha, c2, px[2]);
}

}  // namespace

extern "C" size_t pmce_overlay_workspace_bytes(int width, int height, int chunk_frames) {
  if (width < 1 || height < 1 || width > MAX_DIM || height > MAX_DIM || chunk_frames < 1) {
    pmce_set_error("overlay_workspace_bytes: 1 <= width, height <= %d, chunk_frames >= 1 (got %d, %d, %d)", MAX_DIM, width, height,
                   chunk_frames);
    return 0;
  }
  return (size_t)chunk_frames * width * height * sizeof(unsigned);
}

extern "C" int pmce_draw_overlays(unsigned char* frames, int n_frames, int width, int height, const int* frame_index_host, const int* frame_index,
                                  const double* boxes, int box_format, const long long* ids, const double* keypoints, int n_keypoints, int keypoint_dim,
                                  const int* skeleton, int n_limbs, double score_thresh, int thickness, int radius, int label_scale,
                                  const unsigned char* font, const unsigned char* palette, int n_palette, const unsigned char* text_color,
                                  int alpha, int n_rows, int* status, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const char* what = "draw_overlays";
  const int F = n_frames, W = width, H = height, N = n_rows, K = keypoints ? n_keypoints : 0, L = keypoints ? n_limbs : 0;
  PMCE_REQUIRE(W >= 1 && H >= 1 && W <= MAX_DIM && H <= MAX_DIM, "%s: width and height must be in 1..%d (got %d x %d)", what, MAX_DIM, W, H);
  PMCE_REQUIRE(F >= 0 && N >= 0, "%s: negative size (frames %d, rows %d)", what, F, N);
  PMCE_REQUIRE(N < (1 << 30), "%s: at most 2^30 - 1 rows (got %d)", what, N);
  PMCE_REQUIRE(box_format >= BOX_XYXY && box_format <= BOX_XYWH, "%s: box_format must be 0 (xyxy), 1 (cxcywh) or 2 (xywh) (got %d)", what,
               box_format);
  PMCE_REQUIRE(thickness >= 1 && thickness <= MAX_THICKNESS, "%s: thickness must be in 1..%d (got %d)", what, MAX_THICKNESS, thickness);
  PMCE_REQUIRE(radius >= 1 && radius <= MAX_RADIUS, "%s: radius must be in 1..%d (got %d)", what, MAX_RADIUS, radius);
  PMCE_REQUIRE(label_scale >= 1 && label_scale <= 64, "%s: label_scale must be in 1..64 (got %d)", what, label_scale);
  PMCE_REQUIRE(alpha >= 0 && alpha <= 255, "%s: alpha must be in 0..255 (got %d)", what, alpha);
  PMCE_REQUIRE(n_palette >= 1, "%s: the palette needs a colour (got %d)", what, n_palette);
  PMCE_REQUIRE(!keypoints || (n_keypoints >= 1 && n_keypoints <= 4096 && (keypoint_dim == 2 || keypoint_dim == 3) && n_limbs >= 0 &&
                              n_limbs <= 16384 && (skeleton || n_limbs == 0)),
               "%s: keypoints need 1..4096 points of 2 or 3 components and at most 16384 limbs (got %d, %d, %d)", what, n_keypoints,
               keypoint_dim, n_limbs);
  PMCE_REQUIRE(score_thresh == score_thresh, "%s: score_thresh is not a number", what);
  if (N == 0) return PMCE_OK;
  PMCE_REQUIRE(F >= 1, "%s: %d rows but no frame", what, N);
  PMCE_REQUIRE(frames && frame_index && font && palette && text_color && status && workspace, "%s: null pointer", what);
  const size_t per_frame = (size_t)W * H * sizeof(unsigned);
  if (workspace_bytes < per_frame) {
    pmce_set_error("%s: workspace of %zu bytes, %zu needed for one frame per chunk (pmce_overlay_workspace_bytes)", what, workspace_bytes,
                   per_frame);
    return PMCE_ERR_WORKSPACE;
  }
  PMCE_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: the workspace must be 4-byte aligned", what);
  if (frame_index_host)
    for (int i = 0; i < N; ++i)
      PMCE_REQUIRE(frame_index_host[i] >= 0 && frame_index_host[i] < F && (i == 0 || frame_index_host[i - 1] <= frame_index_host[i]),
                   "%s: frame_index_host must be ascending and inside 0..%d (row %d: %d)", what, F - 1, i, frame_index_host[i]);
  const int chunk = (int)std::min<size_t>(workspace_bytes / per_frame, (size_t)F);
  unsigned* keys = static_cast<unsigned*>(workspace);

  if (hipMemsetAsync(status, 0, (size_t)N * sizeof(int), stream) != hipSuccess ||
      hipMemsetAsync(keys, 0, (size_t)chunk * per_frame, stream) != hipSuccess) {
    pmce_set_error("%s: hipMemsetAsync failed", what);
    return PMCE_ERR_LAUNCH;
  }
  DrawParams P{};
  P.F = F, P.W = W, P.H = H;
  P.box_format = box_format, P.K = K, P.D = keypoint_dim, P.L = L;
  P.score_thresh = score_thresh;
  P.thickness = thickness, P.radius = radius, P.label_scale = label_scale;
  const int prims = 5 + L + K;
  for (int f0 = 0; f0 < F; f0 += chunk) {
    P.f0 = f0, P.f1 = std::min(F, f0 + chunk);
    // the chunk's rows: a slice of the sorted host table, or - frame_index known on the device alone - all rows, of which the kernel
    // skips those of other chunks
    const int lo = frame_index_host ? (int)(std::lower_bound(frame_index_host, frame_index_host + N, P.f0) - frame_index_host) : 0;
    const int hi = frame_index_host ? (int)(std::lower_bound(frame_index_host, frame_index_host + N, P.f1) - frame_index_host) : N;
    for (int r0 = lo; r0 < hi; r0 += 65535)  // grid.y carries the row
      hipLaunchKernelGGL(overlay_raster_kernel, dim3(prims, std::min(65535, hi - r0), SLICES), dim3(THREADS), 0, stream, frame_index, boxes,
                         ids, keypoints, skeleton, font, status, keys, r0, P);
    const size_t n_pixels = (size_t)(P.f1 - f0) * W * H;
    hipLaunchKernelGGL(overlay_resolve_kernel, dim3((unsigned)((n_pixels + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, frames, keys,
                       ids, palette, n_palette, (int)text_color[0], (int)text_color[1], (int)text_color[2], alpha, (size_t)f0 * W * H,
                       n_pixels);
    PMCE_TRY(pmce_check_launch(what));
  }
  return PMCE_OK;
}
