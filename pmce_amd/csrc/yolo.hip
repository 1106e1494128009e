// The detector's operators besides the convolution (YOLOv3 at the tracker's settings, main/run_demo.py:199-215 of the reference; the
// structure is the published yolov3.cfg's): the letterbox that makes the network's square input from video frames, the nearest x2
// upsample that writes into a channel slice of a concatenation buffer, and the decoding of the three detection maps into box rows.
// All three are element-wise: a result depends on its own image only and has the same bits whatever n is.
#include "common.hpp"

namespace {

constexpr int YOLO_SCALES = 3, YOLO_ANCHORS = 3;

// out[img][2 y + dy][2 x + dx][c_off .. c_off + C) = x[img][y][x][0 .. C): a thread moves 16 bytes of one output pixel.
__global__ __launch_bounds__(256) void upsample2x_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ out, long long ldo,
                                                          int n, int H, int W, int C) {
  const int c4 = C >> 2, OW = 2 * W, OH = 2 * H;
  const long long total = (long long)n * OH * OW * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % c4);
    long long t = i / c4;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    const long long img = t / OH;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((img * H + (oy >> 1)) * W + (ox >> 1)) * ldx + 4 * c);
    *reinterpret_cast<f32x4*>(out + ((img * OH + oy) * OW + ox) * ldo + 4 * c) = v;
  }
}

struct DecodeParams {
  const float* map[YOLO_SCALES];  // NHWC [n][g][g][pitch], channel a (5 + nc) + c
  long long pitch[YOLO_SCALES];
  int g[YOLO_SCALES];
  float stride[YOLO_SCALES];                // S / g
  float anchor[YOLO_SCALES][YOLO_ANCHORS][2];  // (w, h) / stride, the division done on the host in fp32
  long long row0[YOLO_SCALES + 1];          // first row of a scale; row0[3] = R
  int n, nc;
  float* out;  // [n][R][5 + nc]
};

// The logistic function and the exponential, correctly rounded to fp32 (evaluated in fp64, rounded once).
__device__ __forceinline__ float sigmoid_cr(float t) { return (float)(1.0 / (1.0 + exp(-(double)t))); }
__device__ __forceinline__ float exp_cr(float t) { return (float)exp((double)t); }

// One thread per output float, adjacent threads adjacent floats of a row (and adjacent channels of the map).
__global__ __launch_bounds__(256) void yolo_decode_kernel(DecodeParams p) {
#pragma clang fp contract(off)
  const int E = 5 + p.nc;
  const long long R = p.row0[YOLO_SCALES], total = (long long)p.n * R * E;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % E);
    long long t = i / E;
    const long long row = t % R, img = t / R;
    const int s = row >= p.row0[2] ? 2 : row >= p.row0[1] ? 1 : 0;
    const int g = p.g[s];
    int r = (int)(row - p.row0[s]);
    const int a = r / (g * g);
    r -= a * g * g;
    const int gy = r / g, gx = r - gy * g;
    const float v = p.map[s][((img * g + gy) * g + gx) * p.pitch[s] + a * E + c];
    const float stride = p.stride[s];
    float o;
    if (c == 0) o = (sigmoid_cr(v) + (float)gx) * stride;
    else if (c == 1) o = (sigmoid_cr(v) + (float)gy) * stride;
    else if (c == 2 || c == 3) o = (exp_cr(v) * p.anchor[s][a][c - 2]) * stride;
    else o = sigmoid_cr(v);
    p.out[i] = o;
  }
}

// job -> frames[frame_index[job]] padded to a square of side L = max(H, W) and sampled at S x S as F.interpolate(mode="nearest") samples:
// src = min((int)floorf(dst * scale), L - 1), scale = (float)L / S.  A thread writes the three channels of one output pixel.
__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* __restrict__ frames, int n_frames, int H, int W,
                                                         const int* __restrict__ frame_index, int n, int S, int pad_x, int pad_y, int L,
                                                         float scale, int swap_rb, const float* __restrict__ table, float pad_value,
                                                         float* __restrict__ out) {
  const long long plane = (long long)S * S, total = (long long)n * plane;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long job = i / plane;
    const int r = (int)(i - job * plane), oy = r / S, ox = r - oy * S;
    const int y = min((int)floorf((float)oy * scale), L - 1) - pad_y, x = min((int)floorf((float)ox * scale), L - 1) - pad_x;
    const int f = frame_index[job];
    float v[3] = {pad_value, pad_value, pad_value};
    if ((unsigned)f < (unsigned)n_frames && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
      const unsigned char* px = frames + (((long long)f * H + y) * W + x) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = table[px[swap_rb ? 2 - c : c]];
    }
    float* o = out + job * 3 * plane + r;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = v[c];
  }
}

unsigned grid_for(long long total) {
  const long long blocks = (total + 255) / 256;
  return (unsigned)(blocks < 65536 ? (blocks < 1 ? 1 : blocks) : 65536);
}

}  // namespace

extern "C" int pmce_upsample2x_nhwc_f32(const float* x, long long in_pitch, float* out, long long out_pitch, int n, int H, int W, int C,
                                        hipStream_t stream) {
  PMCE_REQUIRE(x && out, "upsample2x: null pointer");
  PMCE_REQUIRE(n >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && H <= 16384 && W <= 16384,
               "upsample2x: need n, H, W >= 1 (H, W <= 16384) and C %% 4 == 0 (n=%d H=%d W=%d C=%d)", n, H, W, C);
  PMCE_REQUIRE(in_pitch >= C && out_pitch >= C && in_pitch % 4 == 0 && out_pitch % 4 == 0 && in_pitch < (1ll << 24) && out_pitch < (1ll << 24),
               "upsample2x: the pitches must be multiples of 4 in C..2^24 (C=%d in=%lld out=%lld)", C, in_pitch, out_pitch);
  PMCE_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
               "upsample2x: the buffers (the slice's first channel included) must be 16-byte aligned");
  hipLaunchKernelGGL(upsample2x_kernel, dim3(grid_for((long long)n * 4 * H * W * (C / 4))), dim3(256), 0, stream, x, in_pitch, out, out_pitch,
                     n, H, W, C);
  return pmce_check_launch("upsample2x_nhwc_f32");
}

extern "C" int pmce_yolo_decode_f32(const float* map0, const float* map1, const float* map2, const long long* pitches_host,
                                    const int* grids_host, const float* anchors_host, int n, int nc, int S, float* out, hipStream_t stream) {
  PMCE_REQUIRE(map0 && map1 && map2 && pitches_host && grids_host && anchors_host && out, "yolo_decode: null pointer");
  PMCE_REQUIRE(n >= 1 && nc >= 1 && nc <= 255 && S >= 1 && S <= 16384, "yolo_decode: need n >= 1, nc in 1..255, S in 1..16384 (n=%d nc=%d S=%d)", n,
               nc, S);
  DecodeParams p{};
  const float* maps[YOLO_SCALES] = {map0, map1, map2};
  const int E = 5 + nc;
  long long rows = 0;
  for (int s = 0; s < YOLO_SCALES; ++s) {
    const int g = grids_host[s];
    PMCE_REQUIRE(g >= 1 && g <= 2048, "yolo_decode: grid %d must be in 1..2048 (got %d)", s, g);
    PMCE_REQUIRE(pitches_host[s] >= YOLO_ANCHORS * E && pitches_host[s] < (1ll << 24),
                 "yolo_decode: the pitch of map %d must be in %d..2^24 (got %lld)", s, YOLO_ANCHORS * E, pitches_host[s]);
    p.map[s] = maps[s];
    p.pitch[s] = pitches_host[s];
    p.g[s] = g;
    p.stride[s] = (float)S / (float)g;
    for (int a = 0; a < YOLO_ANCHORS; ++a)
      for (int k = 0; k < 2; ++k) {
        const float v = anchors_host[(s * YOLO_ANCHORS + a) * 2 + k];
        PMCE_REQUIRE(v > 0.f && v < 1e6f, "yolo_decode: anchor %d of map %d must be positive and finite", a, s);
        p.anchor[s][a][k] = v / p.stride[s];
      }
    p.row0[s] = rows;
    rows += (long long)YOLO_ANCHORS * g * g;
  }
  p.row0[YOLO_SCALES] = rows;
  PMCE_REQUIRE((long long)n * rows * E < (1ll << 40), "yolo_decode: the result is too large (%lld rows per image; split the batch)", rows);
  p.n = n; p.nc = nc; p.out = out;
  hipLaunchKernelGGL(yolo_decode_kernel, dim3(grid_for((long long)n * rows * E)), dim3(256), 0, stream, p);
  return pmce_check_launch("yolo_decode_f32");
}

extern "C" int pmce_letterbox_u8_f32(const unsigned char* frames, int n_frames, int height, int width, const int* frame_index_host,
                                     const int* frame_index, int n_jobs, int S, int swap_rb, const float* table, float pad_value, float* out,
                                     hipStream_t stream) {
  PMCE_REQUIRE(frames && frame_index && table && out, "letterbox: null pointer");
  PMCE_REQUIRE(n_frames >= 1 && n_jobs >= 1 && height >= 1 && width >= 1 && height <= 16384 && width <= 16384 && S >= 1 && S <= 4096,
               "letterbox: need n_frames, n_jobs >= 1, height and width in 1..16384, S in 1..4096 (n_frames=%d n_jobs=%d %d x %d S=%d)", n_frames,
               n_jobs, width, height, S);
  PMCE_REQUIRE(pad_value == pad_value, "letterbox: pad_value is NaN");
  if (frame_index_host)
    for (int i = 0; i < n_jobs; ++i)
      PMCE_REQUIRE(frame_index_host[i] >= 0 && frame_index_host[i] < n_frames, "letterbox: frame_index[%d] = %d, there are %d frames", i,
                   frame_index_host[i], n_frames);
  const int L = height > width ? height : width;
  hipLaunchKernelGGL(letterbox_kernel, dim3(grid_for((long long)n_jobs * S * S)), dim3(256), 0, stream, frames, n_frames, height, width, frame_index,
                     n_jobs, S, (L - width) / 2, (L - height) / 2, L, (float)L / (float)S, swap_rb ? 1 : 0, table, pad_value, out);
  return pmce_check_launch("letterbox_u8_f32");
}
