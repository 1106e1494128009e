// Mesh overlays of the reference's demo, on device: a batched triangle rasteriser with a z-buffer, smooth shading and the demo's
// compositing rule.  A JOB is one person in one frame.
//
// What is restated (reference kasvii/PMCE):
//   * demo/renderer.py:28-35 WeakPerspectiveCamera.get_projection_matrix, :65-66 the flip by Rx(180 deg), :76-78 the optional rotation
//     (applied to the flipped mesh), :102 camera pose identity, :111-113 the compositing (covered pixels take the rendering, every other
//     pixel keeps the image), :51-59,94 ambient 0.3, two directional lights of intensity 1.2, emissive 0.1;
//   * main/run_demo.py:402-415: the persons of a frame are drawn one after another, each over the previous one's result.
// With the flip, P and the vertical flip of the read-back image, a vertex q = Rx R Rx p of the model's frame lands, in a pixel grid with
// its origin at the top-left corner, x right and y down, at
//     u = (sx (q.x + tx) + 1) W / 2        v = (sy (q.y + ty) + 1) H / 2        z_ndc = q.z   (smaller = nearer)
// What OpenGL fixes: samples at pixel centres, one sample per pixel, a fragment survives for -1 <= z_ndc <= 1, GL_LESS, back faces
// culled (single-sided material).  Ours: the top-left fill rule on coordinates snapped to 1/256 px, and the shading formula.
//
// Three stages, every one a plain launch on the caller's stream:
//   vertex   one lane per vertex of a job: rotate, project in fp64, snap to int32 fixed point (8 sub-pixel bits), the vertex normal as
//            the normalised sum of the incident faces' cross products, gathered through a vertex -> face CSR in fixed order (no float
//            atomics: the picture must not depend on arrival order); the job's extent as an integer min / max, its status word.
//   raster   GROUP = 8 adjacent lanes per triangle: integer setup, culling from the sign of the integer area, bounding box clipped to the
//            frame.  A box at most 8 pixels wide and 32 high is walked row by row by its group, a lane per column, with incremental int64
//            edge functions - the fragments of a row leave in one wave instruction as neighbouring keys; a larger one is handed to the
//            whole wave, which sweeps it in 8 x 8 blocks (a close-up, or a triangle larger than the frame, costs one wave its sweep and
//            nobody else anything).  Every covered, unclipped pixel: ONE 64-bit atomic min of (order-preserving bits of z) << 32 | face.
//            Min commutes, so the nearest fragment wins, equal z goes to the lowest face index, and the result is the same bits every run.
//   resolve  over the job's rectangle: decode the face, recompute the barycentrics, shade, write the pixel (and face_id / depth), and
//            put the key back to "empty" - the buffer serves the next layer without a clearing pass.
// Persons of a frame are LAYERS: launch l draws the l-th person of every frame that has one, so ordered compositing needs no protocol
// between workgroups.  order = depth rasterises every layer into the same keys first (the face word then carries layer * n_faces + face)
// and resolves afterwards.
//
// Sizing.  The atomic rate of 64-bit integer min on this chip has not been measured; the stand-in is the float-atomic figure (1.3 TB/s
// for 256 contiguous bytes per wave instruction, 17 x less for 64 lanes in 64 rows).  A person at 1920 x 1080 covers ~1e5 pixels at depth
// complexity ~1.2 after culling: ~1 MB of keys per job, 2400 jobs ~2.4 GB -> 2 ms at the contiguous rate, ~30 ms at the scattered one.
// scripts/bench_render.py measures what it is.
#include "common.hpp"

#include <math.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int FIX_BITS = 8;
constexpr int FIX_ONE = 1 << FIX_BITS;
constexpr int FIX_HALF = FIX_ONE / 2;
constexpr int GUARD_FIX = (1 << 14) * FIX_ONE;  // +-2^14 px
constexpr int SNAP_SAT = 1 << 30;               // what a coordinate beyond every bound is stored as
constexpr int MAX_DIM = 8192;
constexpr int MAX_LIGHTS = 8;
constexpr int GROUP = 8;            // lanes per triangle in the raster stage
constexpr int GROUP_MAX_ROWS = 32;  // a bounding box wider than GROUP or higher than this is swept by the whole wave
constexpr int STATUS_NONFINITE = 1;
constexpr int STATUS_GUARD = 2;
constexpr unsigned long long KEY_EMPTY = ~0ull;
constexpr int VERT_THREADS = 256;
constexpr int RASTER_THREADS = 256;
constexpr int TILE_W = 64, TILE_H = 4;  // one wave = 64 consecutive pixels of a row
constexpr int RECT_WGS = 64;            // workgroups that share a job's rectangle

struct ShadeParams {
  float base[3];
  float emissive, ambient, light_scale;  // light_scale = intensity / pi
  int n_lights;
  float lights[MAX_LIGHTS][3];
};

struct JobInfo {
  int minx, miny, maxx, maxy;  // extent of the in-guard vertices, fixed point
};

struct VertRec {
  float z, nx, ny, nz;
};

// pixel columns (rows) whose centres lie in [lo, hi] fixed point, clipped to [0, n - 1]
__device__ __forceinline__ void centre_span(int lo, int hi, int n, int& p0, int& p1) {
  p0 = max(0, (lo + FIX_HALF - 1) >> FIX_BITS);
  p1 = min(n - 1, (hi - FIX_HALF) >> FIX_BITS);
}

struct Rect {
  int x0, y0, x1, y1;  // inclusive; empty when x1 < x0 or y1 < y0
};
__device__ __forceinline__ Rect job_rect(const JobInfo& ji, int W, int H) {
  Rect r;
  if (ji.minx > ji.maxx) return Rect{0, 0, -1, -1};
  centre_span(ji.minx, ji.maxx, W, r.x0, r.x1);
  centre_span(ji.miny, ji.maxy, H, r.y0, r.y1);
  return r;
}

// q = Rx R Rx p: the reference's rotation acts on the flipped mesh, and the flip is undone by the projection
__device__ __forceinline__ void rotate_vertex(const float* __restrict__ R, const float* __restrict__ p, float q[3]) {
#pragma clang fp contract(off)
  if (!R) {
    q[0] = p[0], q[1] = p[1], q[2] = p[2];
    return;
  }
  const float x = p[0], y = -p[1], z = -p[2];
  q[0] = (R[0] * x + R[1] * y) + R[2] * z;
  q[1] = -((R[3] * x + R[4] * y) + R[5] * z);
  q[2] = -((R[6] * x + R[7] * y) + R[8] * z);
}

__device__ __forceinline__ bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

__device__ __forceinline__ int snap(double u) {
  const double s = rint(u * (double)FIX_ONE);
  return (int)fmin(fmax(s, -(double)SNAP_SAT), (double)SNAP_SAT);
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(VERT_THREADS) void render_init_kernel(JobInfo* __restrict__ info, int* __restrict__ status, int N) {
  const int j = blockIdx.x * VERT_THREADS + threadIdx.x;
  if (j >= N) return;
  info[j] = JobInfo{INT_MAX, INT_MAX, INT_MIN, INT_MIN};
  status[j] = 0;
}

__global__ __launch_bounds__(VERT_THREADS) void render_vertex_kernel(const float* __restrict__ verts, const float* __restrict__ cams,
                                                                     const float* __restrict__ rot, const int* __restrict__ faces,
                                                                     const int* __restrict__ vf_off, const int* __restrict__ vf_face,
                                                                     int2* __restrict__ xy_ws, VertRec* __restrict__ rec_ws,
                                                                     int* __restrict__ xy_out, JobInfo* __restrict__ info,
                                                                     int* __restrict__ status, int V, int W, int H) {
#pragma clang fp contract(off)
  const int job = blockIdx.y;
  const int v = blockIdx.x * VERT_THREADS + threadIdx.x;
  const float* P = verts + (size_t)job * V * 3;
  const float* R = rot ? rot + (size_t)job * 9 : nullptr;
  const float* cam = cams + (size_t)job * 4;
  bool bad = false;
  int fx = 0, fy = 0;
  bool in_guard = false;
  if (v < V) {
    bad = !(isfinite(cam[0]) && isfinite(cam[1]) && isfinite(cam[2]) && isfinite(cam[3])) || !finite3(P + 3 * (size_t)v);
    if (R)
      for (int i = 0; i < 9; ++i) bad |= !isfinite(R[i]);
    float q[3];
    rotate_vertex(R, P + 3 * (size_t)v, q);
    VertRec rec{q[2], 0.f, 0.f, 0.f};
    if (!bad) {
      const double u = ((double)cam[0] * ((double)q[0] + (double)cam[2]) + 1.0) * (0.5 * W);
      const double w = ((double)cam[1] * ((double)q[1] + (double)cam[3]) + 1.0) * (0.5 * H);
      fx = snap(u), fy = snap(w);
      in_guard = abs(fx) <= GUARD_FIX && abs(fy) <= GUARD_FIX;
      // the vertex normal: incident faces in the CSR's order, un-normalised cross products (area-weighted)
      float n0 = 0.f, n1 = 0.f, n2 = 0.f;
      for (int e = vf_off[v]; e < vf_off[v + 1]; ++e) {
        const int f = vf_face[e];
        float a[3], b[3], c[3];
        rotate_vertex(R, P + 3 * (size_t)faces[3 * f + 0], a);
        rotate_vertex(R, P + 3 * (size_t)faces[3 * f + 1], b);
        rotate_vertex(R, P + 3 * (size_t)faces[3 * f + 2], c);
        const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
        const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
        n0 += e1y * e2z - e1z * e2y;
        n1 += e1z * e2x - e1x * e2z;
        n2 += e1x * e2y - e1y * e2x;
      }
      const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
      if (len > 0.f && isfinite(len)) rec.nx = n0 / len, rec.ny = n1 / len, rec.nz = n2 / len;
    }
    xy_ws[(size_t)job * V + v] = make_int2(fx, fy);
    rec_ws[(size_t)job * V + v] = rec;
    if (xy_out) {
      xy_out[((size_t)job * V + v) * 2 + 0] = fx;
      xy_out[((size_t)job * V + v) * 2 + 1] = fy;
    }
  }
  // the job's extent and status: one reduction per wave, then integer atomics (order-independent)
  const int mnx = wave_min_i(in_guard ? fx : INT_MAX), mny = wave_min_i(in_guard ? fy : INT_MAX);
  const int mxx = wave_max_i(in_guard ? fx : INT_MIN), mxy = wave_max_i(in_guard ? fy : INT_MIN);
  const bool any_bad = __ballot(bad) != 0ull;
  if ((threadIdx.x & 63) == 0) {
    if (mnx <= mxx) {
      atomicMin(&info[job].minx, mnx);
      atomicMin(&info[job].miny, mny);
      atomicMax(&info[job].maxx, mxx);
      atomicMax(&info[job].maxy, mxy);
    }
    if (any_bad) atomicOr(&status[job], STATUS_NONFINITE);
  }
}

// ---- triangle setup, shared by raster and resolve --------------------------------------------------------------------------------
struct Tri {
  int ax, ay, bx, by, cx, cy;  // fixed point, wound so that the area is positive
  int ia, ib, ic;              // the vertices in that order
  long long area;              // > 0
};

// false: nothing to draw (guard band, zero area, culled).  guard is set when a vertex lies beyond the guard band.
__device__ __forceinline__ bool tri_setup(const int* __restrict__ faces, const int2* __restrict__ xy, int f, bool cull, Tri& t, bool& guard) {
  int ia = faces[3 * f + 0], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  const int2 a = xy[ia], b = xy[ib], c = xy[ic];
  guard = abs(a.x) > GUARD_FIX || abs(a.y) > GUARD_FIX || abs(b.x) > GUARD_FIX || abs(b.y) > GUARD_FIX || abs(c.x) > GUARD_FIX ||
          abs(c.y) > GUARD_FIX;
  if (guard) return false;
  // the winding normal's z in the model's frame; negative = towards the camera = front face
  const long long area = (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
  if (area == 0 || (cull && area > 0)) return false;
  t.ax = a.x, t.ay = a.y, t.ia = ia;
  if (area < 0) {  // swap b and c: positive area
    t.bx = c.x, t.by = c.y, t.ib = ic;
    t.cx = b.x, t.cy = b.y, t.ic = ib;
    t.area = -area;
  } else {
    t.bx = b.x, t.by = b.y, t.ib = ib;
    t.cx = c.x, t.cy = c.y, t.ic = ic;
    t.area = area;
  }
  return true;
}

// Edge function of p0 -> p1 at s: positive inside for a positive-area triangle.  A sample ON the edge belongs to the triangle when the
// edge is a left edge (dy < 0: the interior lies at larger x) or a top edge (dy == 0, dx > 0: the interior lies below, y runs down).
__device__ __forceinline__ long long edge_at(int p0x, int p0y, int p1x, int p1y, int sx, int sy) {
  return (long long)(p1x - p0x) * (sy - p0y) - (long long)(p1y - p0y) * (sx - p0x);
}
__device__ __forceinline__ int edge_bias(int p0x, int p0y, int p1x, int p1y) {
  const int dx = p1x - p0x, dy = p1y - p0y;
  return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
}

// z of a fragment from the integer barycentrics: three products, two sums, one division, fp32
__device__ __forceinline__ float frag_z(long long ea, long long eb, long long ec, long long area, float za, float zb, float zc) {
#pragma clang fp contract(off)
  return (((float)ea * za + (float)eb * zb) + (float)ec * zc) / (float)area;
}

__device__ __forceinline__ unsigned z_order_bits(float z) {
  const unsigned u = __float_as_uint(z + 0.0f);  // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float z_from_bits(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__device__ __forceinline__ void emit(unsigned long long* __restrict__ keys, size_t pix, long long ea, long long eb, long long ec,
                                     long long area, float za, float zb, float zc, unsigned faceword) {
  const float z = frag_z(ea, eb, ec, area, za, zb, zc);
  if (!(z >= -1.0f && z <= 1.0f)) return;  // OpenGL's clip volume
  atomicMin(keys + pix, ((unsigned long long)z_order_bits(z) << 32) | faceword);
}

__global__ __launch_bounds__(RASTER_THREADS) void render_raster_kernel(const int* __restrict__ faces, const int2* __restrict__ xy_ws,
                                                                       const VertRec* __restrict__ rec_ws, const int* __restrict__ sched,
                                                                       const int* __restrict__ job_frame, int* __restrict__ status,
                                                                       unsigned long long* __restrict__ keys, int V, int NF, int W, int H,
                                                                       int frame0, unsigned face_base, int cull) {
  const int job = sched[blockIdx.y];
  if (status[job] & STATUS_NONFINITE) return;  // uniform over the workgroup
  const int lane = threadIdx.x & 63;
  const int sub = lane & (GROUP - 1);  // a GROUP of adjacent lanes shares a triangle: the lane's pixel column inside the box
  const int f = (blockIdx.x * RASTER_THREADS + threadIdx.x) / GROUP;
  const int2* xy = xy_ws + (size_t)job * V;
  const VertRec* rec = rec_ws + (size_t)job * V;
  unsigned long long* K = keys + (size_t)(job_frame[job] - frame0) * W * H;

  Tri t{};
  bool guard = false;
  bool live = f < NF && tri_setup(faces, xy, f, cull != 0, t, guard);
  if (__ballot(guard) != 0ull && lane == 0) atomicOr(&status[job], STATUS_GUARD);
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
  float za = 0.f, zb = 0.f, zc = 0.f;
  long long e0 = 0, e1 = 0, e2 = 0;              // biased edge functions at the centre of pixel (x0, y0): bc, ca, ab
  long long sx0 = 0, sx1 = 0, sx2 = 0, sy0 = 0, sy1 = 0, sy2 = 0;  // their steps per pixel in x and in y
  int b0 = 0, b1 = 0, b2 = 0;
  if (live) {
    centre_span(min(t.ax, min(t.bx, t.cx)), max(t.ax, max(t.bx, t.cx)), W, x0, x1);
    centre_span(min(t.ay, min(t.by, t.cy)), max(t.ay, max(t.by, t.cy)), H, y0, y1);
    live = x0 <= x1 && y0 <= y1;
  }
  if (live) {
    za = rec[t.ia].z, zb = rec[t.ib].z, zc = rec[t.ic].z;
    const int px = x0 * FIX_ONE + FIX_HALF, py = y0 * FIX_ONE + FIX_HALF;
    b0 = edge_bias(t.bx, t.by, t.cx, t.cy), b1 = edge_bias(t.cx, t.cy, t.ax, t.ay), b2 = edge_bias(t.ax, t.ay, t.bx, t.by);
    e0 = edge_at(t.bx, t.by, t.cx, t.cy, px, py) + b0;
    e1 = edge_at(t.cx, t.cy, t.ax, t.ay, px, py) + b1;
    e2 = edge_at(t.ax, t.ay, t.bx, t.by, px, py) + b2;
    sx0 = -(long long)(t.cy - t.by) * FIX_ONE, sy0 = (long long)(t.cx - t.bx) * FIX_ONE;
    sx1 = -(long long)(t.ay - t.cy) * FIX_ONE, sy1 = (long long)(t.ax - t.cx) * FIX_ONE;
    sx2 = -(long long)(t.by - t.ay) * FIX_ONE, sy2 = (long long)(t.bx - t.ax) * FIX_ONE;
  }
  const unsigned fw = face_base + (unsigned)f;
  const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
  const bool small = live && bw <= GROUP && bh <= GROUP_MAX_ROWS;
  const bool big = live && !small && sub == 0;  // one lane of the group hands the triangle to the wave

  if (small) {
    // the group walks the box row by row, lane `sub` on column x0 + sub: a row's fragments leave in ONE wave instruction, next to each other
    const int x = x0 + sub;
    long long c0 = e0 + sub * sx0, c1 = e1 + sub * sx1, c2 = e2 + sub * sx2;
    for (int y = y0; y <= y1; ++y) {
      if (x <= x1 && (c0 | c1 | c2) >= 0) emit(K, (size_t)y * W + x, c0 - b0, c1 - b1, c2 - b2, t.area, za, zb, zc, fw);
      c0 += sy0, c1 += sy1, c2 += sy2;
    }
  }

  // the large boxes, one after another, swept by the whole wave in 8 x 8 blocks
  unsigned long long todo = __ballot(big);
  const int lx = lane & 7, ly = lane >> 3;
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int X0 = __shfl(x0, src, 64), X1 = __shfl(x1, src, 64), Y0 = __shfl(y0, src, 64), Y1 = __shfl(y1, src, 64);
    const long long S0x = __shfl(sx0, src, 64), S1x = __shfl(sx1, src, 64), S2x = __shfl(sx2, src, 64);
    const long long S0y = __shfl(sy0, src, 64), S1y = __shfl(sy1, src, 64), S2y = __shfl(sy2, src, 64);
    const int B0 = __shfl(b0, src, 64), B1 = __shfl(b1, src, 64), B2 = __shfl(b2, src, 64);
    const float ZA = __shfl(za, src, 64), ZB = __shfl(zb, src, 64), ZC = __shfl(zc, src, 64);
    const long long A = __shfl(t.area, src, 64);
    const unsigned FW = __shfl(fw, src, 64);
    // this lane's pixel of the first block
    long long r0 = __shfl(e0, src, 64) + lx * S0x + ly * S0y;
    long long r1 = __shfl(e1, src, 64) + lx * S1x + ly * S1y;
    long long r2 = __shfl(e2, src, 64) + lx * S2x + ly * S2y;
    for (int y = Y0 + ly; y - ly <= Y1; y += 8) {
      long long c0 = r0, c1 = r1, c2 = r2;
      for (int x = X0 + lx; x - lx <= X1; x += 8) {
        if (x <= X1 && y <= Y1 && (c0 | c1 | c2) >= 0) emit(K, (size_t)y * W + x, c0 - B0, c1 - B1, c2 - B2, A, ZA, ZB, ZC, FW);
        c0 += 8 * S0x, c1 += 8 * S1x, c2 += 8 * S2x;
      }
      r0 += 8 * S0y, r1 += 8 * S1y, r2 += 8 * S2y;
    }
  }
}

// Every key of the jobs' rectangles := empty (once per chunk, before its first layer: the workspace arrives with any content).
__global__ __launch_bounds__(TILE_W* TILE_H) void render_clear_kernel(const int* __restrict__ sched, const int* __restrict__ job_frame,
                                                                      const int* __restrict__ status, const JobInfo* __restrict__ info,
                                                                      unsigned long long* __restrict__ keys, int W, int H, int frame0) {
  const int job = sched[blockIdx.y];
  if (status[job] & STATUS_NONFINITE) return;
  const Rect r = job_rect(info[job], W, H);
  if (r.x1 < r.x0 || r.y1 < r.y0) return;
  unsigned long long* K = keys + (size_t)(job_frame[job] - frame0) * W * H;
  const int tx = (r.x1 - r.x0) / TILE_W + 1, ty = (r.y1 - r.y0) / TILE_H + 1;
  const int lx = threadIdx.x & (TILE_W - 1), ly = threadIdx.x / TILE_W;
  for (int tile = blockIdx.x; tile < tx * ty; tile += gridDim.x) {
    const int x = r.x0 + (tile % tx) * TILE_W + lx, y = r.y0 + (tile / tx) * TILE_H + ly;
    if (x <= r.x1 && y <= r.y1) K[(size_t)y * W + x] = KEY_EMPTY;
  }
}

__device__ __forceinline__ unsigned char to_u8(float c) {
  c = fminf(fmaxf(c, 0.0f), 1.0f);
  return (unsigned char)floorf(255.0f * c + 0.5f);
}

__global__ __launch_bounds__(TILE_W* TILE_H) void render_resolve_kernel(const int* __restrict__ faces, const int2* __restrict__ xy_ws,
                                                                        const VertRec* __restrict__ rec_ws, const int* __restrict__ sched,
                                                                        const int* __restrict__ job_frame, const int* __restrict__ status,
                                                                        const JobInfo* __restrict__ info,
                                                                        unsigned long long* __restrict__ keys,
                                                                        unsigned char* __restrict__ images, int* __restrict__ face_id,
                                                                        float* __restrict__ depth, int V, int NF, int W, int H, int frame0,
                                                                        unsigned face_base, ShadeParams sp) {
#pragma clang fp contract(off)
  const int job = sched[blockIdx.y];
  if (status[job] & STATUS_NONFINITE) return;
  const Rect r = job_rect(info[job], W, H);
  if (r.x1 < r.x0 || r.y1 < r.y0) return;
  const int frame = job_frame[job];
  unsigned long long* K = keys + (size_t)(frame - frame0) * W * H;
  const size_t img0 = (size_t)frame * W * H;
  const int2* xy = xy_ws + (size_t)job * V;
  const VertRec* rec = rec_ws + (size_t)job * V;
  const int tx = (r.x1 - r.x0) / TILE_W + 1, ty = (r.y1 - r.y0) / TILE_H + 1;
  const int lx = threadIdx.x & (TILE_W - 1), ly = threadIdx.x / TILE_W;
  for (int tile = blockIdx.x; tile < tx * ty; tile += gridDim.x) {
    const int x = r.x0 + (tile % tx) * TILE_W + lx, y = r.y0 + (tile / tx) * TILE_H + ly;
    if (x > r.x1 || y > r.y1) continue;
    const size_t pix = (size_t)y * W + x;
    const unsigned long long key = K[pix];
    if (key == KEY_EMPTY) continue;
    const unsigned fw = (unsigned)key - face_base;  // another layer's fragment (order = depth) wraps or lands at >= NF
    if (fw >= (unsigned)NF) continue;
    K[pix] = KEY_EMPTY;
    const int f = (int)fw;
    // the triangle as the raster stage wound it
    int ia = faces[3 * f + 0], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    const int2 a = xy[ia];
    int2 b = xy[ib], c = xy[ic];
    if ((long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x) < 0) {
      const int2 t2 = b;
      b = c, c = t2;
      const int ti = ib;
      ib = ic, ic = ti;
    }
    const int px = x * FIX_ONE + FIX_HALF, py = y * FIX_ONE + FIX_HALF;
    const float wa = (float)edge_at(b.x, b.y, c.x, c.y, px, py);
    const float wb = (float)edge_at(c.x, c.y, a.x, a.y, px, py);
    const float wc = (float)edge_at(a.x, a.y, b.x, b.y, px, py);
    const VertRec ra = rec[ia], rb = rec[ib], rc = rec[ic];
    // the weights' common factor 1 / area drops out of the normalisation
    float n0 = (wa * ra.nx + wb * rb.nx) + wc * rc.nx;
    float n1 = (wa * ra.ny + wb * rb.ny) + wc * rc.ny;
    float n2 = (wa * ra.nz + wb * rb.nz) + wc * rc.nz;
    const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
    const float inv = len > 0.f ? 1.0f / len : 0.f;
    n0 *= inv, n1 *= inv, n2 *= inv;
    float lsum = 0.f;
    for (int l = 0; l < sp.n_lights; ++l) lsum += fmaxf(0.f, (n0 * sp.lights[l][0] + n1 * sp.lights[l][1]) + n2 * sp.lights[l][2]);
    const float k = sp.ambient + sp.light_scale * lsum;
    unsigned char* out = images + (img0 + pix) * 3;
    out[0] = to_u8(sp.emissive + k * sp.base[0]);
    out[1] = to_u8(sp.emissive + k * sp.base[1]);
    out[2] = to_u8(sp.emissive + k * sp.base[2]);
    if (face_id) face_id[img0 + pix] = f;
    if (depth) depth[img0 + pix] = z_from_bits((unsigned)(key >> 32));
  }
}

constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t job_bytes(int N, int V) {
  return align256((size_t)N * sizeof(JobInfo)) + align256((size_t)N * V * sizeof(int2)) + align256((size_t)N * V * sizeof(VertRec));
}

}  // namespace

extern "C" size_t pmce_render_workspace_bytes(int n_jobs, int n_verts, int width, int height, int chunk_frames) {
  if (n_jobs < 0 || n_verts < 1 || width < 1 || height < 1 || width > MAX_DIM || height > MAX_DIM || chunk_frames < 1) {
    pmce_set_error("render_workspace_bytes: n_jobs >= 0, n_verts >= 1, 1 <= width, height <= %d, chunk_frames >= 1 (got %d, %d, %d, %d, %d)",
                   MAX_DIM, n_jobs, n_verts, width, height, chunk_frames);
    return 0;
  }
  return job_bytes(n_jobs, n_verts) + (size_t)chunk_frames * width * height * sizeof(unsigned long long);
}

extern "C" int pmce_render_meshes(unsigned char* images, int n_frames, int width, int height, const float* verts, const float* cams,
                                  const float* rotation, int n_jobs, int n_verts, const int* faces, int n_faces, const int* vf_offsets,
                                  const int* vf_faces, const int* job_frame_host, const int* job_frame, const int* sched_host,
                                  const int* sched, const int* layer_offsets_host, int n_layers, const float* material,
                                  const float* lights, int n_lights, int cull_backfaces, int depth_order, int* status, int* xy_fixed,
                                  int* face_id, float* depth, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const char* what = "render_meshes";
  const int N = n_jobs, V = n_verts, NF = n_faces, W = width, H = height, F = n_frames, L = n_layers;
  PMCE_REQUIRE(W >= 1 && H >= 1 && W <= MAX_DIM && H <= MAX_DIM, "%s: width and height must be in 1..%d (got %d x %d)", what, MAX_DIM, W, H);
  PMCE_REQUIRE(F >= 0 && N >= 0 && V >= 1 && NF >= 1 && L >= 0, "%s: negative or empty size (F %d, N %d, V %d, faces %d, layers %d)", what, F,
               N, V, NF, L);
  PMCE_REQUIRE(n_lights >= 0 && n_lights <= MAX_LIGHTS, "%s: at most %d lights (got %d)", what, MAX_LIGHTS, n_lights);
  PMCE_REQUIRE(material && (lights || n_lights == 0), "%s: null material or lights", what);
  if (N == 0) return PMCE_OK;
  PMCE_REQUIRE(images && verts && cams && faces && vf_offsets && vf_faces && job_frame_host && job_frame && sched_host && sched &&
                   layer_offsets_host && status && workspace,
               "%s: null pointer", what);
  PMCE_REQUIRE(N <= 65535 * 64, "%s: too many jobs (%d)", what, N);
  PMCE_REQUIRE(!depth_order || (long long)L * NF < (1ll << 31), "%s: order = depth needs layers * faces < 2^31 (got %d * %d)", what, L, NF);
  PMCE_REQUIRE(L >= 1 && layer_offsets_host[0] == 0 && layer_offsets_host[L] == N, "%s: layer_offsets must run from 0 to n_jobs = %d", what, N);
  for (int l = 0; l < L; ++l) {
    PMCE_REQUIRE(layer_offsets_host[l] <= layer_offsets_host[l + 1], "%s: layer_offsets must be monotone (layer %d)", what, l);
    for (int p = layer_offsets_host[l]; p < layer_offsets_host[l + 1]; ++p) {
      const int j = sched_host[p];
      PMCE_REQUIRE(j >= 0 && j < N, "%s: schedule entry %d names job %d of %d", what, p, j, N);
      const int fr = job_frame_host[j];
      PMCE_REQUIRE(fr >= 0 && fr < F, "%s: job %d belongs to frame %d of %d", what, j, fr, F);
      PMCE_REQUIRE(p == layer_offsets_host[l] || job_frame_host[sched_host[p - 1]] < fr,
                   "%s: the jobs of layer %d must have ascending, distinct frames (entry %d)", what, l, p);
    }
  }
  const size_t jb = job_bytes(N, V), per_frame = (size_t)W * H * sizeof(unsigned long long);
  if (workspace_bytes < jb + per_frame) {
    pmce_set_error("%s: workspace of %zu bytes, %zu needed for one frame per chunk (pmce_render_workspace_bytes)", what, workspace_bytes,
                   jb + per_frame);
    return PMCE_ERR_WORKSPACE;
  }
  PMCE_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  const int chunk = (int)std::min<size_t>((workspace_bytes - jb) / per_frame, (size_t)std::min(F, 65535));

  char* ws = static_cast<char*>(workspace);
  JobInfo* info = reinterpret_cast<JobInfo*>(ws);
  int2* xy_ws = reinterpret_cast<int2*>(ws + align256((size_t)N * sizeof(JobInfo)));
  VertRec* rec_ws = reinterpret_cast<VertRec*>(reinterpret_cast<char*>(xy_ws) + align256((size_t)N * V * sizeof(int2)));
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + jb);

  ShadeParams sp{};
  for (int c = 0; c < 3; ++c) sp.base[c] = material[c];
  sp.emissive = material[3], sp.ambient = material[4], sp.light_scale = (float)((double)material[5] / M_PI);
  sp.n_lights = n_lights;
  for (int l = 0; l < n_lights; ++l)
    for (int c = 0; c < 3; ++c) sp.lights[l][c] = lights[3 * l + c];

  hipLaunchKernelGGL(render_init_kernel, dim3((N + VERT_THREADS - 1) / VERT_THREADS), dim3(VERT_THREADS), 0, stream, info, status, N);
  for (int j0 = 0; j0 < N; j0 += 65535) {  // grid.y carries the job
    const int nj = std::min(65535, N - j0);
    hipLaunchKernelGGL(render_vertex_kernel, dim3((V + VERT_THREADS - 1) / VERT_THREADS, nj), dim3(VERT_THREADS), 0, stream,
                       verts + (size_t)j0 * V * 3, cams + (size_t)j0 * 4, rotation ? rotation + (size_t)j0 * 9 : nullptr, faces, vf_offsets,
                       vf_faces, xy_ws + (size_t)j0 * V, rec_ws + (size_t)j0 * V, xy_fixed ? xy_fixed + (size_t)j0 * V * 2 : nullptr,
                       info + j0, status + j0, V, W, H);
  }
  PMCE_TRY(pmce_check_launch(what));

  std::vector<int> at(layer_offsets_host, layer_offsets_host + L);  // per layer: the first entry not yet drawn
  std::vector<int> lo(L), hi(L);
  const dim3 fgrid((unsigned)(((long long)NF * GROUP + RASTER_THREADS - 1) / RASTER_THREADS));
  for (int f0 = 0; f0 < F; f0 += chunk) {
    const int f1 = std::min(F, f0 + chunk);
    bool any = false;
    for (int l = 0; l < L; ++l) {
      lo[l] = at[l];
      while (at[l] < layer_offsets_host[l + 1] && job_frame_host[sched_host[at[l]]] < f1) ++at[l];
      hi[l] = at[l];
      any |= hi[l] > lo[l];
    }
    if (!any) continue;
    for (int l = 0; l < L; ++l)
      if (hi[l] > lo[l])
        hipLaunchKernelGGL(render_clear_kernel, dim3(RECT_WGS, hi[l] - lo[l]), dim3(TILE_W * TILE_H), 0, stream, sched + lo[l], job_frame,
                           status, info, keys, W, H, f0);
    for (int pass = 0; pass < (depth_order ? 2 : 1); ++pass)
      for (int l = 0; l < L; ++l) {
        if (hi[l] == lo[l]) continue;
        const unsigned base = depth_order ? (unsigned)l * (unsigned)NF : 0u;
        if (!depth_order || pass == 0)
          hipLaunchKernelGGL(render_raster_kernel, dim3(fgrid.x, hi[l] - lo[l]), dim3(RASTER_THREADS), 0, stream, faces, xy_ws, rec_ws,
                             sched + lo[l], job_frame, status, keys, V, NF, W, H, f0, base, cull_backfaces);
        if (!depth_order || pass == 1)
          hipLaunchKernelGGL(render_resolve_kernel, dim3(RECT_WGS, hi[l] - lo[l]), dim3(TILE_W * TILE_H), 0, stream, faces, xy_ws, rec_ws,
                             sched + lo[l], job_frame, status, info, keys, images, face_id, depth, V, NF, W, H, f0, base, sp);
      }
    PMCE_TRY(pmce_check_launch(what));
  }
  return PMCE_OK;
}
