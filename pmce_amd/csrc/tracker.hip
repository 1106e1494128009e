// The tracker's back half on device: non-maximum suppression of the detector's rows and SORT over a video's frames.
//
// What is restated (published texts; nothing of the yolov3, filterpy, sort or multi_person_tracker packages was on the build machine and
// no value was recorded from them; tests/tracker_ref.py is the same text in torch / numpy):
//   * the PyTorch-YOLOv3 lineage's non_max_suppression: candidates conf >= conf_thres, score = conf * max class, sorted by score, a head
//     merges every remaining candidate of its class whose +1-form IoU with it is > nms_thres into the conf-weighted mean box;
//   * Bewley's SORT (sort.py) over filterpy's KalmanFilter formulas: a constant-velocity filter on (u, v, s, r, du, dv, ds) per person,
//     IoU association by an assignment that maximises the total IoU, max_age / min_hits book-keeping;
//   * multi_person_tracker's run_tracker: detections of the person class above a score, a frame without any leaves the tracker alone.
// The project's own rules where the texts leave a choice: sort ties go to the lower row; a head always leaves the list (the lineage
// loops forever on a head whose self-IoU is not > nms_thres, e.g. an infinite extent); the fp32 kept boxes are mapped to the frame in
// fp64; the newer sort.py's shortcut for threshold matrices that are already one-to-one is not built (the publication's form is).
//
// nms_kernel: one workgroup of 1024 threads per image, everything in LDS sized by max_candidates.
//   A  the candidates are compacted in row order: per tile of 1024 rows a ballot per wave, the waves' counts through LDS, a prefix;
//      the strided read of the conf column touches one cache line per row - the rows are (5 + nc) floats apart - once.
//   B  a wave per candidate: the class maximum (first index) across the class columns by a butterfly on (value, index), the corners,
//      the score; key = (descending-orderable score bits, position), position order = row order.
//   C  a bitonic sort of the 64-bit keys in LDS.
//   D  wave 0 walks the heads serially; per head the remaining candidates 64 at a time: IoU, a ballot of the merged ones, and the
//      weighted sums over that ballot's bits in sorted order - one fixed order, no atomics, the same bits whatever n.
//   E  lane k of wave 0 owns kept row k: the person filter and the fp64 map to the frame, compacted by a ballot; then the whole
//      workgroup writes the image's rows (or zeros when a cap was exceeded: an image is never served partially).
//
// sort_kernel: one 64-lane wave (one workgroup) per sequence of frames, lane t owns tracker slot t: its state in registers, its
//   covariance and the products of the Joseph form in LDS ([element][lane]: conflict-free), all fp64 with contraction off in the order
//   tests/tracker_ref.py writes.  Slots are not moved: the list order of sort.py is the creation order, i.e. ascending id, so the
//   reversed walk that reports is "descending id" and needs a rank, not a compaction; a new tracker takes the lowest free slot.  The
//   assignment is exact: shortest augmenting paths with potentials over the matrix cost[d][t] = -IoU (0 for a free slot, which is a
//   dummy column: rows <= 64 = columns always holds), lane t owns column t, one wave minimum per step.
//   With a state record (pmce_sort_track_resume_f64) the wave loads lane state, covariance, frame_count and next_id before its first
//   frame and stores them after its last, [element][lane] like the LDS copy: every load and store is 64 consecutive words.  A slot that
//   is not alive is stored as zeros, and an all-zero record is the fresh tracker, so the bits of a video do not depend on its cuts.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int NMS_THREADS = 1024;
constexpr int NMS_WAVES = NMS_THREADS / 64;
constexpr int NMS_MAX_CAND = 2048;
constexpr int NMS_MAX_KEEP = 64;
constexpr int NMS_BYTES_PER_CAND = 8 + 4 + 16 + 4 + 4 + 4;  // key, row, box, conf, cls_conf, cls

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(const float* __restrict__ rows, int R, int nc, float conf_thres,
                                                           float nms_thres, int max_cand, int cap, int max_keep,
                                                           float* __restrict__ dets, int* __restrict__ count, int* __restrict__ status,
                                                           int* __restrict__ src_row, double* __restrict__ people,
                                                           int* __restrict__ people_count, int class_id, double score_thres,
                                                           int score_product, double pad_x, double pad_y, double ratio) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char nms_lds[];
  __shared__ int wave_cnt[NMS_WAVES];
  __shared__ float kept[NMS_MAX_KEEP * 7];
  __shared__ int kept_row[NMS_MAX_KEEP];
  __shared__ int fin[2];  // count, status
  unsigned long long* key = reinterpret_cast<unsigned long long*>(nms_lds);
  f32x4* box = reinterpret_cast<f32x4*>(nms_lds + (size_t)cap * 8);
  int* rowi = reinterpret_cast<int*>(nms_lds + (size_t)cap * 24);
  float* conf = reinterpret_cast<float*>(nms_lds + (size_t)cap * 28);
  float* clsc = reinterpret_cast<float*>(nms_lds + (size_t)cap * 32);
  int* clsi = reinterpret_cast<int*>(nms_lds + (size_t)cap * 36);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x;
  const int E = 5 + nc;
  const float* base = rows + (size_t)img * R * E;

  // A: compaction in row order
  int M = 0;  // candidates so far (uniform)
  for (int r0 = 0; r0 < R; r0 += NMS_THREADS) {
    const int r = r0 + tid;
    const bool c = r < R && base[(size_t)r * E + 4] >= conf_thres;
    const unsigned long long b = __ballot(c);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NMS_WAVES; ++w) {
      const int v = wave_cnt[w];
      before += w < wave ? v : 0;
      total += v;
    }
    const int at = M + before + __popcll(b & lanes_below(lane));
    if (c && at < max_cand) rowi[at] = r;
    M += total;
    __syncthreads();
  }
  if (M > max_cand) {  // uniform: the image is served empty
    for (int i = tid; i < max_keep * 7; i += NMS_THREADS) dets[(size_t)img * max_keep * 7 + i] = 0.f;
    if (src_row)
      for (int i = tid; i < max_keep; i += NMS_THREADS) src_row[(size_t)img * max_keep + i] = -1;
    if (people)
      for (int i = tid; i < max_keep * 5; i += NMS_THREADS) people[(size_t)img * max_keep * 5 + i] = 0.0;
    if (tid == 0) {
      count[img] = 0;
      status[img] = 1;
      if (people_count) people_count[img] = 0;
    }
    return;
  }

  // B: class maximum, corners, score, key
  for (int p = wave; p < M; p += NMS_WAVES) {
    const float* row = base + (size_t)rowi[p] * E;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < nc; c += 64) {
      const float v = row[5 + c];
      if (v > best || bi == 0x7fffffff) {
        best = v;
        bi = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      const bool take = oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi));
      best = take ? ov : best;
      bi = take ? oi : bi;
    }
    if (lane == 0) {
      const float cx = row[0], cy = row[1], w = row[2], h = row[3], cf = row[4];
      const float hw = w / 2, hh = h / 2;
      box[p] = f32x4{cx - hw, cy - hh, cx + hw, cy + hh};
      conf[p] = cf;
      clsc[p] = best;
      clsi[p] = bi;
      const float score = cf * best + 0.0f;
      unsigned u = __float_as_uint(score);
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending in the float's order
      key[p] = ((unsigned long long)(~u) << 32) | (unsigned)p;
    }
  }
  int P2 = 1;
  while (P2 < M) P2 <<= 1;
  for (int i = M + tid; i < P2; i += NMS_THREADS) key[i] = ~0ull;
  __syncthreads();

  // C: bitonic sort, ascending keys = score descending, row ascending
  for (int k = 2; k <= P2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += NMS_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = key[i], b = key[l];
          const bool up = (i & k) == 0;
          if ((a > b) == up) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
      __syncthreads();
    }
  }

  // D: the greedy loop, wave 0
  if (wave == 0) {
    unsigned alive = 0;  // bit c: candidate 64 c + lane remains
    const int chunks = (M + 63) >> 6;
    for (int c = 0; c < chunks; ++c) alive |= (64 * c + lane < M) ? (1u << c) : 0u;
    int nk = 0, st = 0;
    int h = 0;
    while (true) {
      // the first remaining candidate at or after h
      int c = h >> 6;
      int found = -1;
      for (; c < chunks; ++c) {
        unsigned long long m = __ballot((alive >> c) & 1u);
        if (c == (h >> 6)) m &= ~lanes_below(h & 63);
        if (m) {
          found = 64 * c + __builtin_ctzll(m);
          break;
        }
      }
      if (found < 0) break;
      h = found;
      if (nk >= max_keep) {
        st = 2;
        break;
      }
      const int hp = (int)(key[h] & 0xffffffffu);
      const f32x4 hb = box[hp];
      const int hcls = clsi[hp];
      const float harea = (hb.z - hb.x + 1) * (hb.w - hb.y + 1);
      float acc = 0.f, wsum = 0.f;
      for (c = h >> 6; c < chunks; ++c) {
        const int s = 64 * c + lane;
        bool inv = false;
        if ((alive >> c) & 1u) {
          const int p = (int)(key[s] & 0xffffffffu);
          const f32x4 b = box[p];
          const float ix1 = fmaxf(hb.x, b.x), iy1 = fmaxf(hb.y, b.y), ix2 = fminf(hb.z, b.z), iy2 = fminf(hb.w, b.w);
          const float inter = fmaxf(ix2 - ix1 + 1, 0.f) * fmaxf(iy2 - iy1 + 1, 0.f);
          const float barea = (b.z - b.x + 1) * (b.w - b.y + 1);
          const float iou = inter / (harea + barea - inter + 1e-16f);
          inv = clsi[p] == hcls && iou > nms_thres;
        }
        unsigned long long m = __ballot(inv);
        if (inv) alive &= ~(1u << c);
        while (m) {  // sorted order
          const int sj = 64 * c + __builtin_ctzll(m);
          m &= m - 1;
          const int pj = (int)(key[sj] & 0xffffffffu);
          const float cj = conf[pj];
          const float v = reinterpret_cast<const float*>(&box[pj])[lane & 3];
          acc = acc + cj * v;
          wsum = wsum + cj;
        }
      }
      if ((h & 63) == lane) alive &= ~(1u << (h >> 6));  // the head always leaves
      const float merged = acc / wsum;
      if (lane < 4) kept[nk * 7 + lane] = merged;
      if (lane == 4) kept[nk * 7 + 4] = conf[hp];
      if (lane == 5) kept[nk * 7 + 5] = clsc[hp];
      if (lane == 6) kept[nk * 7 + 6] = (float)hcls;
      if (lane == 7) kept_row[nk] = rowi[hp];
      ++nk;
      ++h;
    }
    if (st) nk = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // E: the tracker's inputs
    if (people) {
      bool ok = false;
      double x1 = 0, y1 = 0, x2 = 0, y2 = 0, sc = 0;
      if (lane < nk) {
        const float cf = kept[lane * 7 + 4], cc = kept[lane * 7 + 5];
        const float s32 = score_product ? cf * cc : cf;
        sc = (double)s32;
        x1 = (double)kept[lane * 7 + 0] * ratio - pad_x;
        y1 = (double)kept[lane * 7 + 1] * ratio - pad_y;
        x2 = (double)kept[lane * 7 + 2] * ratio - pad_x;
        y2 = (double)kept[lane * 7 + 3] * ratio - pad_y;
        ok = (int)kept[lane * 7 + 6] == class_id && sc > score_thres && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) &&
             x2 - x1 > 0 && y2 - y1 > 0;
      }
      const unsigned long long m = __ballot(ok);
      const int np = __popcll(m);
      double* out = people + (size_t)img * max_keep * 5;
      if (ok) {
        double* o = out + 5 * __popcll(m & lanes_below(lane));
        o[0] = x1;
        o[1] = y1;
        o[2] = x2;
        o[3] = y2;
        o[4] = sc;
      }
      if (lane >= np && lane < max_keep)
        for (int e = 0; e < 5; ++e) out[5 * lane + e] = 0.0;
      if (lane == 0) people_count[img] = np;
    }
    if (lane == 0) {
      fin[0] = nk;
      fin[1] = st;
      count[img] = nk;
      status[img] = st;
    }
  }
  __syncthreads();
  const int nk = fin[0];
  for (int i = tid; i < max_keep * 7; i += NMS_THREADS) dets[(size_t)img * max_keep * 7 + i] = i < nk * 7 ? kept[i] : 0.f;
  if (src_row)
    for (int i = tid; i < max_keep; i += NMS_THREADS) src_row[(size_t)img * max_keep + i] = i < nk ? kept_row[i] : -1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// SORT
// ---------------------------------------------------------------------------------------------------------------------------------

constexpr int SORT_MAX = 64;
// LDS doubles: P [49][64], AP [49][64], cost [64][64], det [64][4], u [65]; ints: p [65], way [65], d2t [64]
constexpr int SORT_LDS_DOUBLES = 49 * 64 * 2 + 64 * 64 + 64 * 4 + 65;
constexpr int SORT_LDS_BYTES = SORT_LDS_DOUBLES * 8 + (65 + 65 + 64) * 4;
// the state record of one sequence (include/pmce_hip.h): doubles x [7][64], P [49][64]; ints alive, id, tsu, streak [4][64], then
// frame_count, next_id.  A whole number of doubles, so consecutive records stay aligned.
constexpr int SORT_STATE_DOUBLES = (7 + 49) * 64;
constexpr int SORT_STATE_INTS = 4 * 64 + 2;
constexpr size_t SORT_STATE_BYTES = (size_t)SORT_STATE_DOUBLES * 8 + (size_t)SORT_STATE_INTS * 4;
static_assert(SORT_STATE_BYTES % 8 == 0, "records must keep the doubles aligned");

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

struct Box4 {
  double x1, y1, x2, y2;
};

__device__ __forceinline__ Box4 state_box(const double* x) {
#pragma clang fp contract(off)
  const double w = __dsqrt_rn(x[2] * x[3]);
  const double h = x[2] / w;
  return Box4{x[0] - w / 2, x[1] - h / 2, x[0] + w / 2, x[1] + h / 2};
}

__global__ __launch_bounds__(64) void sort_kernel(const double* __restrict__ people, const int* __restrict__ people_count,
                                                   const int* __restrict__ seq, int F, int K, int max_age, int min_hits, double iou_thr,
                                                   int max_tracks, int update_on_empty, double* __restrict__ tracks,
                                                   int* __restrict__ track_count, int* __restrict__ status,
                                                   unsigned char* __restrict__ state) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char sort_lds[];
  double* Pm = reinterpret_cast<double*>(sort_lds);
  double* APm = Pm + 49 * 64;
  double* cost = APm + 49 * 64;
  double* det = cost + 64 * 64;
  double* u = det + 64 * 4;
  int* pcol = reinterpret_cast<int*>(u + 65);
  int* way = pcol + 65;
  int* d2t = way + 65;
  const int lane = threadIdx.x;
  const int f0 = seq ? seq[blockIdx.x] : 0, f1 = seq ? seq[blockIdx.x + 1] : F;
#define PE(i, j) Pm[((i) * 7 + (j)) * 64 + lane]
#define AP(i, j) APm[((i) * 7 + (j)) * 64 + lane]
  const double Rd[4] = {1.0, 1.0, 10.0, 10.0};
  const double Qd[7] = {1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001};
  const double P0[7] = {10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4};

  double x[7] = {0, 0, 0, 0, 0, 0, 0};
  bool alive = false;
  int id = -1, tsu = 0, streak = 0;
  int frame_count = 0, next_id = 0;

  double* sd = nullptr;  // this sequence's record
  int* si = nullptr;
  if (state) {
    if (f0 >= f1) return;  // no frame in this call: the record is not touched (uniform)
    sd = reinterpret_cast<double*>(state + (size_t)blockIdx.x * SORT_STATE_BYTES);
    si = reinterpret_cast<int*>(sd + SORT_STATE_DOUBLES);
    alive = si[lane] != 0;
    id = si[64 + lane];
    tsu = si[128 + lane];
    streak = si[192 + lane];
    frame_count = si[256];
    next_id = si[257];
#pragma unroll
    for (int i = 0; i < 7; ++i) x[i] = sd[i * 64 + lane];
#pragma unroll
    for (int e = 0; e < 49; ++e) Pm[e * 64 + lane] = sd[(7 + e) * 64 + lane];
  }

  for (int f = f0; f < f1; ++f) {
    int nd = people_count[f];
    nd = nd < 0 ? 0 : (nd > K ? K : nd);
    double* out = tracks + (size_t)f * max_tracks * 5;
    if (nd == 0 && !update_on_empty) {
      if (lane < max_tracks)
        for (int e = 0; e < 5; ++e) out[5 * lane + e] = 0.0;
      if (lane == 0) {
        track_count[f] = 0;
        status[f] = 0;
      }
      continue;
    }
    ++frame_count;
    if (lane < nd) {
      const double* d = people + ((size_t)f * K + lane) * 5;
      det[4 * lane + 0] = d[0];
      det[4 * lane + 1] = d[1];
      det[4 * lane + 2] = d[2];
      det[4 * lane + 3] = d[3];
    }
    d2t[lane] = -1;
    // predict
    Box4 pb{0, 0, 0, 0};
    if (alive) {
      if (x[6] + x[2] <= 0) x[6] = 0;
      x[0] = x[0] + x[4];
      x[1] = x[1] + x[5];
      x[2] = x[2] + x[6];
#pragma unroll
      for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) PE(i, j) = PE(i, j) + PE(i + 4, j);  // F P
#pragma unroll
      for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) PE(i, j) = PE(i, j) + PE(i, j + 4);  // (F P) F'
        PE(i, i) = PE(i, i) + Qd[i];
      }
      if (tsu > 0) streak = 0;
      ++tsu;
      pb = state_box(x);
      if (isnan(pb.x1) || isnan(pb.y1) || isnan(pb.x2) || isnan(pb.y2)) alive = false;
    }
    __syncthreads();
    const unsigned long long amask = __ballot(alive);
    int mdet = -1;  // the detection this tracker is matched to
    if (nd > 0 && amask) {
      // cost[d][t] = -IoU, 0 for a free slot
      for (int d = 0; d < nd; ++d) {
        double c = 0.0;
        if (alive) {
          const double a0 = det[4 * d], a1 = det[4 * d + 1], a2 = det[4 * d + 2], a3 = det[4 * d + 3];
          const double w = fmax(0.0, fmin(a2, pb.x2) - fmax(a0, pb.x1));
          const double h = fmax(0.0, fmin(a3, pb.y2) - fmax(a1, pb.y1));
          const double wh = w * h;
          c = -(wh / ((a2 - a0) * (a3 - a1) + (pb.x2 - pb.x1) * (pb.y2 - pb.y1) - wh));
        }
        cost[d * 64 + lane] = c;
      }
      // shortest augmenting paths with potentials: rows 1..nd, columns 1..64 (lane + 1), column 0 virtual
      double v = 0.0;
      u[lane] = 0.0;
      if (lane == 0) u[64] = 0.0;
      pcol[lane + 1] = 0;
      way[lane + 1] = 0;
      if (lane == 0) pcol[0] = 0;
      __syncthreads();
      for (int i = 1; i <= nd; ++i) {
        if (lane == 0) pcol[0] = i;
        double minv = INFINITY;
        bool used = false;
        int j0 = 0;
        __syncthreads();
        int guard = 0;
        do {
          if (j0 == lane + 1) used = true;
          const int i0 = pcol[j0];
          const double cur = cost[(i0 - 1) * 64 + lane] - u[i0] - v;
          if (!used && cur < minv) {
            minv = cur;
            way[lane + 1] = j0;
          }
          const double delta = wave_min_f64(used ? INFINITY : minv);
          const unsigned long long mm = __ballot(!used && minv == delta);
          if (mm == 0) break;  // (not finite: leave the row unmatched)
          const int j1 = __builtin_ctzll(mm) + 1;
          __syncthreads();
          if (used) {
            u[pcol[lane + 1]] += delta;
            v -= delta;
          } else {
            minv -= delta;
          }
          if (lane == 0) u[i] += delta;  // the virtual column's row
          __syncthreads();
          j0 = j1;
        } while (pcol[j0] != 0 && ++guard < 66);
        if (lane == 0 && pcol[j0] == 0) {
          int j = j0;
          do {
            const int jw = way[j];
            pcol[j] = pcol[jw];
            j = jw;
          } while (j);
        }
        __syncthreads();
      }
      const int prow = pcol[lane + 1];
      if (alive && prow > 0 && -cost[(prow - 1) * 64 + lane] >= iou_thr) {
        mdet = prow - 1;
        d2t[mdet] = lane;
      }
      __syncthreads();
    }
    // update the matched
    if (mdet >= 0) {
      tsu = 0;
      ++streak;
      const double b0 = det[4 * mdet], b1 = det[4 * mdet + 1], b2 = det[4 * mdet + 2], b3 = det[4 * mdet + 3];
      const double zw = b2 - b0, zh = b3 - b1;
      const double z[4] = {b0 + zw / 2, b1 + zh / 2, zw * zh, zw / zh};
      double y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = z[i] - x[i];
      // A = S' (S = P[:4,:4] + R), B = (P H')' [4][7]; solve A X = B; K = X'
      double A[4][4], B[4][7];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) A[i][j] = i == j ? PE(j, i) + Rd[i] : PE(j, i);
#pragma unroll
        for (int j = 0; j < 7; ++j) B[i][j] = PE(j, i);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int piv = k;
        double big = fabs(A[k][k]);
#pragma unroll
        for (int r = k + 1; r < 4; ++r) {
          const double a = fabs(A[r][k]);
          if (a > big) {
            big = a;
            piv = r;
          }
        }
#pragma unroll
        for (int r = k + 1; r < 4; ++r) {
          const bool sw = piv == r;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double a = A[k][j], b = A[r][j];
            A[k][j] = sw ? b : a;
            A[r][j] = sw ? a : b;
          }
#pragma unroll
          for (int j = 0; j < 7; ++j) {
            const double a = B[k][j], b = B[r][j];
            B[k][j] = sw ? b : a;
            B[r][j] = sw ? a : b;
          }
        }
#pragma unroll
        for (int i = k + 1; i < 4; ++i) {
          const double m = A[i][k] / A[k][k];
#pragma unroll
          for (int j = k + 1; j < 4; ++j) A[i][j] = A[i][j] - m * A[k][j];
#pragma unroll
          for (int j = 0; j < 7; ++j) B[i][j] = B[i][j] - m * B[k][j];
        }
      }
      double Kg[7][4];  // K[i][k] = X[k][i]
#pragma unroll
      for (int i = 3; i >= 0; --i) {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          double acc = B[i][c];
#pragma unroll
          for (int j = i + 1; j < 4; ++j) acc = acc - A[i][j] * Kg[c][j];
          Kg[c][i] = acc / A[i][i];
        }
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) x[i] = x[i] + (((Kg[i][0] * y[0] + Kg[i][1] * y[1]) + Kg[i][2] * y[2]) + Kg[i][3] * y[3]);
      // AP = (I - K H) P
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        double a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = (i == k ? 1.0 : 0.0) - Kg[i][k];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          double acc = a[0] * PE(0, j);
#pragma unroll
          for (int k = 1; k < 4; ++k) acc = acc + a[k] * PE(k, j);
          AP(i, j) = i >= 4 ? acc + PE(i, j) : acc;
        }
      }
      // P = AP (I - K H)' + K R K'
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        double a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = (j == k ? 1.0 : 0.0) - Kg[j][k];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          double acc = AP(i, 0) * a[0];
#pragma unroll
          for (int k = 1; k < 4; ++k) acc = acc + AP(i, k) * a[k];
          double g = (Kg[i][0] * Rd[0]) * Kg[j][0];
#pragma unroll
          for (int k = 1; k < 4; ++k) g = g + (Kg[i][k] * Rd[k]) * Kg[j][k];
          PE(i, j) = (j >= 4 ? acc + AP(i, j) : acc) + g;
        }
      }
    }
    // new trackers for the unmatched detections, in detection order, into the lowest free slots
    int st = 0;
    {
      const bool unm = lane < nd && d2t[lane] < 0;
      const unsigned long long um = __ballot(unm);
      const unsigned long long am = __ballot(alive);
      const unsigned long long slots = max_tracks >= 64 ? ~0ull : ((1ull << max_tracks) - 1);
      const unsigned long long freem = ~am & slots;
      const int nfree = __popcll(freem), nun = __popcll(um);
      const int ncreate = nun < nfree ? nun : nfree;
      if (nun > nfree) st = 1;
      // lane takes the q-th unmatched detection when it is the q-th free slot
      const int q = __popcll(freem & lanes_below(lane));
      if (((freem >> lane) & 1ull) && q < ncreate) {
        unsigned long long m = um;
        for (int s = 0; s < q; ++s) m &= m - 1;
        const int d = __builtin_ctzll(m);
        const double b0 = det[4 * d], b1 = det[4 * d + 1], b2 = det[4 * d + 2], b3 = det[4 * d + 3];
        const double zw = b2 - b0, zh = b3 - b1;
        x[0] = b0 + zw / 2;
        x[1] = b1 + zh / 2;
        x[2] = zw * zh;
        x[3] = zw / zh;
        x[4] = x[5] = x[6] = 0.0;
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
          for (int j = 0; j < 7; ++j) PE(i, j) = i == j ? P0[i] : 0.0;
        alive = true;
        id = next_id + q;
        tsu = 0;
        streak = 0;
      }
      next_id += ncreate;
    }
    // report: sort.py walks the list from last to first = descending id
    const bool rep = alive && tsu < 1 && (streak >= min_hits || frame_count <= min_hits);
    const unsigned long long rm = __ballot(rep);
    int pos = 0;
    for (unsigned long long m = rm; m; m &= m - 1) {
      const int l = __builtin_ctzll(m);
      pos += __shfl(id, l, 64) > id ? 1 : 0;
    }
    const int nrep = __popcll(rm);
    if (rep) {
      const Box4 b = state_box(x);
      double* o = out + 5 * pos;
      o[0] = b.x1;
      o[1] = b.y1;
      o[2] = b.x2;
      o[3] = b.y2;
      o[4] = (double)(id + 1);
    }
    if (lane >= nrep && lane < max_tracks)
      for (int e = 0; e < 5; ++e) out[5 * lane + e] = 0.0;
    if (lane == 0) {
      track_count[f] = nrep;
      status[f] = st;
    }
    if (alive && tsu > max_age) alive = false;
    __syncthreads();
  }
  if (state) {  // a slot that is not alive is zeros: equal histories give equal bytes
    si[lane] = alive ? 1 : 0;
    si[64 + lane] = alive ? id : 0;
    si[128 + lane] = alive ? tsu : 0;
    si[192 + lane] = alive ? streak : 0;
    if (lane == 0) {
      si[256] = frame_count;
      si[257] = next_id;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) sd[i * 64 + lane] = alive ? x[i] : 0.0;
#pragma unroll
    for (int e = 0; e < 49; ++e) sd[(7 + e) * 64 + lane] = alive ? Pm[e * 64 + lane] : 0.0;
  }
#undef PE
#undef AP
}

// prepare_output_tracks' box of reported row index[i] of tracks[total][5]: (cx, cy, s, s), s = w if w / h > 1 else h
__global__ __launch_bounds__(256) void tracklet_boxes_kernel(const double* __restrict__ tracks, const int* __restrict__ index, int total,
                                                             int n, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int r = index[i];
  double cx = 0, cy = 0, s = 0;
  if (r >= 0 && r < total) {
    const double* t = tracks + (size_t)r * 5;
    const double w = t[2] - t[0], h = t[3] - t[1];
    cx = t[0] + w / 2;
    cy = t[1] + h / 2;
    s = w / h > 1 ? w : h;
  }
  out[4 * (size_t)i + 0] = cx;
  out[4 * (size_t)i + 1] = cy;
  out[4 * (size_t)i + 2] = s;
  out[4 * (size_t)i + 3] = s;
}

std::atomic<unsigned long long> nms_lds_done{0}, sort_lds_done{0};

}  // namespace

extern "C" int pmce_yolo_nms_f32(const float* rows, int n, int R, int nc, float conf_thres, float nms_thres, int max_candidates,
                                 int max_keep, float* dets, int* count, int* status, int* src_row, double* people, int* people_count,
                                 int class_id, double score_thres, int score_product, double pad_x, double pad_y, double ratio,
                                 hipStream_t stream) {
  const char* what = "yolo_nms_f32";
  PMCE_REQUIRE(rows && dets && count && status, "%s: null pointer", what);
  PMCE_REQUIRE(n >= 0 && R >= 1, "%s: n must be >= 0 and R >= 1 (got %d, %d)", what, n, R);
  PMCE_REQUIRE(nc >= 1 && nc <= 255, "%s: nc must be in 1..255 (got %d)", what, nc);
  PMCE_REQUIRE(isfinite(conf_thres) && isfinite(nms_thres), "%s: the thresholds must be finite", what);
  PMCE_REQUIRE(max_candidates >= 1 && max_candidates <= NMS_MAX_CAND, "%s: max_candidates must be in 1..%d (got %d)", what, NMS_MAX_CAND,
               max_candidates);
  PMCE_REQUIRE(max_keep >= 1 && max_keep <= NMS_MAX_KEEP, "%s: max_keep must be in 1..%d (got %d)", what, NMS_MAX_KEEP, max_keep);
  PMCE_REQUIRE((people != nullptr) == (people_count != nullptr), "%s: people and people_count go together", what);
  if (people) {
    PMCE_REQUIRE(isfinite(score_thres) && isfinite(pad_x) && isfinite(pad_y) && isfinite(ratio) && ratio > 0,
                 "%s: score_thres and the geometry must be finite, ratio positive", what);
    PMCE_REQUIRE(class_id >= 0 && class_id < nc, "%s: class_id must be in 0..%d (got %d)", what, nc - 1, class_id);
  }
  PMCE_REQUIRE((long long)R * (5 + nc) * (long long)(n > 0 ? n : 1) < (1ll << 40), "%s: rows too large", what);
  if (n == 0) return PMCE_OK;
  int cap = 64;
  while (cap < max_candidates) cap <<= 1;
  const int bytes = cap * NMS_BYTES_PER_CAND;
  if (bytes > 48 * 1024) PMCE_TRY(pmce_opt_in_lds((const void*)nms_kernel, bytes, nms_lds_done, what));
  hipLaunchKernelGGL(nms_kernel, dim3(n), dim3(NMS_THREADS), bytes, stream, rows, R, nc, conf_thres, nms_thres, max_candidates, cap,
                     max_keep, dets, count, status, src_row, people, people_count, class_id, score_thres, score_product, pad_x, pad_y,
                     ratio);
  return pmce_check_launch(what);
}

namespace {

// the one launcher: state == nullptr is the whole-video form
int sort_track_launch(const char* what, const double* people, const int* people_count, const int* seq_offsets_host, const int* seq_offsets,
                      int F, int K, int S, int max_age, int min_hits, double iou_threshold, int max_tracks, int update_on_empty,
                      double* tracks, int* track_count, int* status, unsigned char* state, hipStream_t stream) {
  PMCE_REQUIRE(people && people_count && tracks && track_count && status, "%s: null pointer", what);
  PMCE_REQUIRE(F >= 0 && S >= 1, "%s: F must be >= 0 and S >= 1 (got %d, %d)", what, F, S);
  PMCE_REQUIRE(K >= 1 && K <= SORT_MAX, "%s: K (detections per frame) must be in 1..%d (got %d)", what, SORT_MAX, K);
  PMCE_REQUIRE(max_tracks >= 1 && max_tracks <= SORT_MAX, "%s: max_tracks must be in 1..%d (got %d)", what, SORT_MAX, max_tracks);
  PMCE_REQUIRE(max_age >= 0 && min_hits >= 0, "%s: max_age and min_hits must be >= 0 (got %d, %d)", what, max_age, min_hits);
  PMCE_REQUIRE(isfinite(iou_threshold), "%s: iou_threshold must be finite", what);
  PMCE_REQUIRE((seq_offsets_host == nullptr) == (seq_offsets == nullptr), "%s: give seq_offsets on the host and on the device, or neither",
               what);
  if (seq_offsets_host) {
    PMCE_REQUIRE(seq_offsets_host[0] == 0 && seq_offsets_host[S] == F, "%s: seq_offsets must start at 0 and end at F = %d (got %d .. %d)",
                 what, F, seq_offsets_host[0], seq_offsets_host[S]);
    for (int i = 0; i < S; ++i)
      PMCE_REQUIRE(seq_offsets_host[i] <= seq_offsets_host[i + 1], "%s: seq_offsets must be monotone (entry %d)", what, i);
  } else {
    PMCE_REQUIRE(S == 1, "%s: without seq_offsets there is one sequence (got S = %d)", what, S);
  }
  if (F == 0) return PMCE_OK;
  PMCE_TRY(pmce_opt_in_lds((const void*)sort_kernel, SORT_LDS_BYTES, sort_lds_done, what));
  hipLaunchKernelGGL(sort_kernel, dim3(S), dim3(64), SORT_LDS_BYTES, stream, people, people_count, seq_offsets, F, K, max_age, min_hits,
                     iou_threshold, max_tracks, update_on_empty, tracks, track_count, status, state);
  return pmce_check_launch(what);
}

}  // namespace

extern "C" int pmce_sort_track_f64(const double* people, const int* people_count, const int* seq_offsets_host, const int* seq_offsets,
                                   int F, int K, int S, int max_age, int min_hits, double iou_threshold, int max_tracks,
                                   int update_on_empty, double* tracks, int* track_count, int* status, hipStream_t stream) {
  return sort_track_launch("sort_track_f64", people, people_count, seq_offsets_host, seq_offsets, F, K, S, max_age, min_hits,
                           iou_threshold, max_tracks, update_on_empty, tracks, track_count, status, nullptr, stream);
}

extern "C" size_t pmce_sort_state_bytes(void) { return SORT_STATE_BYTES; }

extern "C" int pmce_sort_track_resume_f64(const double* people, const int* people_count, const int* seq_offsets_host,
                                          const int* seq_offsets, int F, int K, int S, int max_age, int min_hits, double iou_threshold,
                                          int max_tracks, int update_on_empty, double* tracks, int* track_count, int* status, void* state,
                                          hipStream_t stream) {
  const char* what = "sort_track_resume_f64";
  PMCE_REQUIRE(state, "%s: null pointer (state)", what);
  PMCE_REQUIRE(reinterpret_cast<uintptr_t>(state) % 8 == 0, "%s: state must be aligned to 8 bytes", what);
  return sort_track_launch(what, people, people_count, seq_offsets_host, seq_offsets, F, K, S, max_age, min_hits, iou_threshold,
                           max_tracks, update_on_empty, tracks, track_count, status, static_cast<unsigned char*>(state), stream);
}

extern "C" int pmce_tracklet_boxes_f64(const double* tracks, const int* index, int total, int n, double* out, hipStream_t stream) {
  const char* what = "tracklet_boxes_f64";
  PMCE_REQUIRE(total >= 0 && n >= 0, "%s: total and n must be >= 0 (got %d, %d)", what, total, n);
  if (n == 0) return PMCE_OK;
  PMCE_REQUIRE(tracks && index && out, "%s: null pointer", what);
  hipLaunchKernelGGL(tracklet_boxes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, tracks, index, total, n, out);
  return pmce_check_launch(what);
}
