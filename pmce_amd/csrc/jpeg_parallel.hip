// The entropy stage of the JPEG reader with many lanes per scan (jpeg_parallel.hpp has the method and the body, shared with
// scripts/jpeg_parallel_host.cpp): what pmce_jpeg_entropy does with one lane per restart interval, for files whose encoder wrote few
// restart markers or none - ffmpeg's and cv2.imwrite's.  The same coefficients and the same status words, for every byte string.
//
// A segment is cut into subsequences of S bytes, one lane each; RUN = 256 consecutive ones of a segment are one workgroup.  Launches
// of a round, fixed by the records (pmce_amd/jpeg.py computes each segment's first subsequence and first run):
//
//   sync     a workgroup per run.  Every lane decodes its subsequence from the guessed state, then the run goes to its fixed point in
//            LDS: a lane whose neighbour's exit differs from the entry it used decodes again, until a workgroup-wide vote finds no
//            change (at most RUN rounds).  The first lane of a segment enters with the true state, the first lane of a later run with
//            the guess.  Nothing but states and block counts is written.
//   join     the same workgroups, JOIN_ROUNDS times: the first lane of a run takes the exit that the run before it had after the launch
//            before (kept in two alternating arrays, so that no workgroup reads what another one writes in the same launch), and the
//            run goes to its fixed point again.  A Huffman stream resynchronises within a few symbols, so a run's last exit is the true
//            one however its first entry was guessed, and one round settles every border; the second serves runs with few lanes.
//   place    a workgroup per segment: the exclusive sum of the completed blocks gives every lane its first block, the first lane that
//            met a code error is found (the stream's first real one: jpeg_parallel.hpp), and the fixed-point
//            condition (entry[i] == exit[i - 1] for every lane, the true state for lane 0) is checked.  A segment that fails it is
//            handed to the serial body in `dc`: the result is exact for every stream, an adversarial one is merely slow.
//   write    a workgroup per run: every lane up to that one decodes once more from its true entry and writes its coefficients (the DC difference
//            at position 0), its status bits and how far it wrote DC differences.
//   dc       a workgroup per segment: status and extent reduced over the lanes, then the DC differences summed per component in 16-bit
//            wrapping arithmetic - or, for a segment that failed the check, jpeg_entropy.hpp's decode_segment by one lane.
//
// No atomics, no host read, no host wait; every loop is bounded by a run's or a segment's subsequence count.  The run's bytes and the
// Huffman tables lie in LDS where they fit.
#include "common.hpp"
#include "jpeg_parallel.hpp"

namespace {

namespace je = jpeg_entropy;
namespace jp = jpeg_parallel;

constexpr int MAX_LDS_TABLES = 16;
constexpr int MAX_DYNAMIC_LDS = 56 * 1024;
constexpr int NEAR_SLACK = 32;            // bytes of the next run kept with a run's own: most symbols that cross the border end there

struct Workspace {
  jp::State* entry;        // [n_sub]
  jp::State* exit;         // [n_sub]
  jp::State* border;       // [2][n_runs]: a run's last exit after the launch before this one, and after this one
  int* rounds;             // [1 + JOIN_ROUNDS][n_runs]: per launch, the rounds in which a lane of the run decoded again (read by nobody
                           // here: pmce_amd.jpeg.parallel_diagnostics)
  int* blocks;             // [n_sub]
  int* block0;             // [n_sub]
  int* status;             // [n_sub]: until `write`, 1: the lane met a code error (jpeg_parallel.hpp); then its status bits
  int* dc_end;             // [n_sub]
  int* serial;             // [n_seg]: 1: the segment failed the fixed-point check
  int* stop;               // [n_seg]: the first lane with a code error, or the number of lanes: no lane behind it is run by `write`
  int n_sub, n_runs;
};

struct Batch {
  const unsigned char* data;
  long long n_bytes;
  const int* segments;
  int seg0, n_seg;
  const int* images;
  int n_images;
  const int* huffman;
  int n_huffman;
  short* coef;
  long long n_blocks;
  const int* offsets;      // [segment][2]: its first subsequence and its first run within the round
  int S;
};

// Segment s of the round (0 .. n_seg): do its records fit the arrays, the workspace included?
__device__ __forceinline__ bool segment_fits(const Batch& a, const Workspace& w, int s, int& sub0, int& run0, int& n_sub) {
  const int* seg = a.segments + (long long)(a.seg0 + s) * je::SEG_WORDS;
  if (!je::check_segment(seg, a.n_bytes, a.images, a.n_images, a.n_huffman, a.n_blocks)) return false;
  sub0 = a.offsets[2 * (a.seg0 + s)];
  run0 = a.offsets[2 * (a.seg0 + s) + 1];
  n_sub = jp::subsequence_count(seg[2] - seg[1], a.S);
  const int runs = (n_sub + jp::RUN - 1) / jp::RUN;
  return sub0 >= 0 && run0 >= 0 && (long long)sub0 + n_sub <= w.n_sub && (long long)run0 + runs <= w.n_runs;
}

// The segment whose runs include run `q` of the round: the last one whose first run is at or below q.
__device__ __forceinline__ int segment_of_run(const Batch& a, int q) {
  int lo = 0, hi = a.n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.offsets[2 * (a.seg0 + mid) + 1] <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// What a workgroup of `sync` and `write` (one run) sets up: the segment, the tables and the run's bytes in LDS.  -> false: nothing to do.
template <bool LDS_TABLES, bool LDS_BYTES>
__device__ __forceinline__ bool run_setup(const Batch& a, const Workspace& w, unsigned char* lds, jp::Segment& g, int& s, int& sub0, int& first, int& q) {
  int* tables = reinterpret_cast<int*>(lds);
  unsigned char* bytes = lds + (LDS_TABLES ? (size_t)a.n_huffman * je::HUFF_WORDS * sizeof(int) : 0);
  if (LDS_TABLES)
    for (int i = threadIdx.x; i < a.n_huffman * je::HUFF_WORDS; i += jp::RUN) tables[i] = a.huffman[i];
  q = blockIdx.x;
  s = segment_of_run(a, q);
  int run0, n_sub;
  const bool fits = segment_fits(a, w, s, sub0, run0, n_sub);
  first = fits ? (q - run0) * jp::RUN : 0;
  if (!fits || q < run0 || first >= n_sub) {
    __syncthreads();
    return false;
  }
  const int* seg = a.segments + (long long)(a.seg0 + s) * je::SEG_WORDS;
  jp::segment_init(g, a.data, seg, a.images, LDS_TABLES ? tables : a.huffman, a.coef, a.S);
  g.near = bytes;
  if (LDS_BYTES) {
    const long long lo = (long long)g.begin + (long long)first * a.S;                 // first < n_sub: below the segment's end
    long long hi = lo + (long long)jp::RUN * a.S + NEAR_SLACK;
    if (hi > g.end) hi = g.end;
    for (int i = threadIdx.x; i < (int)(hi - lo); i += jp::RUN) bytes[i] = a.data[lo + i];
    g.near_lo = (int)lo;
    g.near_hi = (int)hi;
  }
  __syncthreads();
  return true;
}

// sync (join == 0) and the join rounds (1 ..).  grid: the round's runs; block: RUN.
template <bool LDS_TABLES, bool LDS_BYTES>
__global__ __launch_bounds__(jp::RUN) void jpeg_sync_kernel(Batch a, Workspace w, int join) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ jp::State s_exit[jp::RUN];
  jp::Segment g;
  int s, sub0, first, q;
  if (!run_setup<LDS_TABLES, LDS_BYTES>(a, w, lds, g, s, sub0, first, q)) return;
  const int t = threadIdx.x, i = first + t;
  const bool active = i < g.n_sub;
  const int n = min(jp::RUN, g.n_sub - first);           // lanes of this run
  const int at = sub0 + (active ? i : first);
  jp::State entry = 0;
  jp::Lane lane;
  lane.exit = 0;
  lane.blocks = lane.error = 0;
  if (join == 0) {
    if (active) {
      entry = jp::guess(g, i);
      jp::decode_subsequence<false>(g, i, entry, 0, lane);
    }
  } else if (active) {
    entry = w.entry[at];
    lane.exit = w.exit[at];
    lane.blocks = w.blocks[at];
    lane.error = w.status[at];
  }
  // the first lane's entry: the segment's first state, or the exit of the run before this one as the launch before left it
  const jp::State* border_in = w.border + (size_t)((join + 1) & 1) * w.n_runs;
  jp::State* border_out = w.border + (size_t)(join & 1) * w.n_runs;
  const jp::State e0 = first == 0 ? jp::guess(g, 0) : (join == 0 ? jp::guess(g, first) : border_in[q - 1]);
  s_exit[t] = lane.exit;
  int rounds = 0;
  for (int round = 0; round <= n; ++round) {             // lane k is settled after k rounds: the vote ends the loop before n + 1
    __syncthreads();
    const jp::State e = t == 0 ? e0 : s_exit[t - 1];
    const bool changed = active && e != entry;
    __syncthreads();
    if (changed) {
      entry = e;
      jp::decode_subsequence<false>(g, i, entry, 0, lane);
      s_exit[t] = lane.exit;
    }
    if (!__syncthreads_or(changed ? 1 : 0)) break;
    ++rounds;
  }
  if (t == 0) w.rounds[(size_t)join * w.n_runs + q] = rounds;
  if (active) {
    w.entry[at] = entry;
    w.exit[at] = lane.exit;
    w.blocks[at] = lane.blocks;
    w.status[at] = lane.error;
    if (t == n - 1) border_out[q] = lane.exit;
  }
}

// grid: the round's runs; block: RUN
template <bool LDS_TABLES, bool LDS_BYTES>
__global__ __launch_bounds__(jp::RUN) void jpeg_write_kernel(Batch a, Workspace w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  jp::Segment g;
  int s, sub0, first, q;
  if (!run_setup<LDS_TABLES, LDS_BYTES>(a, w, lds, g, s, sub0, first, q)) return;
  const int i = first + threadIdx.x;
  if (i >= g.n_sub || w.serial[s]) return;
  jp::Lane lane;
  lane.status = lane.dc_end = 0;
  if (i <= w.stop[s]) jp::decode_subsequence<true>(g, i, w.entry[sub0 + i], w.block0[sub0 + i], lane);
  w.status[sub0 + i] = lane.status;
  w.dc_end[sub0 + i] = lane.dc_end;
}

__device__ __forceinline__ int add_capped(int x, int y) { return min(x + y, jp::BLOCK_CAP); }        // both at most BLOCK_CAP = 2^30

// grid: the round's segments; block: RUN
__global__ __launch_bounds__(jp::RUN) void jpeg_place_kernel(Batch a, Workspace w) {
  __shared__ int sum[jp::RUN];
  const int s = blockIdx.x, t = threadIdx.x;
  int sub0, run0, n_sub;
  if (!segment_fits(a, w, s, sub0, run0, n_sub)) {
    if (t == 0) w.serial[s] = 0, w.stop[s] = 0;
    return;
  }
  const int* seg = a.segments + (long long)(a.seg0 + s) * je::SEG_WORDS;
  const jp::State start = jp::make_state(seg[1], 0, 0, 0);
  int carry = 0, bad = 0, stop = n_sub;
  for (int base = 0; base < n_sub; base += jp::RUN) {
    const int i = base + t;
    int v = 0;
    if (i < n_sub) {
      v = min(max(w.blocks[sub0 + i], 0), jp::BLOCK_CAP);
      bad |= w.entry[sub0 + i] != (i == 0 ? start : w.exit[sub0 + i - 1]);
      if (w.status[sub0 + i]) stop = min(stop, i);
    }
    sum[t] = v;
    __syncthreads();
    for (int d = 1; d < jp::RUN; d <<= 1) {              // inclusive sums
      const int x = t >= d ? sum[t - d] : 0;
      __syncthreads();
      sum[t] = add_capped(sum[t], x);
      __syncthreads();
    }
    if (i < n_sub) w.block0[sub0 + i] = add_capped(carry, t ? sum[t - 1] : 0);
    carry = add_capped(carry, sum[jp::RUN - 1]);
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
  sum[t] = stop;
  __syncthreads();
  for (int d = jp::RUN / 2; d > 0; d >>= 1) {
    if (t < d) sum[t] = min(sum[t], sum[t + d]);
    __syncthreads();
  }
  if (t == 0) w.serial[s] = bad ? 1 : 0, w.stop[s] = sum[0];
}

// grid: the round's segments; block: RUN
__global__ __launch_bounds__(jp::RUN) void jpeg_dc_kernel(Batch a, Workspace w, int* __restrict__ seg_status) {
  __shared__ int red[2][jp::RUN];
  __shared__ int part[3][jp::RUN];
  const int s = blockIdx.x, t = threadIdx.x;
  int sub0, run0, n_sub;
  if (!segment_fits(a, w, s, sub0, run0, n_sub)) {
    if (t == 0) seg_status[a.seg0 + s] = je::STATUS_RECORD;
    return;
  }
  const int* seg = a.segments + (long long)(a.seg0 + s) * je::SEG_WORDS;
  if (w.serial[s]) {
    if (t == 0)
      seg_status[a.seg0 + s] = je::decode_segment<false>(a.data, a.n_bytes, seg, a.images, a.n_images, a.huffman, a.n_huffman, a.coef,
                                                         a.n_blocks, nullptr, nullptr);
    return;
  }
  int st = 0, n = 0;
  for (int i = t; i < n_sub; i += jp::RUN) {
    st |= w.status[sub0 + i];
    n = max(n, w.dc_end[sub0 + i]);
  }
  red[0][t] = st;
  red[1][t] = n;
  __syncthreads();
  for (int d = jp::RUN / 2; d > 0; d >>= 1) {
    if (t < d) {
      red[0][t] |= red[0][t + d];
      red[1][t] = max(red[1][t], red[1][t + d]);
    }
    __syncthreads();
  }
  st = red[0][0];
  jp::Segment g;
  jp::segment_init(g, a.data, seg, a.images, a.huffman, a.coef, a.S);
  n = min(max(red[1][0], 0), g.limit);                    // (a lane writes no DC at or past the limit)
  if (t == 0) seg_status[a.seg0 + s] = st;
  // blocks [0, n): a piece per lane, the pieces' sums added up across the lanes, then each piece from its offset
  const int per = (n + jp::RUN - 1) / jp::RUN, k0 = min(t * per, n), k1 = min(k0 + per, n);
  int acc[3] = {0, 0, 0};
  for (int k = k0; k < k1; ++k) {
    const int c = jp::component_of(g, k % g.bpm);
    const int d = (unsigned short)g.coef[(long long)k * 64];
    acc[0] += c == 0 ? d : 0;
    acc[1] += c == 1 ? d : 0;
    acc[2] += c == 2 ? d : 0;
  }
  for (int c = 0; c < 3; ++c) part[c][t] = acc[c];
  __syncthreads();
  for (int d = 1; d < jp::RUN; d <<= 1) {
    int x[3];
    for (int c = 0; c < 3; ++c) x[c] = t >= d ? part[c][t - d] : 0;
    __syncthreads();
    for (int c = 0; c < 3; ++c) part[c][t] += x[c];       // wrapping: only the low 16 bits are kept
    __syncthreads();
  }
  for (int c = 0; c < 3; ++c) acc[c] = t ? part[c][t - 1] : 0;
  for (int k = k0; k < k1; ++k) {
    const int c = jp::component_of(g, k % g.bpm);
    const int d = (unsigned short)g.coef[(long long)k * 64];
    const int v = (c == 0 ? acc[0] : c == 1 ? acc[1] : acc[2]) + d;
    acc[0] = c == 0 ? v : acc[0];
    acc[1] = c == 1 ? v : acc[1];
    acc[2] = c == 2 ? v : acc[2];
    g.coef[(long long)k * 64] = (short)v;
  }
}

template <bool T, bool B>
void launch_sync(dim3 grid, size_t lds, hipStream_t stream, const Batch& a, const Workspace& w, int join) {
  hipLaunchKernelGGL((jpeg_sync_kernel<T, B>), grid, dim3(jp::RUN), lds, stream, a, w, join);
}
template <bool T, bool B>
void launch_write(dim3 grid, size_t lds, hipStream_t stream, const Batch& a, const Workspace& w) {
  hipLaunchKernelGGL((jpeg_write_kernel<T, B>), grid, dim3(jp::RUN), lds, stream, a, w);
}

}  // namespace

extern "C" int pmce_jpeg_parallel_run(void) { return jp::RUN; }

extern "C" int pmce_jpeg_parallel_stages(void) { return 4 + jp::JOIN_ROUNDS; }

extern "C" int pmce_jpeg_entropy_parallel(const unsigned char* data, long long n_bytes, const int* segments, int first_segment,
                                          int n_segments, const int* images, int n_images, const int* huffman, int n_huffman,
                                          short* coefficients, long long n_blocks, int* segment_status, int lds_tables, int subsequence,
                                          const int* offsets, int n_subsequences, int n_runs, void* workspace, long long workspace_bytes,
                                          int stage, hipStream_t stream) {
  PMCE_REQUIRE(data && segments && images && huffman && coefficients && segment_status && offsets && workspace,
               "jpeg_entropy_parallel: null pointer");
  PMCE_REQUIRE(n_bytes >= 1 && n_bytes <= 0x7fffffffll - 2 * je::WINDOW, "jpeg_entropy_parallel: need 1 .. 2^31 - 129 bytes of files (got %lld)",
               n_bytes);
  PMCE_REQUIRE(first_segment >= 0 && n_segments >= 1 && n_images >= 1 && n_huffman >= 1,
               "jpeg_entropy_parallel: need first_segment >= 0 and at least one segment, image and Huffman table (got %d, %d, %d, %d)",
               first_segment, n_segments, n_images, n_huffman);
  PMCE_REQUIRE(((uintptr_t)coefficients & 15) == 0, "jpeg_entropy_parallel: the coefficient buffer must be 16-byte aligned");
  PMCE_REQUIRE(n_blocks >= 1 && n_blocks <= (1ll << 40), "jpeg_entropy_parallel: need 1 .. 2^40 coefficient blocks (got %lld)", n_blocks);
  PMCE_REQUIRE(subsequence >= jp::MIN_SUBSEQUENCE && subsequence <= jp::MAX_SUBSEQUENCE && subsequence % 4 == 0,
               "jpeg_entropy_parallel: subsequence must be a multiple of 4 in %d .. %d (got %d)", jp::MIN_SUBSEQUENCE, jp::MAX_SUBSEQUENCE,
               subsequence);
  PMCE_REQUIRE(n_subsequences >= n_segments && n_runs >= n_segments && n_runs <= n_subsequences,
               "jpeg_entropy_parallel: every segment has a subsequence and a run: need n_subsequences >= n_runs >= n_segments (got %d, %d, %d)",
               n_subsequences, n_runs, n_segments);
  PMCE_REQUIRE(((uintptr_t)workspace & 7) == 0, "jpeg_entropy_parallel: the workspace must be 8-byte aligned");
  const long long need = (long long)n_subsequences * jp::SUB_BYTES + (long long)n_runs * jp::RUN_BYTES + (long long)n_segments * 8;
  PMCE_REQUIRE(workspace_bytes >= need, "jpeg_entropy_parallel: the workspace needs %lld bytes (%d per subsequence, %d per run, 8 per segment; got %lld)",
               need, jp::SUB_BYTES, jp::RUN_BYTES, workspace_bytes);
  const int stages = 4 + jp::JOIN_ROUNDS;
  PMCE_REQUIRE(stage >= -1 && stage < stages, "jpeg_entropy_parallel: stage must be -1 (all) or 0 .. %d (got %d)", stages - 1, stage);

  Workspace w;
  w.n_sub = n_subsequences;
  w.n_runs = n_runs;
  w.entry = static_cast<jp::State*>(workspace);
  w.exit = w.entry + n_subsequences;
  w.border = w.exit + n_subsequences;
  w.rounds = reinterpret_cast<int*>(w.border + 2 * (size_t)n_runs);
  w.blocks = w.rounds + (1 + jp::JOIN_ROUNDS) * (size_t)n_runs;
  w.block0 = w.blocks + n_subsequences;
  w.status = w.block0 + n_subsequences;
  w.dc_end = w.status + n_subsequences;
  w.serial = w.dc_end + n_subsequences;
  w.stop = w.serial + n_segments;
  const Batch a = {data, n_bytes, segments, first_segment, n_segments, images, n_images, huffman, n_huffman, coefficients, n_blocks, offsets,
                   subsequence};

  const bool tables = n_huffman <= MAX_LDS_TABLES && lds_tables;
  const size_t table_bytes = tables ? (size_t)n_huffman * je::HUFF_WORDS * sizeof(int) : 0;
  const size_t run_bytes = (size_t)jp::RUN * subsequence + NEAR_SLACK;
  const bool bytes = table_bytes + run_bytes <= (size_t)MAX_DYNAMIC_LDS;
  const size_t lds = table_bytes + (bytes ? run_bytes : 0);
  const dim3 runs((unsigned)n_runs), segs((unsigned)n_segments);
  for (int st = stage < 0 ? 0 : stage; st <= (stage < 0 ? stages - 1 : stage); ++st) {
    if (st == 0) {
      const hipError_t rc = hipMemsetAsync(coefficients, 0, (size_t)n_blocks * 64 * sizeof(short), stream);
      if (rc != hipSuccess) {
        pmce_set_error("jpeg_entropy_parallel: hipMemsetAsync failed: %s", hipGetErrorString(rc));
        return PMCE_ERR_LAUNCH;
      }
    }
    if (st <= jp::JOIN_ROUNDS) {
      if (tables) bytes ? launch_sync<true, true>(runs, lds, stream, a, w, st) : launch_sync<true, false>(runs, lds, stream, a, w, st);
      else bytes ? launch_sync<false, true>(runs, lds, stream, a, w, st) : launch_sync<false, false>(runs, lds, stream, a, w, st);
    } else if (st == jp::JOIN_ROUNDS + 1) {
      hipLaunchKernelGGL(jpeg_place_kernel, segs, dim3(jp::RUN), 0, stream, a, w);
    } else if (st == jp::JOIN_ROUNDS + 2) {
      if (tables) bytes ? launch_write<true, true>(runs, lds, stream, a, w) : launch_write<true, false>(runs, lds, stream, a, w);
      else bytes ? launch_write<false, true>(runs, lds, stream, a, w) : launch_write<false, false>(runs, lds, stream, a, w);
    } else {
      hipLaunchKernelGGL(jpeg_dc_kernel, segs, dim3(jp::RUN), 0, stream, a, w, segment_status);
    }
    const int rc = pmce_check_launch("jpeg_entropy_parallel");
    if (rc) return rc;
  }
  return 0;
}
