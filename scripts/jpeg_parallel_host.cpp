// The parallel entropy decoder of the JPEG reader (pmce_amd/csrc/jpeg_parallel.hpp, the body the device kernels wrap) emulated on the
// host: lanes run one after the other, and every result is compared with the serial body's (jpeg_entropy.hpp, decode_segment<false>)
// on the same bytes - coefficients and status word, for intact, shortened and damaged streams.
//
//   c++ -std=c++17 -O1 -g -I pmce_amd/csrc scripts/jpeg_parallel_host.cpp -o jpeg_parallel_host      (add -fsanitize=address,undefined)
//   ./jpeg_parallel_host records.bin [bit-flip variants, default 3000]
//
// records.bin is what pmce_amd.jpeg.dump_records writes.  Three streams per segment: as it is (status 0 and the dump's coefficients),
// cut short at every length, and copies with one bit flipped (fixed seed).  Each of them at S = 4, 8, 12, 64, 256 and one larger than
// the segment, with the lanes of a synchronise round visited forwards, backwards (every lane then sees its neighbour's exit of the
// round before, as on the device) or in a fixed shuffled order (the intact streams in all three, the others in turn), and with the
// device's structure: runs of `run`
// subsequences that reach their fixed point alone from a guessed first entry, JOIN_ROUNDS rounds that replace those guesses by the
// neighbour's exit, the check of the fixed-point condition and the serial hand-off when it fails (run = 5 makes the hand-off happen,
// run = jpeg_parallel::RUN is the device's).  Every run gets the segment's bytes alone with nothing readable around them, and its
// coefficients between guard regions.  Exit status 0: every run equalled the serial body, no guard was touched, and no fixed point
// took more rounds than it has lanes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_parallel.hpp"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#endif
#endif
#ifndef ASAN_POISON_MEMORY_REGION
#define ASAN_POISON_MEMORY_REGION(addr, size) ((void)(addr), (void)(size))
#define ASAN_UNPOISON_MEMORY_REGION(addr, size) ((void)(addr), (void)(size))
#endif

namespace je = jpeg_entropy;
namespace jp = jpeg_parallel;

namespace {

constexpr size_t GUARD = 4096;             // int16 words on either side
constexpr short GUARD_WORD = 0x5A5A;

struct Records {
  long long n_bytes = 0, n_images = 0, n_quant = 0, n_huffman = 0, n_segments = 0, n_blocks = 0, has_coef = 0;
  std::vector<int> images, huffman, segments;
  std::vector<unsigned short> quant;
  std::vector<unsigned char> data;
  std::vector<short> coef;
};

template <class T>
bool read_array(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool load(const char* path, Records& r) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  char magic[8];
  long long head[7];
  bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, "PMCEJPG1", 8) == 0 && fread(head, sizeof(long long), 7, f) == 7;
  if (ok) {
    r.n_bytes = head[0], r.n_images = head[1], r.n_quant = head[2], r.n_huffman = head[3], r.n_segments = head[4], r.n_blocks = head[5],
    r.has_coef = head[6];
    ok = r.n_bytes > 0 && r.n_bytes < (1ll << 31) && r.n_images > 0 && r.n_images < (1 << 20) && r.n_quant > 0 && r.n_quant < (1 << 20) &&
         r.n_huffman > 0 && r.n_huffman < (1 << 20) && r.n_segments > 0 && r.n_segments < (1 << 24) && r.n_blocks > 0 &&
         r.n_blocks < (1 << 24);
  }
  ok = ok && read_array(f, r.images, (size_t)r.n_images * je::IMG_WORDS) && read_array(f, r.huffman, (size_t)r.n_huffman * je::HUFF_WORDS) &&
       read_array(f, r.segments, (size_t)r.n_segments * je::SEG_WORDS) && read_array(f, r.quant, (size_t)r.n_quant * 64) &&
       read_array(f, r.data, (size_t)r.n_bytes) && (!r.has_coef || read_array(f, r.coef, (size_t)r.n_blocks * 64));
  fclose(f);
  return ok;
}

// the order in which a round visits lanes [0, n): 0 forwards, 1 backwards, 2 a fixed shuffle
void visit_order(int order, int n, std::vector<int>& v) {
  v.resize((size_t)n);
  for (int i = 0; i < n; ++i) v[(size_t)i] = order == 1 ? n - 1 - i : i;
  if (order == 2) {
    unsigned long long rng = 0x2545F4914F6CDD1Dull;
    for (int i = n - 1; i > 0; --i) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(v[(size_t)i], v[(size_t)((rng >> 33) % (unsigned)(i + 1))]);
    }
  }
}

struct Emulation {
  std::vector<jp::State> entry, exit;
  std::vector<int> blocks, error;
  std::vector<int> order_buf;
  long long max_rounds_over = 0, handed_off = 0, decodes = 0;

  // lanes [first, first + n) of one run to their fixed point, lane `first` entering with `e0`.  fresh: no lane has decoded yet.
  bool fixed_point(const jp::Segment& g, int first, int n, jp::State e0, bool fresh, int order) {
    visit_order(order, n, order_buf);
    jp::Lane lane;
    if (fresh)
      for (int k : order_buf) {
        const int i = first + k;
        entry[(size_t)i] = jp::guess(g, i);
        jp::decode_subsequence<false>(g, i, entry[(size_t)i], 0, lane);
        exit[(size_t)i] = lane.exit, blocks[(size_t)i] = lane.blocks, error[(size_t)i] = lane.error;
        ++decodes;
      }
    for (int round = 0;; ++round) {
      bool changed = false;
      for (int k : order_buf) {
        const int i = first + k;
        const jp::State e = k == 0 ? e0 : exit[(size_t)i - 1];
        if (e == entry[(size_t)i]) continue;
        entry[(size_t)i] = e;
        jp::decode_subsequence<false>(g, i, e, 0, lane);
        exit[(size_t)i] = lane.exit, blocks[(size_t)i] = lane.blocks, error[(size_t)i] = lane.error;
        changed = true;
        ++decodes;
      }
      if (!changed) return true;
      if (round >= n) {
        ++max_rounds_over;
        return false;
      }
    }
  }

  // the whole segment -> status; -1: a fixed point needed more rounds than it has lanes
  int run(const jp::Segment& g, const int* seg, const Records& r, const unsigned char* heap, int n_bytes, short* coef, int run_len, int order) {
    const int n = g.n_sub, runs = (n + run_len - 1) / run_len;
    entry.assign((size_t)n, 0), exit.assign((size_t)n, 0), blocks.assign((size_t)n, 0), error.assign((size_t)n, 0);
    std::vector<jp::State> border((size_t)runs), next;
    for (int q = 0; q < runs; ++q) {
      const int first = q * run_len, len = std::min(run_len, n - first);
      if (!fixed_point(g, first, len, jp::guess(g, first), true, order)) return -1;
      border[(size_t)q] = exit[(size_t)(first + len - 1)];
    }
    for (int j = 0; j < jp::JOIN_ROUNDS; ++j) {
      next = border;
      for (int q = 1; q < runs; ++q) {
        const int first = q * run_len, len = std::min(run_len, n - first);
        if (!fixed_point(g, first, len, border[(size_t)q - 1], false, order)) return -1;
        next[(size_t)q] = exit[(size_t)(first + len - 1)];
      }
      border = next;
    }
    bool ok = entry[0] == jp::guess(g, 0);
    for (int i = 1; i < n; ++i) ok = ok && entry[(size_t)i] == exit[(size_t)i - 1];
    if (!ok) {                                            // the serial hand-off
      ++handed_off;
      return je::decode_segment<false>(heap, n_bytes > 0 ? n_bytes : 1, seg, r.images.data(), (int)r.n_images, r.huffman.data(),
                                       (int)r.n_huffman, coef, r.n_blocks, nullptr, nullptr);
    }
    visit_order(order, n, order_buf);
    std::vector<int> block0((size_t)n);
    int sum = 0;
    for (int i = 0; i < n; ++i) {
      block0[(size_t)i] = sum;
      sum = std::min(sum + blocks[(size_t)i], jp::BLOCK_CAP);
    }
    int status = 0, dc_end = 0;
    const int stop = jp::first_error(error.data(), n);    // the lanes behind the first real code error are not run
    jp::Lane lane;
    for (int i : order_buf) {
      if (i > stop) continue;
      jp::decode_subsequence<true>(g, i, entry[(size_t)i], block0[(size_t)i], lane);
      status |= lane.status;
      dc_end = std::max(dc_end, lane.dc_end);
    }
    jp::dc_scan(g, dc_end);
    return status;
  }
};

struct Runner {
  const Records& r;
  std::vector<short> buf, ref;     // guard | coefficients | guard
  Emulation emu;
  long long runs = 0, flagged = 0, lanes = 0;
  explicit Runner(const Records& rec) : r(rec), buf(2 * GUARD + (size_t)rec.n_blocks * 64), ref(buf.size()) {}
  short* coef() { return buf.data() + GUARD; }

  bool guards_ok(const std::vector<short>& v) {
    for (size_t i = 0; i < GUARD; ++i)
      if (v[i] != GUARD_WORD || v[v.size() - 1 - i] != GUARD_WORD) return false;
    return true;
  }

  // Segment s from `bytes` (its own stream, possibly cut or damaged) at every S; all_orders: each in the three orders, else the orders
  // in turn.  Returns the serial status, or -1 after printing what broke.
  int run(int s, const unsigned char* bytes, int n, const char* what, bool all_orders) {
    // the stream with nothing readable around it (scripts/jpeg_entropy_host.cpp: poisoned under AddressSanitizer, FF bytes without)
    const size_t off = (runs & 1) ? (size_t)((runs >> 1) % 16) : (size_t)((runs >> 1) % 2) * 8, size = 16 + (((size_t)(n > 0 ? n : 1) + 15) / 16) * 16 + 16;
    unsigned char* raw = (unsigned char*)aligned_alloc(16, size);
    memset(raw, 0xFF, size);
    unsigned char* heap = raw + off;
    if (n > 0) memcpy(heap, bytes, (size_t)n);
    ASAN_POISON_MEMORY_REGION(raw, off & ~(size_t)7);
    ASAN_POISON_MEMORY_REGION(heap + n, size - off - (size_t)n);
    int seg[je::SEG_WORDS];
    memcpy(seg, &r.segments[(size_t)s * je::SEG_WORDS], sizeof(seg));
    seg[1] = 0;
    seg[2] = n;
    const size_t words = (size_t)r.n_blocks * 64;
    for (size_t i = 0; i < GUARD; ++i) ref[i] = ref[ref.size() - 1 - i] = GUARD_WORD;
    memset(ref.data() + GUARD, 0, words * sizeof(short));
    const int want = je::decode_segment<false>(heap, n > 0 ? n : 1, seg, r.images.data(), (int)r.n_images, r.huffman.data(), (int)r.n_huffman,
                                               ref.data() + GUARD, r.n_blocks, nullptr, nullptr);
    int result = want;
    const int sizes[6] = {4, 8, 12, 64, 256, ((n + 4) / 4) * 4};
    const int run_lens[2] = {5, jp::RUN};
    for (int si = 0; si < 6 && result >= 0; ++si)
      for (int order = all_orders ? 0 : (int)((runs + si) % 3), last = all_orders ? 2 : order; order <= last && result >= 0; ++order)
        for (int ri = (int)((runs + si + order) & 1), once = 0; once < 1 && result >= 0; ++once) {      // the two run lengths in turn
          for (size_t i = 0; i < GUARD; ++i) buf[i] = buf[buf.size() - 1 - i] = GUARD_WORD;
          memset(coef(), 0, words * sizeof(short));
          jp::Segment g;
          jp::segment_init(g, heap, seg, r.images.data(), r.huffman.data(), coef(), sizes[si]);
          lanes += g.n_sub;
          const int got = emu.run(g, seg, r, heap, n, coef(), run_lens[ri], order);
          if (got < 0) {
            printf("FAIL %s: segment %d, S %d, order %d, run %d: a fixed point took more rounds than it has lanes\n", what, s, sizes[si], order,
                   run_lens[ri]);
            result = -1;
          } else if (got != want) {
            printf("FAIL %s: segment %d, S %d, order %d, run %d: status %d, the serial body's is %d\n", what, s, sizes[si], order, run_lens[ri], got,
                   want);
            result = -1;
          } else if (!guards_ok(buf)) {
            printf("FAIL %s: segment %d, S %d: wrote into a guard region\n", what, s, sizes[si]);
            result = -1;
          } else if (memcmp(coef(), ref.data() + GUARD, words * sizeof(short)) != 0) {
            size_t i = 0;
            while (coef()[i] == ref[GUARD + i]) ++i;
            printf("FAIL %s: segment %d (%d bytes), S %d, order %d, run %d: coefficient %zu of block %zu is %d, the serial body's is %d\n", what,
                   s, n, sizes[si], order, run_lens[ri], i % 64, i / 64, coef()[i], ref[GUARD + i]);
            result = -1;
          }
        }
    ASAN_UNPOISON_MEMORY_REGION(raw, size);
    free(raw);
    ++runs;
    flagged += want != 0;
    return result;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s records.bin [bit-flip variants]\n", argv[0]);
    return 2;
  }
  Records r;
  if (!load(argv[1], r)) {
    fprintf(stderr, "%s: not a records file of pmce_amd.jpeg.dump_records\n", argv[1]);
    return 2;
  }
  const long long variants = argc > 2 ? atoll(argv[2]) : 3000;
  const int S = (int)r.n_segments;
  for (int s = 0; s < S; ++s)
    if (!je::check_segment(&r.segments[(size_t)s * je::SEG_WORDS], r.n_bytes, r.images.data(), (int)r.n_images, (int)r.n_huffman,
                           r.n_blocks)) {
      printf("FAIL: segment %d's records do not fit their arrays\n", s);
      return 1;
    }
  Runner run(r);
  // 1. intact
  long long compared = 0;
  for (int s = 0; s < S; ++s) {
    const int* seg = &r.segments[(size_t)s * je::SEG_WORDS];
    const int st = run.run(s, r.data.data() + seg[1], seg[2] - seg[1], "intact", true);
    if (st != 0) {
      if (st > 0) printf("FAIL intact: segment %d has status %d\n", s, st);
      return 1;
    }
    if (r.has_coef) {
      const int* im = &r.images[(size_t)seg[0] * je::IMG_WORDS];
      const long long first = ((long long)im[je::IM_BLOCK0] + (long long)seg[3] * im[je::IM_BLOCKS_PER_MCU]) * 64;
      const long long count = (long long)seg[4] * im[je::IM_BLOCKS_PER_MCU] * 64;
      for (long long i = first; i < first + count; ++i)
        if (run.coef()[i] != r.coef[(size_t)i]) {
          printf("FAIL intact: segment %d, coefficient %lld of block %lld is %d, expected %d\n", s, i % 64, i / 64, run.coef()[i],
                 r.coef[(size_t)i]);
          return 1;
        }
      compared += count;
    }
  }
  const long long intact_runs = run.runs;
  // 2. cut short at every length
  for (int s = 0; s < S; ++s) {
    const int* seg = &r.segments[(size_t)s * je::SEG_WORDS];
    for (int n = 0; n < seg[2] - seg[1]; ++n)
      if (run.run(s, r.data.data() + seg[1], n, "cut", false) < 0) return 1;
  }
  const long long cut_runs = run.runs - intact_runs, cut_flagged = run.flagged;
  // 3. single bits flipped (a fixed seed: the same variants every run)
  unsigned long long rng = 0x9E3779B97F4A7C15ull;
  auto next = [&rng]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng >> 33);
  };
  std::vector<unsigned char> copy;
  long long flips = 0;
  for (long long i = 0; i < variants; ++i) {
    const int s = (int)(next() % (unsigned)S);
    const int* seg = &r.segments[(size_t)s * je::SEG_WORDS];
    const int n = seg[2] - seg[1];
    if (n == 0) continue;
    copy.assign(r.data.begin() + seg[1], r.data.begin() + seg[2]);
    const unsigned bit = next() % (unsigned)(8 * n);
    copy[bit >> 3] ^= (unsigned char)(1u << (bit & 7));
    if (run.run(s, copy.data(), n, "bit flip", false) < 0) return 1;
    ++flips;
  }
  printf("ok: %d segments; intact %lld streams, %lld coefficients compared; cut %lld streams (%lld flagged); bit flips %lld streams (%lld flagged); "
         "%lld lanes, %lld subsequence decodes, %lld serial hand-offs; every run equals the serial body; guards untouched\n",
         S, intact_runs, compared, cut_runs, cut_flagged, flips, run.flagged - cut_flagged, run.lanes, run.emu.decodes, run.emu.handed_off);
  return 0;
}
