// The entropy decoder of the JPEG reader (pmce_amd/csrc/jpeg_entropy.hpp, the body the device kernel wraps) run on the host over
// intact, shortened and damaged streams, with its output between guard regions.
//
//   c++ -std=c++17 -O1 -g -I pmce_amd/csrc scripts/jpeg_entropy_host.cpp -o jpeg_entropy_host      (add -fsanitize=address,undefined)
//   ./jpeg_entropy_host records.bin [bit-flip variants, default 3000]
//
// records.bin is what pmce_amd.jpeg.dump_records writes.  Three streams per segment:
//   1. as it is: status 0, and the coefficients the dump carries (the numpy restatement's), if it carries any;
//   2. cut short at every length 0 .. n - 1;
//   3. copies with one bit flipped, chosen by a fixed-seed generator.
// All of it twice: the body's direct form, and the form the device runs (bytes through a 64-byte window, each block collected in
// scratch memory).  Every run gets the segment's bytes alone, at a changing alignment (so that a sanitizer sees any read outside [begin, end)),
// must return a status made of the known bits, must leave every coefficient outside the segment's own blocks zero, and must leave
// the guards in front of and behind the coefficient buffer untouched.  Exit status 0: all of that held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_entropy.hpp"

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

struct Runner {
  const Records& r;
  std::vector<short> buf;          // guard | coefficients | guard
  long long runs = 0, flagged = 0;
  bool scratch = false;
  explicit Runner(const Records& rec) : r(rec), buf(2 * GUARD + (size_t)rec.n_blocks * 64) {}
  short* coef() { return buf.data() + GUARD; }

  // Decode segment s from `bytes` (its own stream, possibly cut or damaged).  Returns the status, or -1 after printing what broke.
  int run(int s, const unsigned char* bytes, int n, const char* what) {
    for (size_t i = 0; i < GUARD; ++i) buf[i] = buf[buf.size() - 1 - i] = GUARD_WORD;
    memset(coef(), 0, (size_t)r.n_blocks * 64 * sizeof(short));
    // The stream with nothing readable around it: under AddressSanitizer the bytes in front of and behind it are poisoned (without it
    // they hold FF bytes, which the body must never see either).  AddressSanitizer poisons whole 8-byte granules only, so in front of
    // a stream that does not begin on a granule up to 7 bytes stay addressable: every other run therefore places the stream on a
    // granule boundary (alignments 0 and 8 of the window's 16, where the whole front is poisoned), the runs between them walk through
    // all 16 alignments.
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
    // both forms of the body: the direct one, and the one that reads through a window and collects each block in scratch memory
    // (the device's); the scratch sits in heap blocks of exactly its size
    int st;
    if (scratch) {
      unsigned char* window = (unsigned char*)aligned_alloc(16, je::WINDOW);
      short* block = (short*)aligned_alloc(16, 64 * sizeof(short));
      memset(block, 0, 64 * sizeof(short));
      st = je::decode_segment<true>(heap, n > 0 ? n : 1, seg, r.images.data(), (int)r.n_images, r.huffman.data(), (int)r.n_huffman, coef(),
                                    r.n_blocks, window, block);
      for (int i = 0; i < 64; ++i)
        if (block[i] != 0) {
          printf("FAIL %s: segment %d left a coefficient in the scratch block\n", what, s);
          st = -1;
          break;
        }
      free(window);
      free(block);
      if (st < 0) {
        ASAN_UNPOISON_MEMORY_REGION(raw, size);
        free(raw);
        return -1;
      }
    } else {
      st = je::decode_segment<false>(heap, n > 0 ? n : 1, seg, r.images.data(), (int)r.n_images, r.huffman.data(), (int)r.n_huffman, coef(),
                                     r.n_blocks, nullptr, nullptr);
    }
    ASAN_UNPOISON_MEMORY_REGION(raw, size);
    free(raw);
    ++runs;
    flagged += st != 0;
    if (st & ~(je::STATUS_TRUNCATED | je::STATUS_CORRUPT)) {
      printf("FAIL %s: segment %d returned status %d\n", what, s, st);
      return -1;
    }
    for (size_t i = 0; i < GUARD; ++i)
      if (buf[i] != GUARD_WORD || buf[buf.size() - 1 - i] != GUARD_WORD) {
        printf("FAIL %s: segment %d wrote into a guard region\n", what, s);
        return -1;
      }
    const int* im = &r.images[(size_t)seg[0] * je::IMG_WORDS];
    const long long first = ((long long)im[je::IM_BLOCK0] + (long long)seg[3] * im[je::IM_BLOCKS_PER_MCU]) * 64;
    const long long last = first + (long long)seg[4] * im[je::IM_BLOCKS_PER_MCU] * 64;
    for (long long i = 0; i < r.n_blocks * 64; ++i)
      if ((i < first || i >= last) && coef()[i] != 0) {
        printf("FAIL %s: segment %d wrote coefficient %lld, outside its blocks [%lld, %lld)\n", what, s, i, first / 64, last / 64);
        return -1;
      }
    return st;
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

  for (int form = 0; form < 2; ++form) {
  Runner run(r);
  run.scratch = form == 1;
  // 1. intact
  long long compared = 0;
  for (int s = 0; s < S; ++s) {
    const int* seg = &r.segments[(size_t)s * je::SEG_WORDS];
    const int st = run.run(s, r.data.data() + seg[1], seg[2] - seg[1], "intact");
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
      if (run.run(s, r.data.data() + seg[1], n, "cut") < 0) return 1;
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
    if (run.run(s, copy.data(), n, "bit flip") < 0) return 1;
    ++flips;
  }
  printf("ok (%s): %d segments; intact %lld runs, %lld coefficients compared; cut %lld runs (%lld flagged); bit flips %lld runs (%lld flagged); "
         "guards untouched\n",
         form ? "window and block scratch" : "direct", S, intact_runs, compared, cut_runs, cut_flagged, flips, run.flagged - cut_flagged);
  }
  return 0;
}
