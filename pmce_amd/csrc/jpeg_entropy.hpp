// The entropy decoder of the baseline JPEG reader (ITU-T T.81 Annex F.2.2), written once for the device (jpeg.hip: one lane per
// restart interval) and for the host (scripts/jpeg_entropy_host.cpp, which runs this body over intact, shortened and damaged
// streams between guard regions).  The record layouts are those of include/pmce_hip.h; pmce_amd/jpeg.py writes them.
//
// What the body guarantees whatever the stream's bytes say, given records that pass check_segment():
//   * it reads data[begin, end) of its segment and nothing else of `data`;
//   * it writes the 64 coefficients of blocks block0 + mcu * blocks_per_mcu + (0 .. blocks_per_mcu), mcu in [mcu0, mcu0 + count),
//     all below n_blocks, and nothing else of `coef`;
//   * it ends: every step of every loop consumes a coefficient position or a block.
// Beyond the end of the segment the reader supplies zero bits; the first such bit that a symbol or a value CONSUMES sets
// JPEG_STATUS_TRUNCATED (bits merely looked at by the lookahead do not).  A marker inside the segment acts as its end and sets
// JPEG_STATUS_CORRUPT when the decoder runs into it, as do a code that is in no table and a run that passes coefficient 63.  With a
// status bit set the segment ends after the block at hand; what it has not decoded stays zero.
//
// Two optional pieces of scratch memory change where the body's loads and stores go, not what it computes (on the device both are LDS:
// a wave's loads wait for its older stores to global memory, so a lane that stored every coefficient as it came and read every byte
// from global memory stood still for a store's round trip per symbol):
//   window   WINDOW bytes through which the segment's bytes are read, refilled 16 aligned bytes at a time - bytes outside
//            [begin, end) are never loaded, the pieces at the segment's two ends are read byte by byte;
//   block    64 coefficients in which a block is put together; its non-zero rows of 8 leave as 16-byte stores when the block ends.
// The template argument SCRATCH selects the form (false: the two pointers are not used); the host program runs both.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#else
#define JPEG_HD inline
#endif

namespace jpeg_entropy {

constexpr int IMG_WORDS = 24;        // image record, int32 words (pmce_hip.h)
constexpr int SEG_WORDS = 5;         // (image, first byte, end byte, first MCU, MCU count)
constexpr int HUFF_WORDS = 546;      // maxcode[17] | valoff[17] | values[256] | look[256]
constexpr int HUFF_MAXCODE = 0, HUFF_VALOFF = 17, HUFF_VALUES = 34, HUFF_LOOK = 290;
constexpr int LOOK_BITS = 8;
constexpr int WINDOW = 64;            // bytes of a lane's window on its segment (a multiple of 16)

constexpr int STATUS_TRUNCATED = 1, STATUS_CORRUPT = 2, STATUS_RECORD = 4;

// words of the image record
enum { IM_WIDTH = 0, IM_HEIGHT, IM_NCOMP, IM_H, IM_V, IM_MCUS_X, IM_MCUS_Y, IM_RESTART, IM_QUANT /* 8..10 */, IM_DC = 11 /* 11..13 */,
       IM_AC = 14 /* 14..16 */, IM_BLOCK0 = 17, IM_PLANE0 = 18, IM_SEG0 = 19, IM_NSEG = 20, IM_BLOCKS_PER_MCU = 21 };

// natural (row-major) index of the k-th coefficient in zigzag order, T.81 figure A.6
JPEG_HD int natural_index(int k) {
  constexpr unsigned char t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return t[k & 63];
}

struct Reader {
  const unsigned char* data;
  int begin, pos, end;
  uint32_t acc;      // the low `nbits` bits are the stream's next bits, most significant first
  int nbits;
  int pad;           // how many of them (the lowest) are zero bits from beyond the end
  int marker;        // the end was a marker inside the segment, not the segment's end
  int status;
  unsigned char* window;      // SCRATCH only
  int wlo;                    // the window holds data[wlo, wlo + WINDOW), as far as that lies inside [begin, end)
};

JPEG_HD void reader_init(Reader& r, const unsigned char* data, int begin, int end, unsigned char* window) {
  r.data = data;
  r.begin = r.pos = begin;
  r.end = end;
  r.acc = 0;
  r.nbits = r.pad = r.marker = r.status = 0;
  r.window = window;
  r.wlo = end;       // empty: nothing of [begin, end) lies in [end, end + WINDOW)
}

// The window moves to the 16-byte aligned address at or below data + pos.
JPEG_HD void refill(Reader& r, int pos) {
  r.wlo = pos - (int)((uintptr_t)(r.data + pos) & 15);
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
  for (int j = 0; j < WINDOW; j += 16) {
    const int p = r.wlo + j;
    if (p >= r.begin && p + 16 <= r.end) {
      memcpy(r.window + j, __builtin_assume_aligned(r.data + p, 16), 16);
    } else {
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
      for (int k = 0; k < 16; ++k) r.window[j + k] = (p + k >= r.begin && p + k < r.end) ? r.data[p + k] : (unsigned char)0;
    }
  }
}

// byte `pos` of the segment, begin <= pos < end
template <bool SCRATCH>
JPEG_HD uint32_t byte_at(Reader& r, int pos) {
  if (!SCRATCH) return r.data[pos];
  if (pos < r.wlo || pos - r.wlo >= WINDOW) refill(r, pos);
  return r.window[pos - r.wlo];
}

// at least 25 bits afterwards
template <bool SCRATCH>
JPEG_HD void fill(Reader& r) {
  while (r.nbits <= 24) {
    uint32_t b = 0;
    if (r.pos < r.end) {
      b = byte_at<SCRATCH>(r, r.pos++);
      if (b == 0xFF) {
        if (r.pos < r.end && byte_at<SCRATCH>(r, r.pos) == 0) {
          ++r.pos;                     // the stuffed byte
        } else {
          if (r.pos < r.end) r.marker = 1;      // FF xx, xx != 0; a lone FF as the last byte is a stream cut short
          r.pos = r.end;
          b = 0;
          r.pad += 8;
        }
      }
    } else {
      r.pad += 8;
    }
    r.acc = (r.acc << 8) | b;
    r.nbits += 8;
  }
}

JPEG_HD uint32_t peek(const Reader& r, int n) { return (r.acc >> (r.nbits - n)) & ((1u << n) - 1u); }

JPEG_HD void consume(Reader& r, int n) {
  r.nbits -= n;
  if (r.nbits < r.pad) {
    r.status |= r.marker ? STATUS_CORRUPT : STATUS_TRUNCATED;
    r.pad = r.nbits;
  }
}

// one Huffman symbol (0..255), or -1 with STATUS_CORRUPT for a code of no table entry
template <bool SCRATCH>
JPEG_HD int decode_symbol(Reader& r, const int* __restrict__ tab) {
  fill<SCRATCH>(r);
  const int e = tab[HUFF_LOOK + peek(r, LOOK_BITS)];
  if (e) {
    consume(r, e >> 8);
    return e & 255;
  }
  for (int l = LOOK_BITS + 1; l <= 16; ++l) {
    const int code = (int)peek(r, l);
    if (code <= tab[HUFF_MAXCODE + l]) {          // maxcode is -1 for a length without codes
      consume(r, l);
      return tab[HUFF_VALUES + ((code + tab[HUFF_VALOFF + l]) & 255)];
    }
  }
  r.status |= STATUS_CORRUPT;
  return -1;
}

// s bits (0..16) as the signed value of T.81 F.2.2.1 (EXTEND)
template <bool SCRATCH>
JPEG_HD int receive_extend(Reader& r, int s) {
  if (s == 0) return 0;
  fill<SCRATCH>(r);
  const int v = (int)peek(r, s);
  consume(r, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: its 64 coefficients in natural order at `out` (already zero).  Returns the new DC prediction.  With SCRATCH (`block`: 64 zeros,
// left as 64 zeros) the coefficients are collected there and the rows of 8 that received one are then copied to `out`.
template <bool SCRATCH>
JPEG_HD int decode_block(Reader& r, const int* __restrict__ dc, const int* __restrict__ ac, int pred, short* __restrict__ out,
                         short* __restrict__ block) {
  short* dst = SCRATCH ? block : out;
  const int t = decode_symbol<SCRATCH>(r, dc);
  if (t < 0) return pred;
  if (t > 15) {
    r.status |= STATUS_CORRUPT;
    return pred;
  }
  pred = (int)(short)(pred + receive_extend<SCRATCH>(r, t));        // kept to 16 bits: a valid stream never leaves them
  dst[0] = (short)pred;
  unsigned rows = 1;
  int k = 1;
  while (k < 64) {
    const int rs = decode_symbol<SCRATCH>(r, ac);
    if (rs < 0) break;
    const int run = rs >> 4, s = rs & 15;
    if (s == 0) {
      if (run != 15) break;      // EOB
      k += 16;                   // ZRL
      continue;
    }
    k += run;
    if (k > 63) {
      r.status |= STATUS_CORRUPT;
      break;
    }
    const int n = natural_index(k);
    dst[n] = (short)receive_extend<SCRATCH>(r, s);
    rows |= 1u << (n >> 3);
    ++k;
  }
  if (SCRATCH) {
    for (int row = 0; row < 8; ++row)
      if (rows & (1u << row)) {
        memcpy(__builtin_assume_aligned(out + 8 * row, 16), __builtin_assume_aligned(block + 8 * row, 16), 16);
        memset(__builtin_assume_aligned(block + 8 * row, 16), 0, 16);
      }
  }
  return pred;
}

// Is an image record one whose geometry the three stages can follow?  (pmce_amd/jpeg.py never writes one that is not.)
JPEG_HD bool check_image(const int* __restrict__ im) {
  const int ncomp = im[IM_NCOMP], h = im[IM_H], v = im[IM_V];
  if (!(ncomp == 1 || ncomp == 3) || h < 1 || h > 2 || v < 1 || v > 2 || (ncomp == 1 && h * v != 1)) return false;
  if (im[IM_BLOCKS_PER_MCU] != (ncomp == 1 ? 1 : h * v + 2)) return false;
  if (im[IM_MCUS_X] < 1 || im[IM_MCUS_X] > 2048 || im[IM_MCUS_Y] < 1 || im[IM_MCUS_Y] > 2048) return false;
  return im[IM_BLOCK0] >= 0 && im[IM_PLANE0] >= 0;
}

// Do the records of segment `seg` fit the arrays they index?
JPEG_HD bool check_segment(const int* __restrict__ seg, long long n_bytes, const int* __restrict__ images, int n_images, int n_huffman,
                           long long n_blocks) {
  const int image = seg[0], begin = seg[1], end = seg[2], mcu0 = seg[3], count = seg[4];
  if (image < 0 || image >= n_images || begin < 0 || end < begin || end > n_bytes || mcu0 < 0 || count < 0) return false;
  const int* im = images + (long long)image * IMG_WORDS;
  if (!check_image(im)) return false;
  const long long mcus = (long long)im[IM_MCUS_X] * im[IM_MCUS_Y];
  if ((long long)mcu0 + count > mcus || im[IM_BLOCK0] + mcus * im[IM_BLOCKS_PER_MCU] > n_blocks) return false;
  for (int c = 0; c < im[IM_NCOMP]; ++c)
    if (im[IM_DC + c] < 0 || im[IM_DC + c] >= n_huffman || im[IM_AC + c] < 0 || im[IM_AC + c] >= n_huffman) return false;
  return true;
}

// The whole segment -> its status word.  `coef` is 16-byte aligned.  SCRATCH: `window` (WINDOW bytes) and `block` (64 zeroed
// coefficients, 16-byte aligned) are the scratch of the header's comment.
template <bool SCRATCH>
JPEG_HD int decode_segment(const unsigned char* __restrict__ data, long long n_bytes, const int* __restrict__ seg,
                           const int* __restrict__ images, int n_images, const int* __restrict__ huffman, int n_huffman,
                           short* __restrict__ coef, long long n_blocks, unsigned char* window, short* __restrict__ block) {
  if (!check_segment(seg, n_bytes, images, n_images, n_huffman, n_blocks)) return STATUS_RECORD;
  const int* im = images + (long long)seg[0] * IMG_WORDS;
  const int ncomp = im[IM_NCOMP], bpm = im[IM_BLOCKS_PER_MCU], luma_blocks = ncomp == 1 ? 1 : im[IM_H] * im[IM_V];
  Reader r;
  reader_init(r, data, seg[1], seg[2], window);
  int pred0 = 0, pred1 = 0, pred2 = 0;
  const int dc0 = im[IM_DC] * HUFF_WORDS, ac0 = im[IM_AC] * HUFF_WORDS;
  const int dc1 = im[IM_DC + (ncomp == 3 ? 1 : 0)] * HUFF_WORDS, ac1 = im[IM_AC + (ncomp == 3 ? 1 : 0)] * HUFF_WORDS;
  const int dc2 = im[IM_DC + (ncomp == 3 ? 2 : 0)] * HUFF_WORDS, ac2 = im[IM_AC + (ncomp == 3 ? 2 : 0)] * HUFF_WORDS;
  const int mcu_end = seg[3] + seg[4];
  for (int mcu = seg[3]; mcu < mcu_end && !r.status; ++mcu) {
    short* out = coef + ((long long)im[IM_BLOCK0] + (long long)mcu * bpm) * 64;
    for (int b = 0; b < bpm && !r.status; ++b, out += 64) {           // the luma blocks, then Cb, then Cr
      const int c = b < luma_blocks ? 0 : b - luma_blocks + 1;
      const int pred = decode_block<SCRATCH>(r, huffman + (c == 0 ? dc0 : c == 1 ? dc1 : dc2), huffman + (c == 0 ? ac0 : c == 1 ? ac1 : ac2),
                                             c == 0 ? pred0 : c == 1 ? pred1 : pred2, out, block);
      if (c == 0) pred0 = pred;
      else if (c == 1) pred1 = pred;
      else pred2 = pred;
    }
  }
  return r.status;
}

}  // namespace jpeg_entropy
