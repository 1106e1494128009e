// The entropy decoder of the JPEG reader with many lanes per scan: the self-synchronising decode of Weissenberger and Schmidt
// ("Massively Parallel Huffman Decoding on GPUs", ICPP 2018) on T.81's baseline stream.  Written once for the device (jpeg.hip)
// and for the host (scripts/jpeg_parallel_host.cpp, which runs the lanes one after the other in several orders over intact,
// shortened and damaged streams and compares every result with jpeg_entropy.hpp's decode_segment).  Tables, status bits, records and
// check_segment are jpeg_entropy.hpp's; the bit reader is that header's with one addition, the raw position of the next bit.
//
// A segment (a restart interval, or the scan) is cut into subsequences of S bytes of its raw stream; subsequence i is lane i's.
// A decoder between two symbols is described by a State: the raw position of its next bit (byte and bit; stuffed 00 bytes count as
// bytes, and the position is the canonical one - the first byte with an unread bit, never the 00 of a stuffed pair), the block's index
// b within its MCU and the zigzag index z of the next coefficient (0: a DC symbol comes next).  Equal states have equal futures.
//
//   decode_subsequence<false>   lane i from an entry state to its exit state: the first state at or beyond the subsequence's end (the
//                               last subsequence of a segment has no end: its lane runs until the stream gives out), and the number of
//                               blocks it completed.  An entry at or beyond the end passes through.  Running out of stream ends the
//                               lane after the block at hand, as it ends the serial body, with the absorbing state ENDED, which
//                               every later lane passes on; a code error is noted and recovered from (see decode_subsequence).
//                               Nothing is written.
//   fixed point                 entry[0] = the segment's first bit in state (0, 0), entry[i] = exit[i - 1].  It is unique (by induction
//                               over i) and it is the serial decode; lanes start from the guess (first bit of the subsequence, 0, 0)
//                               and decode again whenever their entry changed, in any order and with stale neighbours.
//   decode_subsequence<true>    lane i once more from its true entry, with the absolute block it starts in (the exclusive sum of the
//                               completed blocks): coefficients in natural order, the DC DIFFERENCE at position 0, its status bits,
//                               and one past the last block whose DC it wrote.  The first code error ends it, as it ends the serial
//                               body; the lanes behind that lane are not run.  Blocks at or past the segment's limit (MCU count x
//                               blocks per MCU) are neither decoded nor written, so what trails the last block counts for nothing.
//   dc_scan                     per component, the inclusive sum of the differences over the blocks whose DC was written, in 16-bit
//                               wrapping arithmetic: the serial body's (short)(pred + diff) at every step, and associative.
//
// Bounds, whatever the bytes say: a lane reads data[begin, end) of its segment only, writes only blocks below the segment's limit, and
// every step of its loop consumes a bit, a coefficient position or a block.
#pragma once
#include "jpeg_entropy.hpp"

namespace jpeg_parallel {

namespace je = jpeg_entropy;

constexpr int RUN = 256;                  // subsequences per workgroup of the synchronise stage: one lane each
constexpr int MIN_SUBSEQUENCE = 4, MAX_SUBSEQUENCE = 1 << 16;      // S: a multiple of 4 in this range
constexpr int JOIN_ROUNDS = 2;            // rounds in which the runs' guessed first entries are replaced by their neighbours' exits
constexpr int BLOCK_CAP = 1 << 30;        // block counts saturate here, above every segment's limit (2048 x 2048 x 6)
constexpr int SUB_BYTES = 32;             // workspace per subsequence: entry, exit (8 each), blocks, first block, status, dc end (4 each)
constexpr int RUN_BYTES = 16 + 4 * (1 + JOIN_ROUNDS);      // per run: two border states, a round count per synchronising launch

typedef unsigned long long State;         // byte position (bits 0..30) | bit 32..34 | b 35..37 | z 38..43 | ENDED
constexpr State ENDED = 1ull << 63;

JPEG_HD State make_state(int pos, int bit, int b, int z) {
  return (State)(uint32_t)pos | ((State)bit << 32) | ((State)b << 35) | ((State)z << 38);
}
JPEG_HD int state_pos(State s) { return (int)(uint32_t)(s & 0x7fffffffu); }

// subsequences of a segment of n bytes: at least one (an empty segment still has a lane, which reports it as cut short)
JPEG_HD int subsequence_count(int n, int S) { return n <= S ? 1 : (int)(((long long)n + S - 1) / S); }

struct Reader {
  const unsigned char* data;
  int end;           // of the segment
  int tail;          // the raw position behind the last byte of the stream taken into acc (and its stuffed 00)
  int stop;          // nothing more is taken: the segment's end, a marker, or a lone FF was reached
  uint32_t acc;
  int nbits, pad, marker, status;        // as jpeg_entropy::Reader
  uint32_t stuffed;  // bit j: the (j + 1)-th last byte taken was an FF with its 00
  const unsigned char* near;             // a copy of data[near_lo, near_hi) in faster memory (the device's LDS), or near_lo == near_hi
  int near_lo, near_hi;
};

JPEG_HD uint32_t byte_at(const Reader& r, int pos) {
  if (pos >= r.near_lo && pos < r.near_hi) return r.near[pos - r.near_lo];
  return r.data[pos];
}

// jpeg_entropy::fill, which also keeps `tail` and `stuffed`
JPEG_HD void fill(Reader& r) {
  while (r.nbits <= 24) {
    uint32_t b = 0;
    if (!r.stop && r.tail < r.end) {
      b = byte_at(r, r.tail++);
      r.stuffed <<= 1;
      if (b == 0xFF) {
        if (r.tail < r.end && byte_at(r, r.tail) == 0) {
          ++r.tail;
          r.stuffed |= 1u;
        } else {
          if (r.tail < r.end) r.marker = 1;
          --r.tail;                    // the FF is no data
          r.stuffed >>= 1;
          r.stop = 1;
          b = 0;
          r.pad += 8;
        }
      }
    } else {
      r.stop = 1;
      r.pad += 8;
    }
    r.acc = (r.acc << 8) | b;
    r.nbits += 8;
  }
}

JPEG_HD void reader_init(Reader& r, const unsigned char* data, int end, int pos, int bit, const unsigned char* near, int near_lo,
                         int near_hi) {
  r.data = data;
  r.end = end;
  r.tail = pos;
  r.stop = 0;
  r.acc = 0;
  r.nbits = r.pad = r.marker = r.status = 0;
  r.stuffed = 0;
  r.near = near;
  r.near_lo = near_lo;
  r.near_hi = near_hi;
  fill(r);
  r.nbits -= bit;                      // bit < 8: the part of the first byte that lies in front of the state
  if (r.nbits < r.pad) r.pad = r.nbits;
}

// the canonical raw position of the next bit (meaningful while no status bit is set)
JPEG_HD void position(const Reader& r, int& pos, int& bit) {
  const int real = r.nbits - r.pad;
  if (real <= 0) {
    pos = r.tail;
    bit = 0;
    return;
  }
  const int k = (real + 7) >> 3;       // bytes of the stream in acc with an unread bit: 1 .. 4
  bit = (8 - (real & 7)) & 7;
  pos = r.tail - k - __builtin_popcount(r.stuffed & ((1u << k) - 1u));
}

JPEG_HD uint32_t peek(const Reader& r, int n) { return (r.acc >> (r.nbits - n)) & ((1u << n) - 1u); }

JPEG_HD void consume(Reader& r, int n) {
  r.nbits -= n;
  if (r.nbits < r.pad) {
    r.status |= r.marker ? je::STATUS_CORRUPT : je::STATUS_TRUNCATED;
    r.pad = r.nbits;
  }
}

// the codes longer than the lookahead: rare, and kept off the symbol loop's straight line (decode_symbol)
JPEG_HD int long_symbol(Reader& r, const int* __restrict__ tab) {
  for (int l = je::LOOK_BITS + 1; l <= 16; ++l) {
    const int code = (int)peek(r, l);
    if (code <= tab[je::HUFF_MAXCODE + l]) {
      consume(r, l);
      return tab[je::HUFF_VALUES + ((code + tab[je::HUFF_VALOFF + l]) & 255)];
    }
  }
  return -1;                           // a code of no table: nothing consumed, no status bit (the caller's)
}

JPEG_HD int decode_symbol(Reader& r, const int* __restrict__ tab) {
  fill(r);
  const int e = tab[je::HUFF_LOOK + peek(r, je::LOOK_BITS)];
  if (__builtin_expect(e != 0, 1)) {
    consume(r, e >> 8);
    return e & 255;
  }
  return long_symbol(r, tab);
}

JPEG_HD int receive_extend(Reader& r, int s) {
  if (s == 0) return 0;
  fill(r);
  const int v = (int)peek(r, s);
  consume(r, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// what a segment's lanes share
struct Segment {
  const unsigned char* data;
  int begin, end;                      // the segment's bytes
  int S, n_sub;
  int bpm, luma_blocks;
  const int* tables;                   // the batch's Huffman tables, wherever they lie
  int dc0, dc1, dc2, ac0, ac1, ac2;    // the tables of components 0, 1, 2 as offsets into them (a grey file: its one pair three times)
  int limit;                           // blocks of the segment: MCU count x blocks per MCU
  short* coef;                         // the segment's first block
  const unsigned char* near;
  int near_lo, near_hi;
};

// `seg` passes check_segment.  `huffman`: the tables, wherever they lie.
JPEG_HD void segment_init(Segment& g, const unsigned char* data, const int* __restrict__ seg, const int* __restrict__ images,
                          const int* huffman, short* coef, int S) {
  const int* im = images + (long long)seg[0] * je::IMG_WORDS;
  const int ncomp = im[je::IM_NCOMP];
  g.data = data;
  g.begin = seg[1];
  g.end = seg[2];
  g.S = S;
  g.n_sub = subsequence_count(seg[2] - seg[1], S);
  g.bpm = im[je::IM_BLOCKS_PER_MCU];
  g.luma_blocks = ncomp == 1 ? 1 : im[je::IM_H] * im[je::IM_V];
  g.tables = huffman;
  g.dc0 = im[je::IM_DC] * je::HUFF_WORDS, g.ac0 = im[je::IM_AC] * je::HUFF_WORDS;
  g.dc1 = im[je::IM_DC + (ncomp == 3 ? 1 : 0)] * je::HUFF_WORDS, g.ac1 = im[je::IM_AC + (ncomp == 3 ? 1 : 0)] * je::HUFF_WORDS;
  g.dc2 = im[je::IM_DC + (ncomp == 3 ? 2 : 0)] * je::HUFF_WORDS, g.ac2 = im[je::IM_AC + (ncomp == 3 ? 2 : 0)] * je::HUFF_WORDS;
  g.limit = seg[4] * g.bpm;            // check_segment: at most 2048 x 2048 MCUs
  g.coef = coef + ((long long)im[je::IM_BLOCK0] + (long long)seg[3] * g.bpm) * 64;
  g.near = data;
  g.near_lo = g.near_hi = 0;
}

JPEG_HD int component_of(const Segment& g, int b) { return b < g.luma_blocks ? 0 : b - g.luma_blocks + 1; }

// the state lane i starts from before it knows better; lane 0's is the true one
JPEG_HD State guess(const Segment& g, int i) { return make_state(g.begin + i * g.S, 0, 0, 0); }

struct Lane {
  State exit;
  int blocks;        // completed: the transitions b -> b + 1
  int error;         // not WRITE: the lane met a code error (a code of no table, a run past coefficient 63, a DC size above 15)
  int status;        // WRITE only
  int dc_end;        // WRITE only: one past the last block (counted from the segment's first) whose DC this lane wrote, or 0
};

// Lane i of segment g from `entry`.  WRITE: `entry` is the true one and `block` the block (from the segment's first) it lies in.
//
// The two kinds of error.  Running out of stream - bits consumed beyond the segment's end or beyond a marker inside it - is a fact
// of the bytes, the same for every decoder that gets there: the lane finishes the block at hand on zero bits, as the serial body does,
// and exits ENDED.  A code error depends on the state, and a lane that decodes from a guessed state meets such errors all the time;
// if they ended it, every lane behind it would pass ENDED on and lose the exit it had found by itself, and the true states would then
// travel one lane per round.  So without WRITE a code error is noted in `error` and the lane goes on from a fixed recovery state
// (b = 0, z = 0; after a code of no table one bit further): its exit stays a function of its entry alone.  At the fixed point every
// lane in front of the first one with `error` set has decoded the true stream without a code error, so that lane's is the stream's
// first real one: with WRITE it ends the lane there, as it ends the serial body, and the lanes behind it are not run (first_error).
template <bool WRITE>
JPEG_HD void decode_subsequence(const Segment& g, int i, State entry, int block, Lane& out) {
  out.exit = entry;
  out.blocks = out.error = out.status = out.dc_end = 0;
  if (entry & ENDED) return;
  const bool last = i == g.n_sub - 1;
  const int sub_end = last ? 0x7fffffff : g.begin + (i + 1) * g.S;      // i < n_sub - 1: below the segment's end
  int pos = state_pos(entry), bit = (int)(entry >> 32) & 7, b = (int)(entry >> 35) & 7, z = (int)(entry >> 38) & 63;
  if (!last && pos >= sub_end) return;                   // the entry lies beyond this subsequence: passed through
  if (WRITE && block >= g.limit) return;
  Reader r;
  reader_init(r, g.data, g.end, pos, bit, g.near, g.near_lo, g.near_hi);
  short* dst = g.coef + (long long)block * 64;           // WRITE only
  const int dc0 = g.dc0, dc1 = g.dc1, dc2 = g.dc2, ac0 = g.ac0, ac1 = g.ac1, ac2 = g.ac2, luma_blocks = g.luma_blocks, bpm = g.bpm;
  const int* __restrict__ tables = g.tables;
  int status = 0;
  for (;;) {
    const int c = b < luma_blocks ? 0 : b - luma_blocks + 1;
    if (z == 0) {
      const int t = decode_symbol(r, tables + (c == 0 ? dc0 : c == 1 ? dc1 : dc2));
      if (t < 0 || t > 15) {
        status |= je::STATUS_CORRUPT;
        if (WRITE || r.status) break;
        if (t < 0) consume(r, 1);
        out.error = 1;
        b = 0;
        if (r.status) break;
        goto boundary;
      }
      const int diff = receive_extend(r, t);
      if (WRITE) {
        dst[0] = (short)diff;
        out.dc_end = block + 1;
      }
      z = 1;
    } else {
      const int rs = decode_symbol(r, tables + (c == 0 ? ac0 : c == 1 ? ac1 : ac2));
      if (rs < 0) {
        status |= je::STATUS_CORRUPT;
        if (WRITE || r.status) break;
        consume(r, 1);
        out.error = 1;
        b = z = 0;
        if (r.status) break;
        goto boundary;
      }
      const int run = rs >> 4, s = rs & 15;
      if (s == 0) {
        z = run == 15 ? z + 16 : 64;                     // ZRL, EOB
      } else {
        z += run;
        if (z > 63) {
          status |= je::STATUS_CORRUPT;
          if (WRITE || r.status) break;
          out.error = 1;
          b = z = 0;
          goto boundary;
        }
        const int v = receive_extend(r, s);
        if (WRITE) dst[je::natural_index(z)] = (short)v;
        ++z;
      }
    }
    if (z >= 64) {                                       // the block is complete
      ++out.blocks;
      ++block;
      dst += 64;
      b = b + 1 == bpm ? 0 : b + 1;
      z = 0;
      if (r.status) break;
      if (WRITE && block >= g.limit) break;
    } else if (r.status) {
      continue;                                          // the serial body finishes the block at hand on zero bits
    }
  boundary:
    if (!last && r.tail >= sub_end) {                    // (the next bit lies at or in front of tail)
      position(r, pos, bit);
      if (pos >= sub_end) {
        out.exit = make_state(pos, bit, b, z);
        out.status = status;
        return;
      }
    }
  }
  if (out.blocks > BLOCK_CAP) out.blocks = BLOCK_CAP;
  out.status = status | r.status;
  out.exit = ENDED;
}

// The first lane of lanes [0, n) with a code error, or n: the lanes behind it are not run with WRITE.
JPEG_HD int first_error(const int* __restrict__ error, int n) {
  for (int i = 0; i < n; ++i)
    if (error[i]) return i;
  return n;
}

// The DC differences of blocks [0, n) of a segment -> values, one component after the other.  Serial form (the host's; the device's
// kernel cuts [0, n) into pieces and adds each piece's offset, in the same wrapping arithmetic).
JPEG_HD void dc_scan(const Segment& g, int n) {
  unsigned short pred[3] = {0, 0, 0};
  int b = 0;
  for (int k = 0; k < n; ++k) {
    const int c = component_of(g, b);
    pred[c] = (unsigned short)(pred[c] + (unsigned short)g.coef[(long long)k * 64]);
    g.coef[(long long)k * 64] = (short)pred[c];
    b = b + 1 == g.bpm ? 0 : b + 1;
  }
}

}  // namespace jpeg_parallel
