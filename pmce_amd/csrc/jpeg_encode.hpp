// The baseline JPEG writer's arithmetic and its entropy coder (ITU-T T.81 Annex F.1.2 with the tables of Annex K.3), written once for
// the device (jpeg_encode.hip) and for the host (scripts/jpeg_encode_host.cpp, which runs this body over crafted coefficients between
// guard regions).  Everything is integer arithmetic: jccolor's fixed-point conversion, jfdctint's "islow" forward DCT, the quantiser's
// rounding division (by a reciprocal that the host program shows exact) and the Huffman coder.
//
// The coder is written per LANE, as the device runs it: lane k of a 64-lane wave owns zigzag coefficient k of one block.  From the
// mask of the block's non-zero coefficients a lane knows the run of zeros in front of it, so it knows its own bits - its ZRL codes,
// its run/size code and its value bits (lane 0: the DC difference; lane 63: EOB when its coefficient is zero) - without looking at
// another lane.  A prefix sum of the lengths gives each lane its place; put_bits() ORs the bits into big-endian 32-bit words, so the
// result does not depend on the order in which lanes (or, on the host, loop iterations) arrive.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_ENC_HD __host__ __device__ __forceinline__
#else
#define JPEG_ENC_HD inline
#endif

namespace jpeg_encode {

constexpr int MAX_BLOCK_BYTES = 208;     // a block's code before stuffing: 9 + 11 bits of DC, 63 x (16 + 10) bits of AC = 1658 bits
constexpr int MAX_LANE_BITS = 59;        // three ZRL codes of 11 bits, a run/size code of 16, a value of 10
constexpr int PIECE = 256;               // bytes of the unstuffed stream per wave of the stuffing stage: four per lane
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_PASS = SCAN_THREADS * SCAN_ITEMS;      // entries per pass of a segment's scan
constexpr int STATUS_CAPACITY = 1;       // the frame's file is longer than `capacity`: served with length 0

// ---------------------------------------------------------------------------------------------------------------------------------------
// tables
// ---------------------------------------------------------------------------------------------------------------------------------------
struct Tables {
  uint32_t dc[2][12];       // by category: (code << 8) | length; [0] luma, [1] chroma
  uint32_t ac[2][256];      // by (run << 4) | size; 0: no such symbol
};

constexpr void fill_codes(uint32_t* out, const unsigned char* counts, const unsigned char* values) {
  unsigned code = 0;
  int k = 0;
  for (int length = 1; length <= 16; ++length) {
    for (int i = 0; i < counts[length - 1]; ++i) out[values[k++]] = (code++ << 8) | (unsigned)length;
    code <<= 1;
  }
}

constexpr Tables make_tables() {
  // T.81 Annex K.3: the counts of the code lengths 1..16, then the values in code order
  constexpr unsigned char dc_luma_n[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
  constexpr unsigned char dc_chroma_n[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
  constexpr unsigned char dc_v[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  constexpr unsigned char ac_luma_n[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
  constexpr unsigned char ac_luma_v[162] = {
      1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,
      66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,
      52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100,
      101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
      149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194,
      195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232,
      233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250};
  constexpr unsigned char ac_chroma_n[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
  constexpr unsigned char ac_chroma_v[162] = {
      0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161,
      177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,
      41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,
      100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146,
      147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185,
      186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231,
      232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250};
  Tables t{};
  fill_codes(t.dc[0], dc_luma_n, dc_v);
  fill_codes(t.dc[1], dc_chroma_n, dc_v);
  fill_codes(t.ac[0], ac_luma_n, ac_luma_v);
  fill_codes(t.ac[1], ac_chroma_n, ac_chroma_v);
  return t;
}

JPEG_ENC_HD uint32_t dc_code(int chroma, int category) {
  constexpr Tables t = make_tables();
  return t.dc[chroma & 1][category < 11 ? category : 11];
}
JPEG_ENC_HD uint32_t ac_code(int chroma, int run_size) {
  constexpr Tables t = make_tables();
  return t.ac[chroma & 1][run_size & 255];
}

// position in zigzag order of the coefficient with natural (row-major) index n: the inverse of T.81 figure A.6
JPEG_ENC_HD int zigzag_position(int n) {
  constexpr unsigned char t[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                   41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                   46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
  return t[n & 63];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// colour, forward DCT, quantisation
// ---------------------------------------------------------------------------------------------------------------------------------------
// jccolor.c, 16 fractional bits
JPEG_ENC_HD int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
JPEG_ENC_HD int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
JPEG_ENC_HD int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270, FIX_0_899976223 = 7373,
              FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137, FIX_1_961570560 = 16069,
              FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// jfdctint.c (CONST_BITS 13, PASS1_BITS 2), one pass over eight values.  FIRST: the row pass, whose results stay scaled up by 4 and
// fit 16 bits for 8-bit samples (tests/jpeg_enc_ref.py asserts the ranges); else the column pass.  32-bit integers suffice.
template <bool FIRST>
JPEG_ENC_HD void fdct8(const int* d, int* o) {
  constexpr int N = FIRST ? 11 : 15, HALF = 1 << (N - 1);
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (FIRST) {
    o[0] = (tmp10 + tmp11) * 4;
    o[4] = (tmp10 - tmp11) * 4;
  } else {
    o[0] = (tmp10 + tmp11 + 2) >> 2;
    o[4] = (tmp10 - tmp11 + 2) >> 2;
  }
  int z1 = (tmp12 + tmp13) * FIX_0_541196100;
  o[2] = (z1 + tmp13 * FIX_0_765366865 + HALF) >> N;
  o[6] = (z1 - tmp12 * FIX_1_847759065 + HALF) >> N;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  const int t4 = tmp4 * FIX_0_298631336, t5 = tmp5 * FIX_2_053119869, t6 = tmp6 * FIX_3_072711026, t7 = tmp7 * FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 = z3 * -FIX_1_961570560 + z5;
  z4 = z4 * -FIX_0_390180644 + z5;
  o[7] = (t4 + z1 + z3 + HALF) >> N;
  o[5] = (t5 + z2 + z4 + HALF) >> N;
  o[3] = (t6 + z2 + z3 + HALF) >> N;
  o[1] = (t7 + z1 + z4 + HALF) >> N;
}

// The quantiser divides |c| + qv / 2 by qv = 8 * table entry (8 .. 2040); |c| stays below 2^15.  floor(a / qv) = (a * recip) >> 32 with
// recip = floor((2^32 - 1) / qv) + 1 for every a < 2^21 (recip * qv - 2^32 is in 0 .. qv, so the error a * that / 2^32 / qv stays below
// 1 / qv); scripts/jpeg_encode_host.cpp tries every qv and every a < 2^16.
JPEG_ENC_HD uint32_t quant_reciprocal(uint32_t qv) { return 0xFFFFFFFFu / qv + 1u; }
JPEG_ENC_HD int quantise(int c, uint32_t qv, uint32_t recip) {
  const uint32_t a = (uint32_t)(c < 0 ? -c : c) + (qv >> 1);
  const int q = (int)(((uint64_t)a * recip) >> 32);
  return c < 0 ? -q : q;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// the entropy coder, per lane
// ---------------------------------------------------------------------------------------------------------------------------------------
JPEG_ENC_HD int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// the low s bits that code `value` of category s: the value itself, or value - 1 for a negative one
JPEG_ENC_HD uint32_t value_bits(int value, int s) { return (uint32_t)(value < 0 ? value - 1 : value) & ((1u << s) - 1u); }

// The block with index `block` of a frame (blocks in scan order, an MCU is `luma` luma blocks, then Cb, then Cr; bpm = luma + 2;
// `restart` MCUs per interval, 0: none): its component, and the block whose DC it is predicted from - -1: zero (the interval's first).
JPEG_ENC_HD int block_component(long long block, int luma) {
  const int k = (int)(block % (luma + 2));
  return k < luma ? 0 : k - luma + 1;
}
JPEG_ENC_HD long long dc_predecessor(long long block, int luma, long long restart) {
  const int bpm = luma + 2, k = (int)(block % bpm);
  const long long mcu = block / bpm;
  if (k > 0 && k < luma) return block - 1;
  if (restart ? mcu % restart == 0 : mcu == 0) return -1;
  return k == 0 ? block - 3 : block - bpm;       // the last luma block of the MCU before, or that MCU's block of the same component
}

// What lane k of a block contributes: `value` is its coefficient - for k = 0 the DC difference -, `nonzero` has bit j set where
// zigzag coefficient j of the block is not zero (bit 0 is ignored).  -> the number of bits; they are the low bits of `bits`, the
// first one the most significant.  Values beyond what Annex K's tables code (a DC difference of more than 11 bits, an AC coefficient
// of more than 10) are clamped to the largest codable one.
JPEG_ENC_HD int lane_code(int k, int value, uint64_t nonzero, int chroma, uint64_t& bits) {
  bits = 0;
  if (k == 0) {
    value = value > 2047 ? 2047 : (value < -2047 ? -2047 : value);
    const int s = bit_length((unsigned)(value < 0 ? -value : value));
    const uint32_t e = dc_code(chroma, s);
    bits = ((uint64_t)(e >> 8) << s) | value_bits(value, s);
    return (int)(e & 255) + s;
  }
  if (value == 0) {
    if (k != 63) return 0;
    const uint32_t e = ac_code(chroma, 0x00);          // the block ends in zeros: EOB
    bits = e >> 8;
    return (int)(e & 255);
  }
  value = value > 1023 ? 1023 : (value < -1023 ? -1023 : value);
  const uint64_t below = (nonzero | 1ull) & ((1ull << k) - 1ull);       // bit 0 stands for the DC: runs are counted from coefficient 1
  const int run = k - 1 - (63 - __builtin_clzll(below));
  const uint32_t zrl = ac_code(chroma, 0xF0);
  int n = 0;
  for (int i = 0; i < (run >> 4); ++i) {
    bits = (bits << (zrl & 255)) | (zrl >> 8);
    n += (int)(zrl & 255);
  }
  const int s = bit_length((unsigned)(value < 0 ? -value : value));
  const uint32_t e = ac_code(chroma, ((run & 15) << 4) | s);
  bits = (((bits << (e & 255)) | (e >> 8)) << s) | value_bits(value, s);
  return n + (int)(e & 255) + s;
}

// The low n bits of `bits` (n <= 64 - 5) to bit position `pos` of a stream of big-endian 32-bit words: at most three words are touched,
// each by or_word(word index, bits to OR in).
template <class OrWord>
JPEG_ENC_HD void put_bits(uint64_t bits, int n, long long pos, OrWord&& or_word) {
  long long w = pos >> 5;
  int off = (int)(pos & 31);
  while (n > 0) {
    const int take = n < 32 - off ? n : 32 - off;
    const uint32_t chunk = (uint32_t)((bits >> (n - take)) & ((1ull << take) - 1ull));
    or_word(w, chunk << (32 - off - take));
    n -= take;
    ++w;
    off = 0;
  }
}

JPEG_ENC_HD uint32_t byte_swap(uint32_t v) { return __builtin_bswap32(v); }

// geometry of the workspace (include/pmce_hip.h): bytes of an interval's slot in the unstuffed stream, a whole number of pieces
JPEG_ENC_HD long long slot_bytes(long long blocks_per_interval) {
  return (blocks_per_interval * MAX_BLOCK_BYTES + PIECE - 1) / PIECE * PIECE;
}

}  // namespace jpeg_encode
