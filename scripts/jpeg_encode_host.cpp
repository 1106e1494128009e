// The JPEG writer's entropy body (pmce_amd/csrc/jpeg_encode.hpp) run on the host, lane by lane as the device runs it, over coefficients
// from a file, between guard regions; and the quantiser's reciprocal tried over its whole range.  Stand-alone: build with any C++17
// compiler (add -fsanitize=address,undefined to have the body's loads and stores checked).
//
//   c++ -std=c++17 -O1 -I pmce_amd/csrc scripts/jpeg_encode_host.cpp -o jpeg_encode_host && ./jpeg_encode_host case.bin
//
// case.bin (tests/test_jpeg_enc_host.py writes it): the magic "PMCEJENC"; int64 x 4 = (blocks, luma blocks per MCU, restart interval in
// MCUs, bytes of the expected scan); the coefficients int16 [blocks][64] in zigzag order, blocks in scan order; the expected scan - the
// stuffed bytes with their padding and RSTn markers, without EOI - little-endian, no padding.
// Prints "ok: ..." and exits 0, or "FAIL ..." and exits 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "jpeg_encode.hpp"

namespace jc = jpeg_encode;

static int fail(const char* what, long long a = 0, long long b = 0) {
  std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
  return 1;
}

int main(int argc, char** argv) {
  // the reciprocal: every divisor the quantiser can meet, every dividend of 16 bits, both signs
  long long tried = 0;
  for (uint32_t q = 1; q <= 255; ++q) {
    const uint32_t qv = 8 * q, rc = jc::quant_reciprocal(qv);
    for (int c = 0; c < (1 << 16); ++c) {
      const int want = (int)(((uint32_t)c + (qv >> 1)) / qv);
      if (jc::quantise(c, qv, rc) != want || jc::quantise(-c, qv, rc) != -want) return fail("reciprocal", qv, c);
      ++tried;
    }
  }
  if (argc < 2) return fail("usage: jpeg_encode_host case.bin");
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) return fail("cannot open the case");
  char magic[8];
  long long head[4];
  if (std::fread(magic, 1, 8, fh) != 8 || std::memcmp(magic, "PMCEJENC", 8) != 0 || std::fread(head, 8, 4, fh) != 4) return fail("bad header");
  const long long blocks = head[0], restart_in = head[2], n_expected = head[3];
  const int luma = (int)head[1], bpm = luma + 2;
  if (blocks < 1 || blocks > (1 << 20) || (luma != 1 && luma != 2 && luma != 4) || blocks % bpm || restart_in < 0 || n_expected < 0 ||
      n_expected > (1ll << 30))
    return fail("bad sizes");
  std::vector<short> coef((size_t)blocks * 64);
  std::vector<unsigned char> expected((size_t)n_expected);
  if (std::fread(coef.data(), 2, coef.size(), fh) != coef.size() ||
      (n_expected && std::fread(expected.data(), 1, expected.size(), fh) != expected.size()))
    return fail("short file");
  std::fclose(fh);

  const long long mcus = blocks / bpm, restart = restart_in < mcus ? restart_in : 0;
  const long long bpi = restart ? restart * bpm : blocks, n_int = (blocks + bpi - 1) / bpi, slot = jc::slot_bytes(bpi);
  constexpr int GUARD = 64;                             // words on either side of an interval's slot
  constexpr uint32_t GUARD_WORD = 0xA5C35A3Cu;
  std::vector<unsigned char> out;
  long long longest = 0;
  for (long long i = 0; i < n_int; ++i) {
    const long long b0 = i * bpi, b1 = b0 + bpi < blocks ? b0 + bpi : blocks;
    std::vector<uint32_t> words((size_t)(slot / 4) + 2 * GUARD, 0u);
    for (int g = 0; g < GUARD; ++g) words[g] = words[words.size() - 1 - g] = GUARD_WORD;
    uint32_t* stream = words.data() + GUARD;
    // lengths, then offsets (the device's first two launches)
    std::vector<long long> off((size_t)(b1 - b0) + 1, 0);
    for (long long b = b0; b < b1; ++b) {
      uint64_t nonzero = 0;
      for (int k = 0; k < 64; ++k) nonzero |= (uint64_t)(coef[b * 64 + k] != 0) << k;
      long long total = 0;
      for (int k = 0; k < 64; ++k) {
        int value = coef[b * 64 + k];
        if (k == 0) {
          const long long pred = jc::dc_predecessor(b, luma, restart);
          if (pred >= 0) value -= coef[pred * 64];
        }
        uint64_t bits;
        const int n = jc::lane_code(k, value, nonzero, jc::block_component(b, luma) != 0, bits);
        if (n < 0 || n > jc::MAX_LANE_BITS || (n < 64 && (bits >> n) != 0)) return fail("a lane's code", b, k);
        total += n;
      }
      if (total > 8 * jc::MAX_BLOCK_BYTES) return fail("a block's length", b, total);
      longest = total > longest ? total : longest;
      off[b - b0 + 1] = off[b - b0] + total;
    }
    // bits: lanes and blocks in REVERSE order - the result of OR does not depend on it
    for (long long b = b1 - 1; b >= b0; --b) {
      uint64_t nonzero = 0;
      int len[64];
      uint64_t code[64];
      for (int k = 0; k < 64; ++k) nonzero |= (uint64_t)(coef[b * 64 + k] != 0) << k;
      long long at = off[b - b0];
      long long pos[64];
      for (int k = 0; k < 64; ++k) {
        int value = coef[b * 64 + k];
        if (k == 0) {
          const long long pred = jc::dc_predecessor(b, luma, restart);
          if (pred >= 0) value -= coef[pred * 64];
        }
        len[k] = jc::lane_code(k, value, nonzero, jc::block_component(b, luma) != 0, code[k]);
        pos[k] = at;
        at += len[k];
      }
      for (int k = 63; k >= 0; --k)
        jc::put_bits(code[k], len[k], pos[k], [&](long long w, uint32_t v) {
          if (w >= 0 && w < slot / 4) stream[w] |= v;
          else longest = -1;                                    // a word outside the slot: reported below
        });
    }
    if (longest < 0) return fail("a word outside the interval's slot", i);
    for (int g = 0; g < GUARD; ++g)
      if (words[g] != GUARD_WORD || words[words.size() - 1 - g] != GUARD_WORD) return fail("guard touched", i, g);
    // padding, stuffing, marker (the device's last launches)
    const long long ibits = off[b1 - b0], nbytes = (ibits + 7) >> 3;
    for (long long j = 0; j < nbytes; ++j) {
      unsigned byte = (stream[j >> 2] >> (24 - 8 * (j & 3))) & 255u;                   // big-endian words
      if (j == nbytes - 1 && (ibits & 7)) byte |= (1u << (8 - (ibits & 7))) - 1u;
      out.push_back((unsigned char)byte);
      if (byte == 255u) out.push_back(0);
    }
    if (i != n_int - 1) {
      out.push_back(0xFF);
      out.push_back((unsigned char)(0xD0 + (i & 7)));
    }
  }
  if ((long long)out.size() != n_expected) return fail("the scan's length", (long long)out.size(), n_expected);
  for (size_t j = 0; j < out.size(); ++j)
    if (out[j] != expected[j]) return fail("the scan's bytes differ at", (long long)j, out[j]);
  // the device's view of a word: byte_swap turns the big-endian word into the bytes' order in memory
  const uint32_t probe = jc::byte_swap(0x11223344u);
  unsigned char mem[4];
  std::memcpy(mem, &probe, 4);
  const uint16_t one = 1;
  if (*reinterpret_cast<const unsigned char*>(&one) == 1 && (mem[0] != 0x11 || mem[3] != 0x44)) return fail("byte_swap");
  std::printf("ok: %lld blocks in %lld intervals, %lld bytes compared, longest block %lld bits, reciprocal exact for %lld pairs, guards untouched\n",
              blocks, n_int, n_expected, longest, tried);
  return 0;
}
