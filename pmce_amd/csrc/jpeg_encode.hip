// The demo's frames written as JPEG files on the device (baseline, Huffman, JFIF): what the reference does with cv2.imwrite twice per
// frame (main/run_demo.py:424-426) before it hands the two folders to ffmpeg.  The files are those of libjpeg's default compressor,
// byte for byte: jccolor, jcsample's box filter, jccoefct's dummy blocks, jfdctint, the rounding quantiser and
// Huffman coding with Annex K's tables - integer arithmetic throughout (csrc/jpeg_encode.hpp, shared with the host program that checks it).
//
//   pmce_jpeg_encode_coefficients   frames uint8 [F][H][W][3] -> int16 [blocks][64], zigzag order, blocks in scan (MCU) order, dummy
//                                   blocks included.  A workgroup takes 256 luma columns of one MCU row: the rows' bytes go to LDS by
//                                   16-byte loads, are converted and downsampled into LDS planes, transformed by eight lanes per block
//                                   (a row each, then a column each) and leave as 16-byte stores.
//   pmce_jpeg_encode_entropy        lengths: one wave per block, lane k owns zigzag coefficient k (jpeg_encode.hpp) -> the block's bits;
//                                   offsets: a scan per restart interval; bits: the same lanes place their codes - a block is put
//                                   together in LDS, its inner words are stored, the two it may share with its neighbours are ORed
//                                   in atomically (OR does not depend on order); count / place / frames: 0xFF bytes per 256-byte piece
//                                   of the unstuffed stream, a scan per frame, the frames' offsets; write: stuffed bytes, the 1-bit
//                                   padding, RSTn, the header and EOI at their final places.
//
// No host wait and no floating point; the same bytes whatever the batch and a frame's place in it.
#include "common.hpp"
#include "jpeg_encode.hpp"

namespace {

namespace jc = jpeg_encode;
constexpr int MAX_DIM = 16384;
constexpr int TILE_PX = 256;                              // luma columns per workgroup of the coefficient stage
constexpr int COEF_THREADS = 256;
constexpr int RAW_CHUNKS = TILE_PX * 3 / 16 + 1;          // 16-byte chunks per staged row: the row's bytes keep their alignment
constexpr int RAW_PITCH = RAW_CHUNKS * 16;
constexpr int WS_PITCH = 72;                              // int16 per block between the two passes: 64 + 8, so that the column pass
                                                          // of eight blocks reads eight different groups of four banks
constexpr int MAX_TILE_BLOCKS = 96;                       // 16 MCUs of 6 (4:2:0), 16 of 4 (4:2:2), 32 of 3 (4:4:4)
constexpr int ENTROPY_STAGES = 7;

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ long long wave_inclusive_scan(long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// colour conversion, downsampling, forward DCT, quantisation
// ---------------------------------------------------------------------------------------------------------------------------------------
// grid (tiles of 256 luma columns, MCU rows, frames).  quant: uint16 [2][64], natural order (luma, chroma).
template <int HS, int VS>
__global__ __launch_bounds__(COEF_THREADS) void jpeg_coefficients_kernel(const unsigned char* __restrict__ frames, long long first_frame,
                                                                         int W, int H, int rgb, const unsigned short* __restrict__ quant,
                                                                         short* __restrict__ coef, long long blocks_per_frame) {
  constexpr int LUMA = HS * VS, BPM = LUMA + 2, T = TILE_PX / (8 * HS), ROWS = 8 * VS, CW = TILE_PX / HS;
  static_assert(T * BPM <= MAX_TILE_BLOCKS, "tile blocks");
  // `raw` (the rows' bytes) is dead once the planes are made; the quantised blocks take its place
  __shared__ __attribute__((aligned(16))) unsigned char raw[16 * RAW_PITCH > MAX_TILE_BLOCKS * 128 ? 16 * RAW_PITCH : MAX_TILE_BLOCKS * 128];
  __shared__ __attribute__((aligned(16))) unsigned char yp[16 * TILE_PX];
  __shared__ __attribute__((aligned(16))) unsigned char cp[2][8 * TILE_PX];
  __shared__ __attribute__((aligned(16))) short ws[MAX_TILE_BLOCKS * WS_PITCH];
  __shared__ unsigned s_qv[128], s_rc[128];
  short* outb = reinterpret_cast<short*>(raw);

  const int tid = threadIdx.x, tile = blockIdx.x, my_i = blockIdx.y;
  const int mx = (W + 8 * HS - 1) / (8 * HS), wb = (W + 7) / 8, hb = (H + 7) / 8, chh = (H + VS - 1) / VS;
  const int x0 = tile * TILE_PX, npx = min(TILE_PX, W - x0);
  const unsigned char* fbase = frames + (size_t)(first_frame + blockIdx.z) * H * W * 3;
  if (tid < 128) {
    const unsigned q = quant[tid];
    const unsigned qv = 8u * (q < 1u ? 1u : (q > 255u ? 255u : q));
    s_qv[tid] = qv;
    s_rc[tid] = jc::quant_reciprocal(qv);
  }
  // the tile's rows (the image's last row again below it), byte for byte at the alignment they have in memory
  for (int t = tid; t < ROWS * RAW_CHUNKS; t += COEF_THREADS) {
    const int r = t / RAW_CHUNKS, c = t - r * RAW_CHUNKS;
    const unsigned char* g = fbase + ((size_t)min(my_i * ROWS + r, H - 1) * W + x0) * 3;
    const int len = npx * 3, lo = c * 16 - (int)((uintptr_t)g & 15);
    if (lo >= len || lo + 16 <= 0) continue;
    unsigned char* d = raw + r * RAW_PITCH + c * 16;
    if (lo >= 0 && lo + 16 <= len) {
      *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(g + lo);
    } else {
      for (int j = 0; j < 16; ++j)
        if (lo + j >= 0 && lo + j < len) d[j] = g[lo + j];
    }
  }
  __syncthreads();

  // one lane per chroma sample: its HS x VS pixels' luma, and the box filter of their chroma (jcsample: the bias alternates by column)
  auto row_bytes = [&](int r) -> const unsigned char* {
    const unsigned char* g = fbase + ((size_t)min(my_i * ROWS + r, H - 1) * W + x0) * 3;
    return raw + r * RAW_PITCH + (int)((uintptr_t)g & 15);
  };
  for (int t = tid; t < 8 * CW; t += COEF_THREADS) {
    const int cy = t / CW, cx = t - cy * CW;
    // below the image the LAST DOWNSAMPLED row repeats (the input is padded only to a multiple of VS)
    const int cyc = min(cy, chh - 1 - my_i * 8);
    int cbs = 0, crs = 0;
#pragma unroll
    for (int dy = 0; dy < VS; ++dy) {
      const unsigned char* row = row_bytes(cy * VS + dy);
      const unsigned char* crow = cyc == cy ? row : row_bytes(cyc * VS + dy);
#pragma unroll
      for (int dx = 0; dx < HS; ++dx) {
        const int x = min(cx * HS + dx, npx - 1);          // the row's last pixel repeats to the right
        const int c0 = row[3 * x], g = row[3 * x + 1], c2 = row[3 * x + 2];
        yp[(cy * VS + dy) * TILE_PX + cx * HS + dx] = (unsigned char)jc::ycc_y(rgb ? c0 : c2, g, rgb ? c2 : c0);
        const int d0 = crow[3 * x], dg = crow[3 * x + 1], d2 = crow[3 * x + 2];
        cbs += jc::ycc_cb(rgb ? d0 : d2, dg, rgb ? d2 : d0);
        crs += jc::ycc_cr(rgb ? d0 : d2, dg, rgb ? d2 : d0);
      }
    }
    if (HS == 2 && VS == 2) {
      cbs = (cbs + 1 + (cx & 1)) >> 2;
      crs = (crs + 1 + (cx & 1)) >> 2;
    } else if (HS == 2) {
      cbs = (cbs + (cx & 1)) >> 1;
      crs = (crs + (cx & 1)) >> 1;
    }
    cp[0][cy * TILE_PX + cx] = (unsigned char)cbs;
    cp[1][cy * TILE_PX + cx] = (unsigned char)crs;
  }
  __syncthreads();

  const int mcu0 = tile * T, n_blk = min(T, mx - mcu0) * BPM;
  // rows: lane (block, row).  A dummy luma block (beyond the component's real blocks: jccoefct.c) transforms the block whose DC it
  // repeats - the one before it in the MCU, for a whole dummy row the last block before that row - and keeps the DC alone.
  for (int t = tid; t < n_blk * 8; t += COEF_THREADS) {
    const int lb = t >> 3, row = t & 7, m = lb / BPM, k = lb - m * BPM;
    const unsigned char* src;
    if (k < LUMA) {
      int ks = k;
      if (my_i * VS + k / HS >= hb)
        ks = (HS == 2 && (mcu0 + m) * HS + 1 < wb) ? 1 : 0;
      else if ((mcu0 + m) * HS + k % HS >= wb)
        ks = k - 1;
      src = yp + ((ks / HS) * 8 + row) * TILE_PX + (m * HS + ks % HS) * 8;
    } else {
      src = cp[k - LUMA] + row * TILE_PX + m * 8;
    }
    const uint2 px = *reinterpret_cast<const uint2*>(src);
    int d[8], o[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d[i] = (int)((px.x >> (8 * i)) & 255u) - 128;
      d[4 + i] = (int)((px.y >> (8 * i)) & 255u) - 128;
    }
    jc::fdct8<true>(d, o);
    uint4 pk;
    pk.x = (unsigned)(o[0] & 0xffff) | ((unsigned)o[1] << 16);
    pk.y = (unsigned)(o[2] & 0xffff) | ((unsigned)o[3] << 16);
    pk.z = (unsigned)(o[4] & 0xffff) | ((unsigned)o[5] << 16);
    pk.w = (unsigned)(o[6] & 0xffff) | ((unsigned)o[7] << 16);
    *reinterpret_cast<uint4*>(ws + lb * WS_PITCH + row * 8) = pk;
  }
  __syncthreads();
  // columns: lane (block, column), then the quantiser; the block is put together in zigzag order
  for (int t = tid; t < n_blk * 8; t += COEF_THREADS) {
    const int lb = t >> 3, col = t & 7, m = lb / BPM, k = lb - m * BPM;
    const bool dummy = k < LUMA && (my_i * VS + k / HS >= hb || (mcu0 + m) * HS + k % HS >= wb);
    const int tb = k < LUMA ? 0 : 64;
    int d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = ws[lb * WS_PITCH + r * 8 + col];
    jc::fdct8<false>(d, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int n = r * 8 + col;
      const int q = jc::quantise(o[r], s_qv[tb + n], s_rc[tb + n]);
      outb[lb * 64 + jc::zigzag_position(n)] = (short)((dummy && n) ? 0 : q);
    }
  }
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(coef + ((size_t)blockIdx.z * blocks_per_frame + ((size_t)my_i * mx + mcu0) * BPM) * 64);
  for (int t = tid; t < n_blk * 8; t += COEF_THREADS) dst[t] = reinterpret_cast<const uint4*>(outb)[t];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// entropy coding
// ---------------------------------------------------------------------------------------------------------------------------------------
// The workspace of one call (include/pmce_hip.h).  nb: blocks per frame; bpi: blocks per restart interval; n_int: intervals per frame;
// slot: bytes of an interval in the unstuffed stream; P: pieces per slot; NP: pieces per frame.
struct Layout {
  long long nb, bpi, n_int, slot, P, NP;
  size_t o_stream, o_bits, o_off, o_ibits, o_plen, o_ppos, o_ftot, total;
};

bool make_layout(long long n, long long mcus, int luma, long long restart, Layout& L) {
  if (n < 1 || n > 65535 || mcus < 1 || mcus > (1ll << 22) || (luma != 1 && luma != 2 && luma != 4) || restart < 0 || restart > 65535) return false;
  const long long bpm = luma + 2;
  L.nb = mcus * bpm;
  L.bpi = restart ? (restart < mcus ? restart : mcus) * bpm : L.nb;
  L.n_int = (L.nb + L.bpi - 1) / L.bpi;
  L.slot = jc::slot_bytes(L.bpi);
  L.P = L.slot / jc::PIECE;
  L.NP = L.n_int * L.P;
  if (n * L.nb >= (1ll << 31) || n * L.NP >= (1ll << 31) || n * L.n_int * L.slot >= (1ll << 40)) return false;
  auto up = [](size_t v) { return (v + 15) / 16 * 16; };
  size_t at = 0;
  L.o_stream = at, at += up((size_t)(n * L.n_int * L.slot));
  L.o_bits = at, at += up((size_t)(n * L.nb) * sizeof(int));
  L.o_off = at, at += up((size_t)(n * L.nb) * sizeof(long long));
  L.o_ibits = at, at += up((size_t)(n * L.n_int) * sizeof(long long));
  L.o_plen = at, at += up((size_t)(n * L.NP) * sizeof(int));
  L.o_ppos = at, at += up((size_t)(n * L.NP) * sizeof(long long));
  L.o_ftot = at, at += up((size_t)n * sizeof(long long));
  L.total = at;
  return true;
}

// What lane `lane` of the wave that owns block b contributes (jpeg_encode.hpp): -> its number of bits.
__device__ __forceinline__ int block_lane_code(const short* __restrict__ coef, long long b, long long nb, int luma, long long restart,
                                               int lane, uint64_t& bits) {
  const long long lb = b % nb;
  int value = coef[b * 64 + lane];
  const uint64_t nonzero = __ballot(value != 0);
  if (lane == 0) {
    const long long pred = jc::dc_predecessor(lb, luma, restart);
    if (pred >= 0) value -= coef[(b - lb + pred) * 64];
  }
  return jc::lane_code(lane, value, nonzero, jc::block_component(lb, luma) != 0, bits);
}

// one wave per block, four per workgroup -> block_bits[b]
__global__ __launch_bounds__(256) void jpeg_lengths_kernel(const short* __restrict__ coef, long long total_blocks, long long nb, int luma,
                                                           long long restart, int* __restrict__ block_bits) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= total_blocks) return;
  uint64_t bits;
  const int n = block_lane_code(coef, b, nb, luma, restart, lane, bits);
  const int incl = wave_inclusive_scan(n, lane);
  if (lane == 63) block_bits[b] = incl;
}

// An exclusive scan per segment: segment i of frame f covers in[f * per_frame + i * per_segment ...], per_segment entries (the frame's
// last one what is left); SCAN_PASS entries per pass, the total carried from pass to pass.  grid: frames x segments per frame.
__global__ __launch_bounds__(jc::SCAN_THREADS) void jpeg_segment_scan_kernel(const int* __restrict__ in, long long* __restrict__ out,
                                                                             long long* __restrict__ totals, long long per_frame,
                                                                             long long per_segment, long long segments_per_frame) {
  __shared__ long long wave_total[jc::SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long f = blockIdx.x / segments_per_frame, i = blockIdx.x - f * segments_per_frame;
  const long long start = f * per_frame + i * per_segment, len = min(per_segment, per_frame - i * per_segment);
  long long carry = 0;
  for (long long base = 0; base < len; base += jc::SCAN_PASS) {
    const long long at = base + (long long)tid * jc::SCAN_ITEMS;
    int v[jc::SCAN_ITEMS];
    long long s = 0;
#pragma unroll
    for (int j = 0; j < jc::SCAN_ITEMS; ++j) {
      v[j] = at + j < len ? in[start + at + j] : 0;
      s += v[j];
    }
    const long long incl = wave_inclusive_scan(s, lane);
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    long long before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < jc::SCAN_THREADS / 64; ++w) {
      if (w < wave) before += wave_total[w];
      all += wave_total[w];
    }
    long long run = before + incl - s;
#pragma unroll
    for (int j = 0; j < jc::SCAN_ITEMS; ++j) {
      if (at + j < len) out[start + at + j] = run;
      run += v[j];
    }
    carry += all;
    __syncthreads();
  }
  if (tid == 0) totals[blockIdx.x] = carry;
}

// one wave per block: the block's bits into the unstuffed stream (zeroed beforehand), at the interval's slot + block_off[b] bits
__global__ __launch_bounds__(256) void jpeg_bits_kernel(const short* __restrict__ coef, long long total_blocks, long long nb, int luma,
                                                        long long restart, const long long* __restrict__ block_off, long long n_int,
                                                        long long slot, unsigned* __restrict__ stream) {
  __shared__ unsigned sh[4][56];        // 31 bits of the word shared with the block before + 1658 bits: 53 words
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long b = (long long)blockIdx.x * 4 + wave;
  const bool active = b < total_blocks;
  if (lane < 56) sh[wave][lane] = 0;
  __syncthreads();
  uint64_t bits = 0;
  int n = 0, first_bit = 0;
  long long word0 = 0;
  if (active) {
    n = block_lane_code(coef, b, nb, luma, restart, lane, bits);
    const long long off = block_off[b];
    const long long bpm = luma + 2, lb = b % nb, interval = (b / nb) * n_int + (restart ? lb / bpm / restart : 0);
    first_bit = (int)(off & 31);
    word0 = interval * (slot / 4) + (off >> 5);
  }
  const int incl = wave_inclusive_scan(n, lane);
  const int total = __shfl(incl, 63, 64);
  unsigned* mine = sh[wave];
  jc::put_bits(bits, n, first_bit + incl - n, [&](long long w, unsigned v) { atomicOr(&mine[w], v); });
  __syncthreads();
  const int n_words = (first_bit + total + 31) >> 5;
  if (active && lane < n_words) {
    const unsigned v = jc::byte_swap(mine[lane]);
    const bool shared = (lane == 0 && first_bit != 0) || (lane == n_words - 1 && ((first_bit + total) & 31) != 0);
    if (!shared)
      stream[word0 + lane] = v;
    else if (v)
      atomicOr(&stream[word0 + lane], v);
  }
}

// The four bytes lane `lane` of a piece's wave owns (little-endian in the word), the interval's last byte padded with 1-bits.
__device__ __forceinline__ unsigned piece_word(const unsigned* __restrict__ stream, long long interval, long long slot, long long p,
                                               int lane, long long interval_bits, int valid) {
  unsigned w = 4 * lane < valid ? stream[(interval * slot + p * jc::PIECE) / 4 + lane] : 0u;
  const int pad = (int)((8 - (interval_bits & 7)) & 7);
  const long long last = ((interval_bits + 7) >> 3) - 1 - p * jc::PIECE - 4 * lane;
  if (pad && last >= 0 && last < 4) w |= ((1u << pad) - 1u) << (8 * (int)last);
  return w;
}
__device__ __forceinline__ int count_ff(unsigned w, int n_valid) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c += (j < n_valid && ((w >> (8 * j)) & 255u) == 255u) ? 1 : 0;
  return c;
}

// one wave per piece -> piece_len: its bytes in the file (valid + stuffed), the slot's last piece with the marker behind the interval
__global__ __launch_bounds__(256) void jpeg_count_kernel(const unsigned* __restrict__ stream, const long long* __restrict__ interval_bits,
                                                         long long total_pieces, long long NP, long long P, long long n_int, long long slot,
                                                         int* __restrict__ piece_len) {
  const int lane = threadIdx.x & 63;
  const long long gp = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gp >= total_pieces) return;
  const long long f = gp / NP, r = gp - f * NP, i = r / P, p = r - i * P, interval = f * n_int + i;
  const long long ib = interval_bits[interval], left = ((ib + 7) >> 3) - p * jc::PIECE;
  const int valid = (int)(left < 0 ? 0 : (left > jc::PIECE ? jc::PIECE : left));
  int c = 0;
  if (valid) {
    const unsigned w = piece_word(stream, interval, slot, p, lane, ib, valid);
    c = wave_inclusive_scan(count_ff(w, valid - 4 * lane), lane);
  }
  if (lane == 63) piece_len[gp] = valid + c + (p == P - 1 ? 2 : 0);
}

// the frames' places in `data`: one lane walks the call's frames (at most 65535)
__global__ void jpeg_frames_kernel(const long long* __restrict__ frame_total, int n_frames, int header_bytes, long long capacity,
                                   long long data_bytes, long long first_frame, long long* __restrict__ offsets, int* __restrict__ status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long at = first_frame ? offsets[first_frame] : 0;
  if (!first_frame) offsets[0] = 0;
  for (int f = 0; f < n_frames; ++f) {
    const long long len = header_bytes + frame_total[f];
    const bool fits = len <= capacity && at + len <= data_bytes;
    status[first_frame + f] = fits ? 0 : jc::STATUS_CAPACITY;
    at += fits ? len : 0;
    offsets[first_frame + f + 1] = at;
  }
}

// one wave per piece: its bytes, a zero behind every 0xFF, to their place; RSTn / EOI behind the interval; the header by the frame's first piece
__global__ __launch_bounds__(256) void jpeg_write_kernel(const unsigned* __restrict__ stream, const long long* __restrict__ interval_bits,
                                                         const long long* __restrict__ piece_pos, long long total_pieces, long long NP,
                                                         long long P, long long n_int, long long slot,
                                                         const unsigned char* __restrict__ header, int header_bytes, long long first_frame,
                                                         const long long* __restrict__ offsets, const int* __restrict__ status,
                                                         unsigned char* __restrict__ data) {
  const int lane = threadIdx.x & 63;
  const long long gp = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gp >= total_pieces) return;
  const long long f = gp / NP, r = gp - f * NP, i = r / P, p = r - i * P, interval = f * n_int + i;
  if (status[first_frame + f] != 0) return;
  unsigned char* file = data + offsets[first_frame + f];
  if (r == 0)
    for (int j = lane; j < header_bytes; j += 64) file[j] = header[j];
  const long long ib = interval_bits[interval], left = ((ib + 7) >> 3) - p * jc::PIECE;
  const int valid = (int)(left < 0 ? 0 : (left > jc::PIECE ? jc::PIECE : left));
  unsigned char* dst = file + header_bytes + piece_pos[gp];
  int ff_total = 0;
  if (valid) {
    const unsigned w = piece_word(stream, interval, slot, p, lane, ib, valid);
    const int mine = min(max(valid - 4 * lane, 0), 4), c = count_ff(w, mine);
    const int incl = wave_inclusive_scan(c, lane);
    ff_total = __shfl(incl, 63, 64);
    int at = 4 * lane + incl - c;
    for (int j = 0; j < mine; ++j) {
      const unsigned byte = (w >> (8 * j)) & 255u;
      dst[at++] = (unsigned char)byte;
      if (byte == 255u) dst[at++] = 0;
    }
  }
  if (p == P - 1 && lane == 0) {
    dst[valid + ff_total] = 0xFF;
    dst[valid + ff_total + 1] = (unsigned char)(i == n_int - 1 ? 0xD9 : 0xD0 + (int)(i & 7));
  }
}

}  // namespace

extern "C" int pmce_jpeg_encode_scan_pass(void) { return jc::SCAN_PASS; }
extern "C" int pmce_jpeg_encode_stages(void) { return ENTROPY_STAGES; }

extern "C" size_t pmce_jpeg_encode_workspace_bytes(int n_frames, long long mcus_per_frame, int luma_blocks, int restart_interval) {
  Layout L;
  return make_layout(n_frames, mcus_per_frame, luma_blocks, restart_interval, L) ? L.total : 0;
}

extern "C" int pmce_jpeg_encode_coefficients(const unsigned char* frames, long long first_frame, int n_frames, int width, int height, int h,
                                             int v, int rgb, const unsigned short* quant, short* coefficients, long long n_blocks,
                                             hipStream_t stream) {
  PMCE_REQUIRE(frames && quant && coefficients, "jpeg_encode_coefficients: null pointer");
  PMCE_REQUIRE(first_frame >= 0 && n_frames >= 1 && n_frames <= 65535, "jpeg_encode_coefficients: need first_frame >= 0 and 1 .. 65535 frames (got %lld, %d)",
               first_frame, n_frames);
  PMCE_REQUIRE(width >= 1 && width <= MAX_DIM && height >= 1 && height <= MAX_DIM,
               "jpeg_encode_coefficients: need a frame of 1..%d x 1..%d (got %d x %d)", MAX_DIM, MAX_DIM, width, height);
  PMCE_REQUIRE((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2),
               "jpeg_encode_coefficients: luma sampling must be 1x1, 2x1 or 2x2 (got %dx%d)", h, v);
  PMCE_REQUIRE(((uintptr_t)coefficients & 15) == 0, "jpeg_encode_coefficients: the coefficient buffer must be 16-byte aligned");
  const int mx = (width + 8 * h - 1) / (8 * h), my = (height + 8 * v - 1) / (8 * v);
  const long long nb = (long long)mx * my * (h * v + 2);
  PMCE_REQUIRE(n_blocks >= nb * n_frames, "jpeg_encode_coefficients: %d frames of %lld blocks need %lld blocks (got %lld)", n_frames, nb,
               nb * n_frames, n_blocks);
  const int T = TILE_PX / (8 * h);
  const dim3 grid((unsigned)((mx + T - 1) / T), (unsigned)my, (unsigned)n_frames);
  if (h == 1)
    hipLaunchKernelGGL((jpeg_coefficients_kernel<1, 1>), grid, dim3(COEF_THREADS), 0, stream, frames, first_frame, width, height, rgb ? 1 : 0,
                       quant, coefficients, nb);
  else if (v == 1)
    hipLaunchKernelGGL((jpeg_coefficients_kernel<2, 1>), grid, dim3(COEF_THREADS), 0, stream, frames, first_frame, width, height, rgb ? 1 : 0,
                       quant, coefficients, nb);
  else
    hipLaunchKernelGGL((jpeg_coefficients_kernel<2, 2>), grid, dim3(COEF_THREADS), 0, stream, frames, first_frame, width, height, rgb ? 1 : 0,
                       quant, coefficients, nb);
  return pmce_check_launch("jpeg_encode_coefficients");
}

extern "C" int pmce_jpeg_encode_entropy(const short* coefficients, int n_frames, long long mcus_per_frame, int luma_blocks, int restart_interval,
                                        const unsigned char* header, int header_bytes, long long capacity, void* workspace,
                                        size_t workspace_bytes, unsigned char* data, long long data_bytes, long long* offsets, int* status,
                                        long long first_frame, int stage, hipStream_t stream) {
  PMCE_REQUIRE(coefficients && header && workspace && data && offsets && status, "jpeg_encode_entropy: null pointer");
  Layout L;
  PMCE_REQUIRE(make_layout(n_frames, mcus_per_frame, luma_blocks, restart_interval, L),
               "jpeg_encode_entropy: need 1 .. 65535 frames of 1 .. 2^22 MCUs, 1, 2 or 4 luma blocks per MCU, a restart interval of 0 .. 65535 "
               "and fewer than 2^31 blocks and pieces together (got %d, %lld, %d, %d)",
               n_frames, mcus_per_frame, luma_blocks, restart_interval);
  PMCE_REQUIRE(header_bytes >= 2 && header_bytes <= 4096 && capacity >= 0 && data_bytes >= 0 && first_frame >= 0,
               "jpeg_encode_entropy: need a header of 2 .. 4096 bytes, capacity >= 0, data_bytes >= 0, first_frame >= 0 (got %d, %lld, %lld, %lld)",
               header_bytes, capacity, data_bytes, first_frame);
  PMCE_REQUIRE(stage >= -1 && stage < ENTROPY_STAGES, "jpeg_encode_entropy: stage must be -1 or 0 .. %d (got %d)", ENTROPY_STAGES - 1, stage);
  PMCE_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)coefficients & 1) == 0, "jpeg_encode_entropy: the workspace must be 16-byte aligned");
  if (workspace_bytes < L.total) {
    pmce_set_error("jpeg_encode_entropy: the workspace has %zu bytes, %zu are needed", workspace_bytes, L.total);
    return PMCE_ERR_WORKSPACE;
  }
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  unsigned* ustream = reinterpret_cast<unsigned*>(ws + L.o_stream);
  int* block_bits = reinterpret_cast<int*>(ws + L.o_bits);
  long long* block_off = reinterpret_cast<long long*>(ws + L.o_off);
  long long* interval_bits = reinterpret_cast<long long*>(ws + L.o_ibits);
  int* piece_len = reinterpret_cast<int*>(ws + L.o_plen);
  long long* piece_pos = reinterpret_cast<long long*>(ws + L.o_ppos);
  long long* frame_total = reinterpret_cast<long long*>(ws + L.o_ftot);
  const long long n = n_frames, blocks = n * L.nb, pieces = n * L.NP;
  const long long restart = restart_interval < mcus_per_frame ? restart_interval : 0;       // one interval: no marker inside the scan
  const auto run = [&](int s) { return stage < 0 || stage == s; };
  if (run(0)) {
    hipLaunchKernelGGL(jpeg_lengths_kernel, dim3((unsigned)((blocks + 3) / 4)), dim3(256), 0, stream, coefficients, blocks, L.nb, luma_blocks,
                       restart, block_bits);
    PMCE_TRY(pmce_check_launch("jpeg_encode_entropy (lengths)"));
  }
  if (run(1)) {
    hipLaunchKernelGGL(jpeg_segment_scan_kernel, dim3((unsigned)(n * L.n_int)), dim3(jc::SCAN_THREADS), 0, stream, block_bits, block_off,
                       interval_bits, L.nb, L.bpi, L.n_int);
    PMCE_TRY(pmce_check_launch("jpeg_encode_entropy (offsets)"));
  }
  if (run(2)) {
    const hipError_t rc = hipMemsetAsync(ustream, 0, (size_t)(n * L.n_int * L.slot), stream);
    if (rc != hipSuccess) {
      pmce_set_error("jpeg_encode_entropy: hipMemsetAsync failed: %s", hipGetErrorString(rc));
      return PMCE_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpeg_bits_kernel, dim3((unsigned)((blocks + 3) / 4)), dim3(256), 0, stream, coefficients, blocks, L.nb, luma_blocks,
                       restart, block_off, L.n_int, L.slot, ustream);
    PMCE_TRY(pmce_check_launch("jpeg_encode_entropy (bits)"));
  }
  if (run(3)) {
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)((pieces + 3) / 4)), dim3(256), 0, stream, ustream, interval_bits, pieces, L.NP, L.P,
                       L.n_int, L.slot, piece_len);
    PMCE_TRY(pmce_check_launch("jpeg_encode_entropy (count)"));
  }
  if (run(4)) {
    hipLaunchKernelGGL(jpeg_segment_scan_kernel, dim3((unsigned)n), dim3(jc::SCAN_THREADS), 0, stream, piece_len, piece_pos, frame_total, L.NP,
                       L.NP, 1ll);
    PMCE_TRY(pmce_check_launch("jpeg_encode_entropy (place)"));
  }
  if (run(5)) {
    hipLaunchKernelGGL(jpeg_frames_kernel, dim3(1), dim3(64), 0, stream, frame_total, n_frames, header_bytes, capacity, data_bytes, first_frame,
                       offsets, status);
    PMCE_TRY(pmce_check_launch("jpeg_encode_entropy (frames)"));
  }
  if (run(6)) {
    hipLaunchKernelGGL(jpeg_write_kernel, dim3((unsigned)((pieces + 3) / 4)), dim3(256), 0, stream, ustream, interval_bits, piece_pos, pieces,
                       L.NP, L.P, L.n_int, L.slot, header, header_bytes, first_frame, offsets, status, data);
    PMCE_TRY(pmce_check_launch("jpeg_encode_entropy (write)"));
  }
  return PMCE_OK;
}
