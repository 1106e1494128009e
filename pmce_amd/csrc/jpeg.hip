// The demo's frames from JPEG files (baseline, Huffman), decoded on the device: what the reference does with cv2.imread, four or more
// times per frame (lib/utils/demo_utils.py:101-121 writes the files; main/run_demo.py:264-286, 392-395 and lib/utils/_dataset_demo.py:60
// read them back).  pmce_amd/jpeg.py parses the markers on the host and writes the records (include/pmce_hip.h); three stages follow:
//
//   pmce_jpeg_entropy   one lane per restart interval (per image without DRI): bit reader, Huffman decode, EXTEND, DC prediction,
//                       run/size pairs -> int16 coefficients in natural order, blocks in scan order.  The body is jpeg_entropy.hpp,
//                       shared with the host program that checks its bounds.  A lane's branches are its own, so a wavefront is given
//                       as few segments as still fill the chip (`lanes` of its 64): 32 images are 32 wavefronts of one lane each.
//                       A lane reads its bytes through a 64-byte window in LDS, reads the Huffman tables from LDS and puts each
//                       block together in LDS (a wave's loads wait for its older stores).  One lane is still a slow decoder - about a
//                       microsecond per byte, DESIGN.md section 8 - so the stage's speed is the number of segments in flight.
//   pmce_jpeg_idct      one lane per 8 x 8 block: dequantisation and libjpeg's jidctint ("islow", CONST_BITS 13, PASS1_BITS 2) ->
//                       one uint8 plane per component at the component's own resolution, padded to whole blocks.
//   pmce_jpeg_colour    libjpeg's "fancy" chroma upsampling (jdsample h2v1 / h2v2, on the real chroma extent) and jdcolor's fixed-point
//                       YCbCr -> RGB, four pixels per lane -> frames[F][H][W][3] in B, G, R or R, G, B; it also reduces the segments'
//                       status words to one per image.
//
// Integer arithmetic throughout and no atomics: the same bits whatever the batch and an image's place in it.
#include "common.hpp"
#include "jpeg_entropy.hpp"

namespace {

namespace je = jpeg_entropy;
constexpr int MAX_DIM = 16384;
constexpr int IDCT_THREADS = 256;            // blocks (8 x 8) per workgroup of the inverse DCT
constexpr int COLOUR_TX = 64, COLOUR_TY = 4, COLOUR_PX = 4;      // a workgroup of the colour stage: 256 pixels x 4 rows

// ---------------------------------------------------------------------------------------------------------------------------------------
// entropy decode
// ---------------------------------------------------------------------------------------------------------------------------------------
// A lane's scratch is LDS: the block it puts together, the window through which it reads its segment's bytes (jpeg_entropy.hpp) and -
// LDS_TABLES, when the batch has at most MAX_LDS_TABLES distinct Huffman tables, which is every folder ffmpeg or cv2.imwrite wrote:
// they use the standard four - the tables themselves.  Dynamic LDS: block[lanes][64] int16 | window[lanes][WINDOW] | tables.
constexpr int MAX_LDS_TABLES = 16;
constexpr int LANE_LDS_BYTES = 64 * (int)sizeof(short) + je::WINDOW;
template <bool LDS_TABLES>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const unsigned char* __restrict__ data, long long n_bytes,
                                                          const int* __restrict__ segments, int seg0, int n_seg,
                                                          const int* __restrict__ images, int n_images, const int* __restrict__ huffman,
                                                          int n_huffman, short* __restrict__ coef, long long n_blocks,
                                                          int* __restrict__ seg_status, int lanes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  short* block = reinterpret_cast<short*>(lds);
  unsigned char* window = lds + lanes * 64 * (int)sizeof(short);
  int* tables = reinterpret_cast<int*>(lds + lanes * LANE_LDS_BYTES);
  for (int i = threadIdx.x; i < lanes * 64; i += 64) block[i] = 0;
  if (LDS_TABLES)
    for (int i = threadIdx.x; i < n_huffman * je::HUFF_WORDS; i += 64) tables[i] = huffman[i];
  __syncthreads();
  if ((int)threadIdx.x >= lanes) return;
  const int s = blockIdx.x * lanes + threadIdx.x;
  if (s >= n_seg) return;
  seg_status[seg0 + s] = je::decode_segment<true>(data, n_bytes, segments + (long long)(seg0 + s) * je::SEG_WORDS, images, n_images,
                                                  LDS_TABLES ? tables : huffman, n_huffman, coef, n_blocks,
                                                  window + threadIdx.x * je::WINDOW, block + threadIdx.x * 64);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// dequantise + inverse DCT (jidctint.c, jpeg_idct_islow; the all-zero shortcut of its column pass gives the same values and is left out)
// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270, FIX_0_899976223 = 7373,
              FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137, FIX_1_961570560 = 16069,
              FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// eight inputs -> eight outputs, descaled by SHIFT with rounding
template <int SHIFT>
__device__ __forceinline__ void idct8(int i0, int i1, int i2, int i3, int i4, int i5, int i6, int i7, int* o) {
  int z2 = i2, z3 = i6;
  int z1 = (z2 + z3) * FIX_0_541196100;
  int tmp2 = z1 + z3 * (-FIX_1_847759065);
  int tmp3 = z1 + z2 * FIX_0_765366865;
  int tmp0 = (int)((unsigned)(i0 + i4) << 13);
  int tmp1 = (int)((unsigned)(i0 - i4) << 13);
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = i7;
  tmp1 = i5;
  tmp2 = i3;
  tmp3 = i1;
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  tmp0 *= FIX_0_298631336;
  tmp1 *= FIX_2_053119869;
  tmp2 *= FIX_3_072711026;
  tmp3 *= FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 *= -FIX_1_961570560;
  z4 *= -FIX_0_390180644;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  constexpr int BIAS = 1 << (SHIFT - 1);
  o[0] = (tmp10 + tmp3 + BIAS) >> SHIFT;
  o[7] = (tmp10 - tmp3 + BIAS) >> SHIFT;
  o[1] = (tmp11 + tmp2 + BIAS) >> SHIFT;
  o[6] = (tmp11 - tmp2 + BIAS) >> SHIFT;
  o[2] = (tmp12 + tmp1 + BIAS) >> SHIFT;
  o[5] = (tmp12 - tmp1 + BIAS) >> SHIFT;
  o[3] = (tmp13 + tmp0 + BIAS) >> SHIFT;
  o[4] = (tmp13 - tmp0 + BIAS) >> SHIFT;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

// grid (blocks of the largest image / IDCT_THREADS, images of the round).  quant[n_quant][64] uint16, zigzag order as stored.
__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const short* __restrict__ coef, const int* __restrict__ images,
                                                                 int image0, const unsigned short* __restrict__ quant, int n_quant,
                                                                 unsigned char* __restrict__ planes, long long n_blocks,
                                                                 long long plane_bytes) {
  __shared__ int q[3][64];       // natural order
  const int* im = images + (long long)(image0 + blockIdx.y) * je::IMG_WORDS;
  const int ncomp = im[je::IM_NCOMP];
  if (threadIdx.x < 64 * 3) {
    const int c = threadIdx.x >> 6, k = threadIdx.x & 63;
    const int t = im[je::IM_QUANT + (c < ncomp ? c : 0)];
    q[c][je::natural_index(k)] = (t >= 0 && t < n_quant) ? quant[t * 64 + k] : 0;
  }
  __syncthreads();
  if (!je::check_image(im)) return;
  const int h = im[je::IM_H], v = im[je::IM_V], mx = im[je::IM_MCUS_X], my = im[je::IM_MCUS_Y], bpm = im[je::IM_BLOCKS_PER_MCU];
  const int b = blockIdx.x * IDCT_THREADS + threadIdx.x;
  if (b >= mx * my * bpm) return;
  const int mcu = b / bpm, k = b - mcu * bpm;
  const int luma = ncomp == 1 ? 1 : h * v;
  const int c = k < luma ? 0 : k - luma + 1;                 // component
  const int kc = c == 0 ? k : 0, hc = c == 0 ? h : 1, vc = c == 0 ? v : 1;
  const int mcu_y = mcu / mx, mcu_x = mcu - mcu_y * mx;
  const int bx = mcu_x * hc + kc % hc, by = mcu_y * vc + kc / hc;
  const int stride = mx * hc * 8;
  // the planes of an image follow each other: luma (mx h 8) x (my v 8), then the two chroma planes (mx 8) x (my 8)
  const size_t luma_bytes = (size_t)(mx * h * 8) * (size_t)(my * v * 8), chroma_bytes = (size_t)(mx * 8) * (size_t)(my * 8);
  // records that do not fit the workspace (pmce_amd/jpeg.py writes none) are not followed
  if ((long long)im[je::IM_BLOCK0] + (long long)mx * my * bpm > n_blocks ||
      (long long)im[je::IM_PLANE0] + (long long)(luma_bytes + (ncomp == 3 ? 2 * chroma_bytes : 0)) > plane_bytes)
    return;
  unsigned char* plane = planes + (size_t)im[je::IM_PLANE0] + (c == 0 ? 0 : luma_bytes + (size_t)(c - 1) * chroma_bytes);

  const short* src = coef + ((long long)im[je::IM_BLOCK0] + b) * 64;
  int x[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int4 w = *reinterpret_cast<const int4*>(src + 8 * r);
    const int u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[8 * r + 2 * e] = (int)(short)(u[e] & 0xffff) * q[c][8 * r + 2 * e];
      x[8 * r + 2 * e + 1] = (u[e] >> 16) * q[c][8 * r + 2 * e + 1];
    }
  }
  int ws[64];
#pragma unroll
  for (int col = 0; col < 8; ++col) {       // pass 1: down each column
    int o[8];
    idct8<11>(x[col], x[8 + col], x[16 + col], x[24 + col], x[32 + col], x[40 + col], x[48 + col], x[56 + col], o);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[8 * r + col] = o[r];
  }
  unsigned char* dst = plane + (size_t)(by * 8) * stride + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {             // pass 2: along each row
    int o[8];
    idct8<18>(ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4], ws[8 * r + 5], ws[8 * r + 6], ws[8 * r + 7], o);
    uint2 px;
    px.x = clamp255(o[0] + 128) | (clamp255(o[1] + 128) << 8) | (clamp255(o[2] + 128) << 16) | (clamp255(o[3] + 128) << 24);
    px.y = clamp255(o[4] + 128) | (clamp255(o[5] + 128) << 8) | (clamp255(o[6] + 128) << 16) | (clamp255(o[7] + 128) << 24);
    *reinterpret_cast<uint2*>(dst + (size_t)r * stride) = px;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// upsample + colour + store
// ---------------------------------------------------------------------------------------------------------------------------------------
// One chroma sample at output pixel (x, y).  The plane's real extent is cw x ch; hs, vs: 1 where the plane is halved in that direction.
// jdsample filters only planes wider than two columns; narrower ones it replicates.
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int stride, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 0) return p[(size_t)y * stride + x];
  const int cx = x >> 1;
  if (cw <= 2) return p[(size_t)(y >> vs) * stride + cx];
  if (vs == 0) {                                     // h2v1
    const unsigned char* row = p + (size_t)y * stride;
    const int c = row[cx];
    if (x & 1) return cx == cw - 1 ? c : (3 * c + row[cx + 1] + 2) >> 2;
    return cx == 0 ? c : (3 * c + row[cx - 1] + 1) >> 2;
  }
  const int cy = y >> 1;                             // h2v2
  const int far = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  const unsigned char* rn = p + (size_t)cy * stride;
  const unsigned char* rf = p + (size_t)far * stride;
  const int s = 3 * rn[cx] + rf[cx];
  if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * rn[cx + 1] + rf[cx + 1] + 7) >> 4;
  return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * rn[cx - 1] + rf[cx - 1] + 8) >> 4;
}

// grid (W / 256, H / 4, images of the round); block (64, 4).  ALIGNED: W % 4 == 0 and a 4-byte aligned `frames`, so that a lane's
// four pixels are three whole words.
template <bool ALIGNED>
__global__ __launch_bounds__(COLOUR_TX* COLOUR_TY) void jpeg_colour_kernel(const unsigned char* __restrict__ planes,
                                                                           const int* __restrict__ images, int image0,
                                                                           const int* __restrict__ seg_status, int n_seg_total, int W,
                                                                           int H, int rgb, unsigned char* __restrict__ frames,
                                                                           int* __restrict__ status, long long plane_bytes) {
  const int image = image0 + blockIdx.z;
  const int* im = images + (long long)image * je::IMG_WORDS;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
    int st = 0;
    const int s0 = im[je::IM_SEG0], n = im[je::IM_NSEG];
    for (int s = s0; s < s0 + n; ++s) st |= (s >= 0 && s < n_seg_total) ? seg_status[s] : je::STATUS_RECORD;
    status[image] = st;
  }
  const int x0 = (blockIdx.x * COLOUR_TX + threadIdx.x) * COLOUR_PX, y = blockIdx.y * COLOUR_TY + threadIdx.y;
  if (x0 >= W || y >= H || !je::check_image(im)) return;
  const int ncomp = im[je::IM_NCOMP], h = im[je::IM_H], v = im[je::IM_V], mx = im[je::IM_MCUS_X], my = im[je::IM_MCUS_Y];
  const int ls = mx * h * 8, cs = mx * 8;
  const size_t luma_bytes = (size_t)ls * (size_t)(my * v * 8), chroma_bytes = (size_t)cs * (size_t)(my * 8);
  if ((long long)im[je::IM_PLANE0] + (long long)(luma_bytes + (ncomp == 3 ? 2 * chroma_bytes : 0)) > plane_bytes ||
      ls < W || my * v * 8 < H)
    return;
  const unsigned char* py = planes + (size_t)im[je::IM_PLANE0];
  const unsigned char* pcb = py + luma_bytes;
  const unsigned char* pcr = pcb + chroma_bytes;
  const int hs = h - 1, vs = v - 1, cw = (W + hs) >> hs, ch = (H + vs) >> vs;
  unsigned char out[3 * COLOUR_PX];
#pragma unroll
  for (int i = 0; i < COLOUR_PX; ++i) {
    const int x = min(x0 + i, W - 1);
    const int Y = py[(size_t)y * ls + x];
    int r = Y, g = Y, b = Y;
    if (ncomp == 3) {
      const int cb = chroma_at(pcb, cs, cw, ch, hs, vs, x, y) - 128, cr = chroma_at(pcr, cs, cw, ch, hs, vs, x, y) - 128;
      r = (int)clamp255(Y + ((91881 * cr + 32768) >> 16));
      g = (int)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      b = (int)clamp255(Y + ((116130 * cb + 32768) >> 16));
    }
    out[3 * i] = (unsigned char)(rgb ? r : b);
    out[3 * i + 1] = (unsigned char)g;
    out[3 * i + 2] = (unsigned char)(rgb ? b : r);
  }
  unsigned char* dst = frames + (((size_t)image * H + y) * W + x0) * 3;
  if (ALIGNED) {
    unsigned* d = reinterpret_cast<unsigned*>(dst);
#pragma unroll
    for (int wd = 0; wd < 3; ++wd)
      d[wd] = out[4 * wd] | ((unsigned)out[4 * wd + 1] << 8) | ((unsigned)out[4 * wd + 2] << 16) | ((unsigned)out[4 * wd + 3] << 24);
  } else {
    const int n = min(COLOUR_PX, W - x0) * 3;
#pragma unroll
    for (int i = 0; i < 3 * COLOUR_PX; ++i)
      if (i < n) dst[i] = out[i];
  }
}

}  // namespace

extern "C" int pmce_jpeg_entropy(const unsigned char* data, long long n_bytes, const int* segments, int first_segment, int n_segments,
                                 const int* images, int n_images, const int* huffman, int n_huffman, short* coefficients,
                                 long long n_blocks, int* segment_status, int lds_tables, int lanes, hipStream_t stream) {
  PMCE_REQUIRE(data && segments && images && huffman && coefficients && segment_status, "jpeg_entropy: null pointer");
  // (a lane's window reaches up to WINDOW bytes past the byte it reads: offsets stay clear of the end of int)
  PMCE_REQUIRE(n_bytes >= 1 && n_bytes <= 0x7fffffffll - 2 * je::WINDOW, "jpeg_entropy: need 1 .. 2^31 - 129 bytes of files (got %lld)",
               n_bytes);
  PMCE_REQUIRE(lanes >= 0 && lanes <= 64, "jpeg_entropy: lanes must be 0 (chosen here) or 1 .. 64 (got %d)", lanes);
  PMCE_REQUIRE(first_segment >= 0 && n_segments >= 1 && n_images >= 1 && n_huffman >= 1,
               "jpeg_entropy: need first_segment >= 0 and at least one segment, image and Huffman table (got %d, %d, %d, %d)",
               first_segment, n_segments, n_images, n_huffman);
  PMCE_REQUIRE(((uintptr_t)coefficients & 15) == 0, "jpeg_entropy: the coefficient buffer must be 16-byte aligned");
  PMCE_REQUIRE(n_blocks >= 1 && n_blocks <= (1ll << 40), "jpeg_entropy: need 1 .. 2^40 coefficient blocks (got %lld)", n_blocks);
  const hipError_t rc = hipMemsetAsync(coefficients, 0, (size_t)n_blocks * 64 * sizeof(short), stream);
  if (rc != hipSuccess) {
    pmce_set_error("jpeg_entropy: hipMemsetAsync failed: %s", hipGetErrorString(rc));
    return PMCE_ERR_LAUNCH;
  }
  // As few lanes per wavefront as still give every segment a lane within 4096 wavefronts: lanes of one wavefront that decode
  // different streams take their branches one after the other, wavefronts do not, and 4096 of them with a lane's LDS each are resident.
  // (`lanes` != 0 is the caller's choice: the tests' way to the forms a large round takes.)
  if (lanes == 0) {
    lanes = (n_segments + 4095) / 4096;
    lanes = lanes < 1 ? 1 : (lanes > 64 ? 64 : lanes);
  }
  const dim3 grid((unsigned)((n_segments + lanes - 1) / lanes));
  const bool in_lds = n_huffman <= MAX_LDS_TABLES && lds_tables;
  const size_t lds = (size_t)lanes * LANE_LDS_BYTES + (in_lds ? (size_t)n_huffman * je::HUFF_WORDS * sizeof(int) : 0);
  if (in_lds)
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, grid, dim3(64), lds, stream, data, n_bytes, segments, first_segment, n_segments, images,
                       n_images, huffman, n_huffman, coefficients, n_blocks, segment_status, lanes);
  else
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, grid, dim3(64), lds, stream, data, n_bytes, segments, first_segment, n_segments, images,
                       n_images, huffman, n_huffman, coefficients, n_blocks, segment_status, lanes);
  return pmce_check_launch("jpeg_entropy");
}

extern "C" int pmce_jpeg_idct(const short* coefficients, const int* images, int first_image, int n_images, int max_blocks,
                              const unsigned short* quant, int n_quant, long long n_blocks, unsigned char* planes, long long plane_bytes,
                              hipStream_t stream) {
  PMCE_REQUIRE(coefficients && images && quant && planes, "jpeg_idct: null pointer");
  PMCE_REQUIRE(first_image >= 0 && n_images >= 1 && n_images <= 65535 && max_blocks >= 1 && n_quant >= 1,
               "jpeg_idct: need first_image >= 0, 1 .. 65535 images, max_blocks >= 1, n_quant >= 1 (got %d, %d, %d, %d)", first_image,
               n_images, max_blocks, n_quant);
  PMCE_REQUIRE(n_blocks >= 1 && plane_bytes >= 64, "jpeg_idct: need n_blocks >= 1 and plane_bytes >= 64 (got %lld, %lld)", n_blocks,
               plane_bytes);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + IDCT_THREADS - 1) / IDCT_THREADS), (unsigned)n_images),
                     dim3(IDCT_THREADS), 0, stream, coefficients, images, first_image, quant, n_quant, planes, n_blocks, plane_bytes);
  return pmce_check_launch("jpeg_idct");
}

extern "C" int pmce_jpeg_colour(const unsigned char* planes, long long plane_bytes, const int* images, int first_image, int n_images, const int* segment_status,
                                int n_segments_total, int width, int height, int rgb, unsigned char* frames, int* status,
                                hipStream_t stream) {
  PMCE_REQUIRE(planes && images && segment_status && frames && status, "jpeg_colour: null pointer");
  PMCE_REQUIRE(first_image >= 0 && n_images >= 1 && n_images <= 65535 && n_segments_total >= 1,
               "jpeg_colour: need first_image >= 0, 1 .. 65535 images, at least one segment (got %d, %d, %d)", first_image, n_images,
               n_segments_total);
  PMCE_REQUIRE(plane_bytes >= 64, "jpeg_colour: need plane_bytes >= 64 (got %lld)", plane_bytes);
  PMCE_REQUIRE(width >= 1 && width <= MAX_DIM && height >= 1 && height <= MAX_DIM, "jpeg_colour: need a frame of 1..%d x 1..%d (got %d x %d)",
               MAX_DIM, MAX_DIM, width, height);
  const dim3 grid((unsigned)((width + COLOUR_TX * COLOUR_PX - 1) / (COLOUR_TX * COLOUR_PX)), (unsigned)((height + COLOUR_TY - 1) / COLOUR_TY),
                  (unsigned)n_images);
  const dim3 block(COLOUR_TX, COLOUR_TY);
  if (width % 4 == 0 && ((uintptr_t)frames & 3) == 0)
    hipLaunchKernelGGL(jpeg_colour_kernel<true>, grid, block, 0, stream, planes, images, first_image, segment_status, n_segments_total,
                       width, height, rgb ? 1 : 0, frames, status, plane_bytes);
  else
    hipLaunchKernelGGL(jpeg_colour_kernel<false>, grid, block, 0, stream, planes, images, first_image, segment_status, n_segments_total,
                       width, height, rgb ? 1 : 0, frames, status, plane_bytes);
  return pmce_check_launch("jpeg_colour");
}
