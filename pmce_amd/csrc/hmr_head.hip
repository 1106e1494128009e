// SPIN's regression head on device (reference kasvii/PMCE lib/models/spin.py:145-208 HMR.forward after the backbone, the same head as
// Regressor.forward :211-293): features [n,2048] -> the state (6D pose 144, shape 10, camera 3), the 24 rotation matrices, theta.
//
// In eval mode there is nothing non-linear between fc1, fc2 and the three decoders, so n_iter iterations from an initial state s_0 are
// one affine map  s_n = P s_0 + Q xf + c_n  (pmce_amd.hmr.fold_regressor builds Q [157 x 2048], P [157 x 157] and c_n in fp64 and rounds
// them to fp32 once).  With the shared mean parameters P s_0 + c_n is one constant and only Q is applied here.  With per-sample initial
// states the kernel is handed P - I and computes  s_0 + (c_n + Q xf + (P - I) s_0):  P is the identity plus a small correction, and a
// diagonal rounded as 1 + eps loses eps's low bits, while 157 terms summed at the magnitude of the state lose 4 x as much as the
// reference's own fp32 iteration (measured); the correction summed on its own and added to s_0 once loses less than that iteration.
//
//   hmr_head_kernel    one workgroup of 768 lanes per batch tile of 16 samples.  The 2048-long sum is cut into four slices of 512, one per
//                      group of three waves; in a group lane j < 160 owns state entry j for the 16 samples (16 accumulators), reads
//                      Q^T[k][j] - 640 contiguous bytes per k for the group, L2-resident: Q is 1.3 MB - and the 16 features of step k as
//                      four 16-byte LDS broadcasts.  The four partial sums are added in one fixed order, then the constant, then - with
//                      a per-sample initial state - the 157 terms of (P - I) s_0 in index order, then s_0.  Every product is a plain fp32
//                      fmaf: with Q = 0, P = I, c = 0 the map returns s_0 to the bit, which is how the tests drive the rotation stage
//                      with chosen vectors.
//                      Then one lane per (sample, joint): rot6d_to_rotmat (lib/geometry.py:346-360) and rotation_matrix_to_angle_axis
//                      (:84-249), operation by operation as torch's fp32 runs them (contraction off: torch fuses nothing).
//   hmr_joints_kernel  one wave per sample: the 49 joints of lib/models/smpl_mps.py:65-83 - a posed SMPL joint, or a CSR row times the
//                      vertices (one vertex with weight 1, or a row of J_regressor_extra) - and the weak-perspective projection of
//                      spin.py:309-353 in closed form.
// A sample's numbers are a function of its own row alone (a tail tile computes on zeros and stores nothing), sums run in a fixed order
// that does not depend on n or on the sample's place in the batch: the same bits whatever the batch.  No atomics, no host wait.
//
// Why not the three-product f16 matrix path of gemm_split_f16.hip: the whole product is 0.77 GFLOP for 2400 samples - tens of
// microseconds on the vector pipe, next to a backbone of seconds; the split would need a pass that pre-splits the features, M = 157 is
// no multiple of its tiles, and its products are not exact fp32 products, which the identity property above needs.
#include "common.hpp"
#include "rotation.hpp"

namespace {

constexpr int HMR_F = 2048;              // features
constexpr int HMR_S = 157;               // state: 144 + 10 + 3
constexpr int HMR_SP = 160;              // a row of Q^T / P^T: 157 + 3 zeros
constexpr int HMR_TB = 16;               // samples per workgroup
constexpr int HMR_KS = 4;                // slices of the feature sum
constexpr int HMR_ST = 192;              // lanes per slice (three waves, 160 of them accumulate)
constexpr int HMR_NT = HMR_KS * HMR_ST;  // 768
constexpr int HMR_KC = 128;              // features per slice staged at a time
constexpr int HMR_CLD = 20;              // LDS row of one feature: 16 samples + 4 pad (16-byte aligned rows, 8 banks for the transposing fill)
constexpr int HMR_J = 24;
constexpr int HMR_THETA = 85;
constexpr int HMR_MAX_K = 256;

// rot6d_to_rotmat + rotation_matrix_to_angle_axis for one joint; x: the joint's six numbers
__device__ __forceinline__ void rot6d_rotmat_aa(const float* x, float* R, float* aa) {
#pragma clang fp contract(off)
  // geometry.py:347-358.  reshape(-1, 3, 2): a1 = elements 0, 2, 4, a2 = elements 1, 3, 5.  F.normalize(v, eps) = v / max(|v|, eps)
  const float a1x = x[0], a1y = x[2], a1z = x[4], a2x = x[1], a2y = x[3], a2z = x[5];
  const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-6f);
  const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
  const float dot = b1x * a2x + b1y * a2y + b1z * a2z;
  const float ux = a2x - dot * b1x, uy = a2y - dot * b1y, uz = a2z - dot * b1z;
  const float n2 = fmaxf(sqrtf(ux * ux + uy * uy + uz * uz), 1e-6f);
  const float b2x = ux / n2, b2y = uy / n2, b2z = uz / n2;
  const float b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
  // the vectors are the COLUMNS
  R[0] = b1x, R[1] = b2x, R[2] = b3x;
  R[3] = b1y, R[4] = b2y, R[5] = b3y;
  R[6] = b1z, R[7] = b2z, R[8] = b3z;
  rotmat_to_angle_axis(R, aa);  // geometry.py:169-249 + :146-166 (rotation.hpp)
}

__global__ __launch_bounds__(HMR_NT) void hmr_head_kernel(const float* __restrict__ features, const float* __restrict__ q_t,
                                                          const float* __restrict__ cst, const float* __restrict__ pmi_t,
                                                          const float* __restrict__ init, int n, float* __restrict__ state,
                                                          float* __restrict__ rotmat, float* __restrict__ theta) {
  // the staged features [slice][k][sample] during the sum, the four partial sums [slice][sample][160] after it: 40 KB either way
  __shared__ __attribute__((aligned(16))) float sBuf[HMR_KS * HMR_TB * HMR_SP];
  __shared__ float sState[HMR_TB][HMR_SP];
  static_assert(HMR_KS * HMR_KC * HMR_CLD <= HMR_KS * HMR_TB * HMR_SP, "the feature stage must fit the buffer of the partial sums");
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * HMR_TB;
  const int slice = tid / HMR_ST, j = tid % HMR_ST;
  float acc[HMR_TB];
#pragma unroll
  for (int t = 0; t < HMR_TB; ++t) acc[t] = 0.f;

  for (int c = 0; c < HMR_F / (HMR_KS * HMR_KC); ++c) {
    if (c) __syncthreads();
    // (k runs fastest: neighbouring lanes read neighbouring features of one sample and transpose on the way into LDS)
    for (int i = tid; i < HMR_KS * HMR_KC * HMR_TB; i += HMR_NT) {
      const int kk = i % HMR_KC, t = (i / HMR_KC) % HMR_TB, q = i / (HMR_KC * HMR_TB);
      const int s = s0 + t;
      const int k = q * (HMR_F / HMR_KS) + c * HMR_KC + kk;
      sBuf[(q * HMR_KC + kk) * HMR_CLD + t] = s < n ? features[(size_t)s * HMR_F + k] : 0.f;
    }
    __syncthreads();
    if (j < HMR_SP) {
      const float* qrow = q_t + (size_t)(slice * (HMR_F / HMR_KS) + c * HMR_KC) * HMR_SP + j;
      const float* frow = sBuf + slice * HMR_KC * HMR_CLD;
      for (int k4 = 0; k4 < HMR_KC; k4 += 4) {
        float qv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) qv[u] = qrow[(k4 + u) * HMR_SP];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f32x4* f = reinterpret_cast<const f32x4*>(frow + (k4 + u) * HMR_CLD);
#pragma unroll
          for (int t4 = 0; t4 < HMR_TB / 4; ++t4) {
            const f32x4 fv = f[t4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * t4 + e] = fmaf(qv[u], fv[e], acc[4 * t4 + e]);
          }
        }
      }
    }
  }
  __syncthreads();
  if (j < HMR_SP) {
#pragma unroll
    for (int t = 0; t < HMR_TB; ++t) sBuf[(slice * HMR_TB + t) * HMR_SP + j] = acc[t];
  }
  __syncthreads();
  // the state: the four slices in one fixed order, the constant, then (P - I) s_0 term by term, then s_0
  for (int i = tid; i < HMR_TB * HMR_SP; i += HMR_NT) {
    const int t = i / HMR_SP, e = i % HMR_SP;
    const int s = s0 + t;
    float v = (sBuf[(0 * HMR_TB + t) * HMR_SP + e] + sBuf[(1 * HMR_TB + t) * HMR_SP + e]) +
              (sBuf[(2 * HMR_TB + t) * HMR_SP + e] + sBuf[(3 * HMR_TB + t) * HMR_SP + e]);
    if (e < HMR_S) {
      v += cst[e];
      if (pmi_t && s < n) {
        const float* in = init + (size_t)s * HMR_S;
        for (int k = 0; k < HMR_S; ++k) v = fmaf(pmi_t[k * HMR_SP + e], in[k], v);
        v = in[e] + v;
      }
      if (s < n) state[(size_t)s * HMR_S + e] = v;
    }
    sState[t][e] = v;
  }
  __syncthreads();
  if (tid < HMR_TB * HMR_J) {
    const int t = tid / HMR_J, jn = tid % HMR_J;
    const int s = s0 + t;
    if (s < n) {
      float R[9], aa[3];
      rot6d_rotmat_aa(&sState[t][6 * jn], R, aa);
      float* ro = rotmat + ((size_t)s * HMR_J + jn) * 9;
#pragma unroll
      for (int e = 0; e < 9; ++e) ro[e] = R[e];
      float* th = theta + (size_t)s * HMR_THETA + 3 + 3 * jn;
      th[0] = aa[0], th[1] = aa[1], th[2] = aa[2];
    }
  } else if (tid < HMR_TB * HMR_J + HMR_TB * 13) {
    // theta = (cam 3, axis-angle 72, shape 10)
    const int i = tid - HMR_TB * HMR_J;
    const int t = i / 13, e = i % 13;
    const int s = s0 + t;
    if (s < n) theta[(size_t)s * HMR_THETA + (e < 3 ? e : 72 + e)] = e < 3 ? sState[t][154 + e] : sState[t][144 + (e - 3)];
  }
}

__global__ __launch_bounds__(64) void hmr_joints_kernel(const float* __restrict__ joints, const float* __restrict__ verts,
                                                        const int* __restrict__ sel, const int* __restrict__ indptr,
                                                        const int* __restrict__ indices, const float* __restrict__ data,
                                                        const float* __restrict__ cam, int cam_stride, int K, int V,
                                                        float* __restrict__ kp_3d, float* __restrict__ kp_2d) {
#pragma clang fp contract(off)
  const int s = blockIdx.x;
  const float c0 = cam[(size_t)s * cam_stride + 0], c1 = cam[(size_t)s * cam_stride + 1], c2 = cam[(size_t)s * cam_stride + 2];
  // spin.py:310-312
  const float tz = 2.0f * 5000.0f / (224.0f * c0 + 1e-9f);
  for (int k = threadIdx.x; k < K; k += 64) {
    float x, y, z;
    const int src = sel[k];
    if (src >= 0) {
      const float* p = joints + ((size_t)s * HMR_J + min(src, HMR_J - 1)) * 3;
      x = p[0], y = p[1], z = p[2];
    } else {
      x = y = z = 0.f;
      for (int e = indptr[k]; e < indptr[k + 1]; ++e) {
        const float w = data[e];
        const float* p = verts + ((size_t)s * V + min(max(indices[e], 0), V - 1)) * 3;
        x = fmaf(w, p[0], x), y = fmaf(w, p[1], y), z = fmaf(w, p[2], z);
      }
    }
    float* o3 = kp_3d + ((size_t)s * K + k) * 3;
    o3[0] = x, o3[1] = y, o3[2] = z;
    // spin.py:344-353 with the identity rotation, a zero centre and focal length 5000, then :321
    const float px = x + c1, py = y + c2, pz = z + tz;
    float* o2 = kp_2d + ((size_t)s * K + k) * 2;
    o2[0] = 5000.0f * (px / pz) / 112.0f;
    o2[1] = 5000.0f * (py / pz) / 112.0f;
  }
}

}  // namespace

extern "C" int pmce_hmr_head_batch_tile(void) { return HMR_TB; }

extern "C" int pmce_hmr_head_f32(const float* features, const float* q_t, const float* cst, const float* pmi_t, const float* init, int n,
                                 float* state, float* rotmat, float* theta, hipStream_t stream) {
  const char* what = "hmr_head";
  PMCE_REQUIRE(n >= 1, "%s: n must be >= 1 (got %d)", what, n);
  PMCE_REQUIRE(n <= 65535 * HMR_TB, "%s: n = %d is more than one launch takes (%d)", what, n, 65535 * HMR_TB);
  PMCE_REQUIRE(features && q_t && cst && state && rotmat && theta, "%s: null pointer", what);
  PMCE_REQUIRE((pmi_t != nullptr) == (init != nullptr), "%s: P - I and the per-sample initial state go together (both or neither)", what);
  PMCE_REQUIRE(((uintptr_t)features & 3) == 0 && ((uintptr_t)q_t & 3) == 0, "%s: misaligned pointer", what);
  hipLaunchKernelGGL(hmr_head_kernel, dim3((n + HMR_TB - 1) / HMR_TB), dim3(HMR_NT), 0, stream, features, q_t, cst, pmi_t, init, n, state,
                     rotmat, theta);
  return pmce_check_launch(what);
}

extern "C" int pmce_hmr_joints_f32(const float* joints, const float* verts, const int* sel, const int* indptr, const int* indices,
                                   const float* data, const float* cam, int cam_stride, int n, int K, int V, float* kp_3d, float* kp_2d,
                                   hipStream_t stream) {
  const char* what = "hmr_joints";
  PMCE_REQUIRE(n >= 1, "%s: n must be >= 1 (got %d)", what, n);
  PMCE_REQUIRE(K >= 1 && K <= HMR_MAX_K, "%s: K must be in 1..%d (got %d)", what, HMR_MAX_K, K);
  PMCE_REQUIRE(V >= 1, "%s: V must be >= 1 (got %d)", what, V);
  PMCE_REQUIRE(cam_stride >= 3, "%s: cam_stride must be >= 3 (got %d)", what, cam_stride);
  PMCE_REQUIRE(joints && verts && sel && indptr && indices && data && cam && kp_3d && kp_2d, "%s: null pointer", what);
  hipLaunchKernelGGL(hmr_joints_kernel, dim3(n), dim3(64), 0, stream, joints, verts, sel, indptr, indices, data, cam, cam_stride, K, V,
                     kp_3d, kp_2d);
  return pmce_check_launch(what);
}
