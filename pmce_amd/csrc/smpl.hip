// Batched SMPL forward on device: the ground-truth meshes of the evaluation, from the datasets' own SMPL fits.
//
// What is restated (reference kasvii/PMCE), fp32 throughout:
//   * smplpytorch/smplpytorch/pytorch/smpl_layer.py:65-158, SMPL_Layer.forward with center_idx = None, and
//     rodrigues_layer.py:13-52 (batch_rodrigues: the norm of axisang + 1e-8, the half-angle quaternion, quat2mat's renormalisation and
//     its 9-term matrix).  A zero vector gives the identity: norm = sqrt(3) 1e-8, axis = 0 / norm = 0, quaternion (1, 0, 0, 0).
//   * data/PW3D/dataset.py:86,240: mesh * 1000 - root, as the fused output transform  out = (vert + trans) * scale - offset[b].
//   * data/Human36M/dataset.py:354-398, the world -> camera form: root rotation cam_R . R_0 (the reference goes through an axis-angle
//     round trip, the same rotation up to rounding), betas zeroed where any |beta| > 3, translation cam_R trans + cam_t / 1000 - J_0 +
//     cam_R J_0 with J_0 the layer's root joint.  A zero root pose (0 / 0 = NaN in the reference, :370) gives cam_R itself here.
//
// Two launches per call:
//   smpl_pose_kernel   one 64-lane wave per sample: 24 Rodrigues matrices, the 207 pose-map coefficients, the rest joints
//                      J = J_template + J_shapedirs . betas (the regressor was applied to the template and the shape directions once, at
//                      model load, in fp64), the kinematic chain along `parents`, A_i = G_i - pack(G_i [J_i; 0]).  Writes A[B][24][12],
//                      the blend coefficients [B][220] (10 betas, 207 pose-map entries, 3 zeros), the effective translation and the
//                      posed joints.
//   smpl_skin_kernel   (vertex tile of 256) x (batch tile of 16).  The tile's coefficients [220][16] and A matrices [16][288] sit in
//                      LDS (17 KB with row padding + 18 KB) and are read as broadcasts; each lane owns ONE vertex and walks the 217 blend rows once for
//                      the 16 samples, 48 accumulators in registers.  The blend directions are stored [220][3][V] (three zero rows pad
//                      217 to a multiple of four), so a wave's loads are 256 contiguous bytes; the next four rows are requested
//                      while the current four are consumed.  Skinning runs joint by joint: out_t += w[v][j] (A_tj [v_posed_t; 1]) -
//                      the same twelve multiply-adds per (joint, sample) as T = sum_j w A_j followed by T v, without 192 live registers;
//                      a joint whose weight is exactly zero for all 64 vertices of a wave is skipped (a property of the model alone).
// The model is read once per batch tile instead of once per sample: about 32 FLOP per loaded float, so the kernel sits on the vector
// pipe.  No atomics; a sample's result is a function of its own row only (a tail tile computes on zeros and stores nothing), so it
// does not depend on the batch it is in, and two runs give the same bits.  `sample_index` makes one launch serve the samples of one
// gender in place: rows are read and written at the listed indices, nothing is gathered or scattered.
// pmce_smpl_forward_rotmat is the same layer on rotation matrices (smplx's pose2rot = False, what SPIN's regression head calls,
// lib/models/spin.py:184-189): smpl_pose_rotmat_kernel takes the 24 matrices as they are instead of going through Rodrigues' formula; the
// two pose kernels are instantiations of one body, the skinning kernel is shared.
#include "common.hpp"

namespace {

constexpr int SMPL_J = 24;
constexpr int SMPL_K = 217;        // 10 shape + 207 pose-map coefficients
constexpr int SMPL_KP = 220;       // padded to a multiple of 4 (zero rows / zero coefficients)
constexpr int SMPL_TB = 16;        // samples per batch tile
constexpr int SMPL_CLD = 20;       // LDS row of a blend coefficient: 16 samples + 4 pad (16-byte aligned rows, 8 banks for the transposing fill)
constexpr int SMPL_VT = 256;       // vertices per workgroup
constexpr int SMPL_A = SMPL_J * 12;
constexpr int SMPL_WS_FLOATS = SMPL_A + SMPL_KP + 4;   // per sample: A, coefficients, effective translation (+1 pad)

struct SmplParents {
  int p[SMPL_J];
};

__device__ __forceinline__ float* ws_A(float* ws, int s) { return ws + (size_t)s * SMPL_A; }
__device__ __forceinline__ float* ws_coef(float* ws, int B, int s) { return ws + (size_t)B * SMPL_A + (size_t)s * SMPL_KP; }
__device__ __forceinline__ float* ws_trans(float* ws, int B, int s) { return ws + (size_t)B * (SMPL_A + SMPL_KP) + (size_t)s * 4; }

// The pose stage's body, shared by the two kernels below.  ROTMAT = false: `pose` holds 72 axis-angle numbers per sample and goes through
// Rodrigues' formula.  ROTMAT = true (smplx's pose2rot = False, what the HMR head calls): `pose` holds the 24 matrices themselves, row-major,
// and they are taken as they are.  Everything after the matrices - pose map, rest joints, chain, A - is the same text for both.
template <bool ROTMAT>
__device__ __forceinline__ void smpl_pose_body(const float* __restrict__ pose, const float* __restrict__ betas, int betas_stride,
                                               const float* __restrict__ trans, const float* __restrict__ cam_R,
                                               const float* __restrict__ cam_t, const float* __restrict__ j_template,
                                               const float* __restrict__ j_shapedirs, const SmplParents& par,
                                               const int* __restrict__ sample_index, int B, float scale,
                                               const float* __restrict__ offset, float* __restrict__ ws,
                                               float* __restrict__ joints_out) {
  __shared__ float sR[SMPL_J][9];
  __shared__ float sJ[SMPL_J][3];
  __shared__ float sG[SMPL_J][12];
  __shared__ float sBeta[10];
  __shared__ float sT[3];
  const int s = sample_index ? sample_index[blockIdx.x] : (int)blockIdx.x;
  if ((unsigned)s >= (unsigned)B) return;  // block-uniform: a list entry out of range owns no row
  const int lane = threadIdx.x;
  float* coef = ws_coef(ws, B, s);

  // shape: Human36M/dataset.py:365 zeroes the whole row where any |beta| > 3 (camera form only)
  float b = lane < 10 ? betas[(size_t)s * betas_stride + lane] : 0.f;
  if (cam_R && __ballot(lane < 10 && fabsf(b) > 3.0f) != 0ull) b = 0.f;
  if (lane < 10) {
    sBeta[lane] = b;
    coef[lane] = b;
  }
  if (lane < 3) coef[SMPL_K + lane] = 0.f;

  if (ROTMAT) {
    for (int i = lane; i < SMPL_J * 9; i += 64) sR[i / 9][i % 9] = pose[(size_t)s * (SMPL_J * 9) + i];
  } else if (lane < SMPL_J) {  // rodrigues_layer.py:41-52 + :13-38, one joint per lane
    const float a0 = pose[(size_t)s * 72 + 3 * lane + 0], a1 = pose[(size_t)s * 72 + 3 * lane + 1],
                a2 = pose[(size_t)s * 72 + 3 * lane + 2];
    const float e0 = a0 + 1e-8f, e1 = a1 + 1e-8f, e2 = a2 + 1e-8f;
    const float nrm = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    const float h = nrm * 0.5f;
    const float vc = cosf(h), vs = sinf(h);
    float w = vc, x = vs * (a0 / nrm), y = vs * (a1 / nrm), z = vs * (a2 / nrm);
    const float qn = sqrtf(w * w + x * x + y * y + z * z);
    w /= qn, x /= qn, y /= qn, z /= qn;
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    float* r = sR[lane];
    r[0] = w2 + x2 - y2 - z2;
    r[1] = 2 * xy - 2 * wz;
    r[2] = 2 * wy + 2 * xz;
    r[3] = 2 * wz + 2 * xy;
    r[4] = w2 - x2 + y2 - z2;
    r[5] = 2 * yz - 2 * wx;
    r[6] = 2 * xz - 2 * wy;
    r[7] = 2 * wx + 2 * yz;
    r[8] = w2 - x2 - y2 + z2;
  }
  __syncthreads();

  // the rest joints: a 10-term sum on tables the regressor was folded into at load time
  for (int i = lane; i < SMPL_J * 3; i += 64) {
    float j = j_template[i];
#pragma unroll
    for (int k = 0; k < 10; ++k) j += j_shapedirs[i * 10 + k] * sBeta[k];
    sJ[i / 3][i % 3] = j;
  }
  // the pose map: the 23 non-root matrices minus the identity
  for (int i = lane; i < 207; i += 64) {
    const int e = i % 9;
    coef[10 + i] = sR[1 + i / 9][e] - ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f);
  }
  // camera form: the root rotation becomes cam_R . R_0
  float r0 = 0.f;
  if (cam_R && lane < 9) {
    const int r = lane / 3, c = lane % 3;
    const float* cr = cam_R + (size_t)s * 9;
    r0 = cr[3 * r + 0] * sR[0][c] + cr[3 * r + 1] * sR[0][3 + c] + cr[3 * r + 2] * sR[0][6 + c];
  }
  __syncthreads();
  if (cam_R && lane < 9) sR[0][lane] = r0;
  // the effective translation (Human36M/dataset.py:386-390 in the camera form: the layer's root joint output is J_0)
  if (lane < 3) {
    float t = 0.f;
    if (cam_R) {
      const float* cr = cam_R + (size_t)s * 9 + 3 * lane;
      const float t0 = trans ? trans[(size_t)s * 3 + 0] : 0.f, t1 = trans ? trans[(size_t)s * 3 + 1] : 0.f,
                  t2 = trans ? trans[(size_t)s * 3 + 2] : 0.f;
      t = (cr[0] * t0 + cr[1] * t1 + cr[2] * t2) + cam_t[(size_t)s * 3 + lane] / 1000.0f;
      t = t - sJ[0][lane] + (cr[0] * sJ[0][0] + cr[1] * sJ[0][1] + cr[2] * sJ[0][2]);
    } else if (trans) {
      t = trans[(size_t)s * 3 + lane];
    }
    sT[lane] = t;
    ws_trans(ws, B, s)[lane] = t;
  }
  __syncthreads();

  // the kinematic chain (smpl_layer.py:102-120): entry (r, c) of the 3 x 4 transform per lane, joints in order (parent < child)
  const int r = (lane >> 2) % 3, c = lane & 3;
  if (lane < 12) sG[0][lane] = c < 3 ? sR[0][3 * r + c] : sJ[0][r];
  __syncthreads();
  for (int i = 1; i < SMPL_J; ++i) {
    const int p = par.p[i];
    if (lane < 12) {
      const float* g = sG[p] + 4 * r;
      float v;
      if (c < 3) {
        v = g[0] * sR[i][c] + g[1] * sR[i][3 + c] + g[2] * sR[i][6 + c];
      } else {
        v = g[0] * (sJ[i][0] - sJ[p][0]) + g[1] * (sJ[i][1] - sJ[p][1]) + g[2] * (sJ[i][2] - sJ[p][2]) + g[3];
      }
      sG[i][lane] = v;
    }
    __syncthreads();
  }
  // A_i = G_i - pack(G_i [J_i; 0]) (:126-132), and the posed joints with the output transform
  float* A = ws_A(ws, s);
  for (int i = lane; i < SMPL_A; i += 64) {
    const int j = i / 12, e = i % 12, rr = e >> 2, cc = e & 3;
    const float* g = sG[j] + 4 * rr;
    A[i] = cc < 3 ? g[cc] : g[3] - (g[0] * sJ[j][0] + g[1] * sJ[j][1] + g[2] * sJ[j][2]);
  }
  for (int i = lane; i < SMPL_J * 3; i += 64) {
    const int j = i / 3, rr = i % 3;
    const float o = offset ? offset[(size_t)s * 3 + rr] : 0.f;
    joints_out[(size_t)s * 72 + i] = (sG[j][4 * rr + 3] + sT[rr]) * scale - o;
  }
}

__global__ __launch_bounds__(64) void smpl_pose_kernel(const float* __restrict__ pose, const float* __restrict__ betas,
                                                       const float* __restrict__ trans, const float* __restrict__ cam_R,
                                                       const float* __restrict__ cam_t, const float* __restrict__ j_template,
                                                       const float* __restrict__ j_shapedirs, SmplParents par,
                                                       const int* __restrict__ sample_index, int B, float scale,
                                                       const float* __restrict__ offset, float* __restrict__ ws,
                                                       float* __restrict__ joints_out) {
  smpl_pose_body<false>(pose, betas, 10, trans, cam_R, cam_t, j_template, j_shapedirs, par, sample_index, B, scale, offset, ws,
                        joints_out);
}

__global__ __launch_bounds__(64) void smpl_pose_rotmat_kernel(const float* __restrict__ rotmats, const float* __restrict__ betas,
                                                              int betas_stride, const float* __restrict__ trans,
                                                              const float* __restrict__ j_template,
                                                              const float* __restrict__ j_shapedirs, SmplParents par,
                                                              const int* __restrict__ sample_index, int B, float scale,
                                                              const float* __restrict__ offset, float* __restrict__ ws,
                                                              float* __restrict__ joints_out) {
  smpl_pose_body<true>(rotmats, betas, betas_stride, trans, nullptr, nullptr, j_template, j_shapedirs, par, sample_index, B, scale,
                       offset, ws, joints_out);
}

__global__ __launch_bounds__(SMPL_VT, 4) void smpl_skin_kernel(const float* __restrict__ vt, const float* __restrict__ dirs,
                                                            const float* __restrict__ wts, const float* __restrict__ ws_,
                                                            const int* __restrict__ sample_index, int n, int B, int V, float scale,
                                                            const float* __restrict__ offset, float* __restrict__ verts_out) {
  __shared__ __attribute__((aligned(16))) float sC[SMPL_KP][SMPL_CLD];
  __shared__ __attribute__((aligned(16))) float sA[SMPL_TB][SMPL_A];
  __shared__ float sT[SMPL_TB][3];
  __shared__ float sO[SMPL_TB][3];
  __shared__ int sS[SMPL_TB];
  float* ws = const_cast<float*>(ws_);
  const int tid = threadIdx.x;
  if (tid < SMPL_TB) {
    const int g = blockIdx.y * SMPL_TB + tid;
    int s = -1;
    if (g < n) s = sample_index ? sample_index[g] : g;
    if ((unsigned)s >= (unsigned)B) s = -1;
    sS[tid] = s;
  }
  __syncthreads();
  // (k runs fastest: neighbouring lanes read neighbouring floats of one sample's coefficient row and transpose on the way into LDS)
  for (int i = tid; i < SMPL_KP * SMPL_TB; i += SMPL_VT) {
    const int k = i % SMPL_KP, t = i / SMPL_KP;
    const int s = sS[t];
    sC[k][t] = (s >= 0 && k < SMPL_K) ? ws_coef(ws, B, s)[k] : 0.f;
  }
  for (int i = tid; i < SMPL_TB * SMPL_A; i += SMPL_VT) {
    const int t = i / SMPL_A, e = i % SMPL_A;
    const int s = sS[t];
    sA[t][e] = s >= 0 ? ws_A(ws, s)[e] : 0.f;
  }
  if (tid < SMPL_TB * 3) {
    const int t = tid / 3, e = tid % 3;
    const int s = sS[t];
    sT[t][e] = s >= 0 ? ws_trans(ws, B, s)[e] : 0.f;
    sO[t][e] = (s >= 0 && offset) ? offset[(size_t)s * 3 + e] : 0.f;
  }
  __syncthreads();

  const int v = blockIdx.x * SMPL_VT + tid;
  const int vc = min(v, V - 1);  // lanes past the last vertex compute on it and store nothing
  float acc[SMPL_TB][3];
  {
    const float x = vt[(unsigned)vc], y = vt[(unsigned)(V + vc)], z = vt[(unsigned)(2 * V + vc)];
#pragma unroll
    for (int t = 0; t < SMPL_TB; ++t) acc[t][0] = x, acc[t][1] = y, acc[t][2] = z;
  }
  // v_posed = v_template + [shapedirs | posedirs] . coefficients: four rows per step, the next four in flight
  float d[12], nd[12];
#pragma unroll
  for (int u = 0; u < 12; ++u) d[u] = dirs[(unsigned)(u * V + vc)];  // (32-bit offsets on a uniform base: 3 V 220 < 2^31, checked on the host)
  for (int k4 = 0; k4 < SMPL_KP / 4; ++k4) {
    const int kn = min(k4 + 1, SMPL_KP / 4 - 1);
#pragma unroll
    for (int u = 0; u < 12; ++u) nd[u] = dirs[(unsigned)((kn * 12 + u) * V + vc)];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4* cf = reinterpret_cast<const f32x4*>(sC[4 * k4 + q]);
#pragma unroll
      for (int t4 = 0; t4 < SMPL_TB / 4; ++t4) {
        const f32x4 c = cf[t4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[4 * t4 + e][0] = fmaf(d[3 * q + 0], c[e], acc[4 * t4 + e][0]);
          acc[4 * t4 + e][1] = fmaf(d[3 * q + 1], c[e], acc[4 * t4 + e][1]);
          acc[4 * t4 + e][2] = fmaf(d[3 * q + 2], c[e], acc[4 * t4 + e][2]);
        }
      }
      // one row's 16 coefficients live at a time: left alone the scheduler hoists all four rows' LDS reads (64 registers) and spills
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < 12; ++u) d[u] = nd[u];
  }
  // skinning, joint by joint, eight samples at a time (24 live sums instead of 48); the next joint's weight is requested a joint ahead
#pragma unroll
  for (int h = 0; h < SMPL_TB; h += SMPL_TB / 2) {
    float out[SMPL_TB / 2][3];
#pragma unroll
    for (int t = 0; t < SMPL_TB / 2; ++t) out[t][0] = out[t][1] = out[t][2] = 0.f;
    float w = wts[(unsigned)vc];
    for (int j = 0; j < SMPL_J; ++j) {
      const float wn = wts[(unsigned)(min(j + 1, SMPL_J - 1) * V + vc)];
      if (__ballot(w != 0.f) != 0ull) {  // wave-uniform
#pragma unroll
        for (int t = 0; t < SMPL_TB / 2; ++t) {
          const f32x4* a = reinterpret_cast<const f32x4*>(&sA[h + t][12 * j]);
          const f32x4 a0 = a[0], a1 = a[1], a2 = a[2];
          const float* p = acc[h + t];
          const float px = fmaf(a0.x, p[0], fmaf(a0.y, p[1], fmaf(a0.z, p[2], a0.w)));
          const float py = fmaf(a1.x, p[0], fmaf(a1.y, p[1], fmaf(a1.z, p[2], a1.w)));
          const float pz = fmaf(a2.x, p[0], fmaf(a2.y, p[1], fmaf(a2.z, p[2], a2.w)));
          out[t][0] = fmaf(w, px, out[t][0]);
          out[t][1] = fmaf(w, py, out[t][1]);
          out[t][2] = fmaf(w, pz, out[t][2]);
        }
      }
      w = wn;
    }
    if (v < V) {
#pragma unroll
      for (int t = 0; t < SMPL_TB / 2; ++t) {
        const int s = sS[h + t];
        if (s >= 0) {  // workgroup-uniform
          float* o = verts_out + ((size_t)s * V + v) * 3;
          o[0] = (out[t][0] + sT[h + t][0]) * scale - sO[h + t][0];
          o[1] = (out[t][1] + sT[h + t][1]) * scale - sO[h + t][1];
          o[2] = (out[t][2] + sT[h + t][2]) * scale - sO[h + t][2];
        }
      }
    }
  }
}

}  // namespace

extern "C" size_t pmce_smpl_workspace_bytes(int B) {
  if (B < 1) {
    pmce_set_error("smpl_workspace_bytes: B must be >= 1 (got %d)", B);
    return 0;
  }
  return (size_t)B * SMPL_WS_FLOATS * sizeof(float);
}

namespace {

// The checks and the two launches that both entry points share; `rot`: pose holds rotation matrices [B][24][9] instead of axis-angle.
int smpl_forward_impl(const char* what, const float* v_template_t, const float* dirs_t, const float* weights_t, const float* j_template,
                      const float* j_shapedirs, const int* parents_host, int n_joints, const float* pose, bool rot,
                      const float* betas, int betas_stride, const float* trans, const float* cam_R, const float* cam_t,
                      const int* sample_index, int n, float scale, const float* offset, float* verts_out, float* joints_out,
                      void* workspace, size_t workspace_bytes, int B, int V, hipStream_t stream) {
  PMCE_REQUIRE(V >= 1, "%s: V must be >= 1 (got %d)", what, V);
  PMCE_REQUIRE(B >= 1, "%s: B must be >= 1 (got %d)", what, B);
  PMCE_REQUIRE(n_joints == SMPL_J, "%s: the kinematic tree must have %d joints (got %d)", what, SMPL_J, n_joints);
  PMCE_REQUIRE(parents_host, "%s: null parents", what);
  SmplParents par;
  par.p[0] = 0;  // (the root's entry is not read: SMPL files hold 2^32 - 1 there)
  for (int i = 1; i < SMPL_J; ++i) {
    PMCE_REQUIRE(parents_host[i] >= 0 && parents_host[i] < i, "%s: the parent of joint %d must be in [0, %d) (got %d)", what, i, i,
                 parents_host[i]);
    par.p[i] = parents_host[i];
  }
  PMCE_REQUIRE(v_template_t && dirs_t && weights_t && j_template && j_shapedirs, "%s: null model table", what);
  PMCE_REQUIRE(pose && betas && verts_out && joints_out && workspace, "%s: null pointer", what);
  PMCE_REQUIRE(betas_stride >= 10, "%s: betas_stride must be >= 10 (got %d)", what, betas_stride);
  PMCE_REQUIRE((cam_R != nullptr) == (cam_t != nullptr), "%s: cam_R and cam_t go together (both or neither)", what);
  if (sample_index) {
    PMCE_REQUIRE(n >= 1 && n <= B, "%s: with sample_index n must be in 1..B = %d (got %d)", what, B, n);
  } else {
    PMCE_REQUIRE(n == B, "%s: without sample_index n must equal B (got %d, %d)", what, n, B);
  }
  if (workspace_bytes < (size_t)B * SMPL_WS_FLOATS * sizeof(float)) {
    pmce_set_error("%s: workspace of %zu bytes, %zu needed for B = %d", what, workspace_bytes,
                   (size_t)B * SMPL_WS_FLOATS * sizeof(float), B);
    return PMCE_ERR_WORKSPACE;
  }
  PMCE_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  PMCE_REQUIRE((long long)V * 3 * SMPL_KP < (1ll << 31), "%s: V = %d is too large", what, V);
  PMCE_REQUIRE(n <= 65535 * SMPL_TB, "%s: n = %d is more than one launch takes (%d)", what, n, 65535 * SMPL_TB);
  float* ws = static_cast<float*>(workspace);
  if (rot) {
    hipLaunchKernelGGL(smpl_pose_rotmat_kernel, dim3(n), dim3(64), 0, stream, pose, betas, betas_stride, trans, j_template,
                       j_shapedirs, par, sample_index, B, scale, offset, ws, joints_out);
  } else {
    hipLaunchKernelGGL(smpl_pose_kernel, dim3(n), dim3(64), 0, stream, pose, betas, trans, cam_R, cam_t, j_template, j_shapedirs, par,
                       sample_index, B, scale, offset, ws, joints_out);
  }
  PMCE_TRY(pmce_check_launch(rot ? "smpl_forward_rotmat(pose)" : "smpl_forward(pose)"));
  const dim3 grid((V + SMPL_VT - 1) / SMPL_VT, (n + SMPL_TB - 1) / SMPL_TB);
  hipLaunchKernelGGL(smpl_skin_kernel, grid, dim3(SMPL_VT), 0, stream, v_template_t, dirs_t, weights_t, ws, sample_index, n, B, V,
                     scale, offset, verts_out);
  return pmce_check_launch(rot ? "smpl_forward_rotmat(skin)" : "smpl_forward(skin)");
}

}  // namespace

extern "C" int pmce_smpl_forward(const float* v_template_t, const float* dirs_t, const float* weights_t, const float* j_template,
                                 const float* j_shapedirs, const int* parents_host, int n_joints, const float* pose,
                                 const float* betas, const float* trans, const float* cam_R, const float* cam_t,
                                 const int* sample_index, int n, float scale, const float* offset, float* verts_out,
                                 float* joints_out, void* workspace, size_t workspace_bytes, int B, int V, hipStream_t stream) {
  return smpl_forward_impl("smpl_forward", v_template_t, dirs_t, weights_t, j_template, j_shapedirs, parents_host, n_joints, pose,
                           false, betas, 10, trans, cam_R, cam_t, sample_index, n, scale, offset, verts_out, joints_out, workspace,
                           workspace_bytes, B, V, stream);
}

extern "C" int pmce_smpl_forward_rotmat(const float* v_template_t, const float* dirs_t, const float* weights_t, const float* j_template,
                                        const float* j_shapedirs, const int* parents_host, int n_joints, const float* rotmats,
                                        const float* betas, int betas_stride, const float* trans, const int* sample_index, int n,
                                        float scale, const float* offset, float* verts_out, float* joints_out, void* workspace,
                                        size_t workspace_bytes, int B, int V, hipStream_t stream) {
  return smpl_forward_impl("smpl_forward_rotmat", v_template_t, dirs_t, weights_t, j_template, j_shapedirs, parents_host, n_joints,
                           rotmats, true, betas, betas_stride, trans, nullptr, nullptr, sample_index, n, scale, offset, verts_out,
                           joints_out, workspace, workspace_bytes, B, V, stream);
}
