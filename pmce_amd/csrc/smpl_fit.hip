// SMPL parameters from meshes on device: pose (24 rotations), shape (10 betas) and translation of the SMPL body that is nearest to a
// mesh of SMPL's topology - the inverse of smpl.hip's layer, for the non-parametric meshes the video route hands out.  The reference
// has no such function: the algorithm is this project's, and tests/smpl_fit_ref.py restates it in numpy.
//
// With the GLOBAL rotations G_0 = R_0, G_j = G_parent(j) R_j the layer is linear in the rotations:
//     x = T + S beta + P vec(R_1..23 - I),  J = J_T + J_S beta,  b_c = J_c - J_parent(c),  W[c][v] = sum of w[v][k] over the subtree of c
//     v_v = trans + J_0 + sum_j G_j m_vj,      m_vj = w_vj (x_v - J_j) + sum_{c child of j} W_vc b_c
// (the skinning weights of a vertex sum to one).  Given the other rotations the best G_j is an orthogonal Procrustes problem; given all
// rotations v is affine in (beta, trans).  One sweep:
//   1. e_v = y_v - v_v at the current state (carried over from the end of the previous sweep).
//   2. for j = 0..23 IN INDEX ORDER (Gauss-Seidel; updating all joints from one residual was tried and diverges), the pose map fixed:
//      r_v = e_v + G_j m_vj,  C = sum_v r_v m_vj^T,  C = U S V^T,  G_j' = U diag(1, 1, det(U V^T)) V^T,  e_v = r_v - G_j' m_vj.
//      sigma_1 == 0, sigma_2 <= 1e-6 sigma_1 or a non-finite C keep G_j and set PMCE_SMPL_FIT_DEGENERATE_JOINT.
//   3. R from the new G, x with the new pose map, e again; then the 13 unknowns (d beta, d trans) of  min sum_v |e_v - M_v d beta - d trans|^2
//      through the normal equations (M_v = J_S0 + sum_j w_vj G_j (S_v - J_Sj) + sum_{c >= 1} W_vc G_parent(c) (J_Sc - J_Sparent(c))),
//      Cholesky; a pivot <= 0 or non-finite keeps (beta, trans) and sets PMCE_SMPL_FIT_SINGULAR_SHAPE.  Without fit_shape: trans += mean e.
//   4. e at the new state; residual = mean_v |e_v| - the distance of the layer at the returned parameters, the pose map being current.
//
// One workgroup of 1024 lanes per sample; lane t owns the vertices t, t + 1024, ... in every pass, so e (LDS, [3][V]) and x (the
// per-sample workspace, [3][V]) are only ever read by the lane that wrote them.  Per-vertex arithmetic is fp32.  The nine sums of C, the
// 98 sums of the normal equations and the means are fp64: each lane adds its vertices in order, a wave its lanes by a butterfly, lane k
// the sixteen waves in order - no atomics, and the same bits whatever the batch, the other rows or the launch.  The SVD (rotation.hpp)
// and the factorisation run in fp64 on lane 0.  The normal equations are gathered in four passes over the vertices, a few rows of the
// matrix each: 98 fp64 sums do not fit the 128 registers a lane of a 1024-lane workgroup has.  The blend directions are read once per
// sample and sweep (18 MB at V = 6890, shared between the workgroups in flight through L2): with one workgroup per sample there is no
// batch tile to amortise them over, as smpl.hip's skinning kernel has.
#include "common.hpp"
#include "rotation.hpp"

#define PMCE_SMPL_FIT_DEGENERATE_JOINT 1
#define PMCE_SMPL_FIT_SINGULAR_SHAPE 2
#define PMCE_SMPL_FIT_NONFINITE 4

namespace {

constexpr int FIT_J = 24;
constexpr int FIT_NT = 1024;
constexpr int FIT_NW = FIT_NT / 64;
constexpr int FIT_K = 217;   // 10 shape + 207 pose-map coefficients
constexpr int FIT_NS = 98;   // sums of the normal equations: rows i = 0..9 of (14 - i) entries, then the three sums of e
constexpr int FIT_RED = 40;  // most sums one block_sum takes

struct FitTree {
  int parent[FIT_J];
  int off[FIT_J + 1];  // children of j: list[off[j] .. off[j + 1])
  int list[FIT_J];
};

// the small tables of a sample, in LDS in front of e
struct FitShared {
  double red[FIT_NW * FIT_RED];
  double sums[FIT_NS + 6];
  double sol[16];
  float G[FIT_J][9];    // global rotations (the state)
  float R[FIT_J][9];    // local rotations
  float J[FIT_J][3];    // rest joints
  float b[FIT_J][3];    // J_c - J_parent(c); zero for the root
  float gb[FIT_J][3];   // G_parent(c) b_c
  float coef[220];      // betas, pose map
  float Q[FIT_J][30];   // G_j J_Sj
  float E[FIT_J][30];   // G_parent(c) (J_Sc - J_Sparent(c)); zero for the root
  float trans[4];
  int parent[FIT_J];    // the tree (FitTree), where a lane may index it by a number of its own
  int off[FIT_J + 1];
  int list[FIT_J];
  int status;
  int pad[2];
};
static_assert(sizeof(FitShared) % 16 == 0, "e starts 16-byte aligned");
constexpr int FIT_LDS_TOTAL = 163840;
constexpr int FIT_MAX_V = (FIT_LDS_TOTAL - (int)sizeof(FitShared)) / 12;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out[k] = sum over the workgroup of a[k], k < N: lanes of a wave by a butterfly, the waves in index order.  Every lane calls it.
template <int N>
__device__ __forceinline__ void block_sum(double (&a)[N], FitShared& sh, double* out) {
  static_assert(N <= FIT_RED, "block_sum: more sums than the staging rows hold");
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double s = wave_sum_f64(a[k]);
    if ((tid & 63) == 0) sh.red[(tid >> 6) * FIT_RED + k] = s;
  }
  __syncthreads();
  if (tid < N) {
    double s = 0.0;
    for (int w = 0; w < FIT_NW; ++w) s += sh.red[w * FIT_RED + tid];
    out[tid] = s;
  }
  __syncthreads();
}

// R from G, the pose map and the betas into coef - after this and a barrier `blend` may run.  Every lane calls it; G is complete.
__device__ __forceinline__ void pose_tables(FitShared& sh) {
  const int tid = threadIdx.x;
  if (tid < FIT_J * 9) {
    const int j = tid / 9, r = (tid % 9) / 3, c = tid % 3;
    float v;
    if (j == 0) {
      v = sh.G[0][3 * r + c];
    } else {
      const float* gp = sh.G[sh.parent[j]];
      const float* g = sh.G[j];
      v = fmaf(gp[r], g[c], fmaf(gp[3 + r], g[3 + c], gp[6 + r] * g[6 + c]));  // (G_p^T G_j)[r][c]
    }
    sh.R[j][3 * r + c] = v;
    if (j > 0) sh.coef[10 + 9 * (j - 1) + 3 * r + c] = v - (r == c ? 1.0f : 0.0f);
  }
}

// J, b, G_parent b from the betas in coef.  Every lane calls it; barriers inside, and one before the tables are read is the caller's.
__device__ __forceinline__ void joint_tables(FitShared& sh, const float* __restrict__ j_template,
                                             const float* __restrict__ j_shapedirs) {
  const int tid = threadIdx.x;
  if (tid < FIT_J * 3) {
    float j = j_template[tid];
#pragma unroll
    for (int k = 0; k < 10; ++k) j = fmaf(j_shapedirs[tid * 10 + k], sh.coef[k], j);
    sh.J[tid / 3][tid % 3] = j;
  }
  __syncthreads();
  if (tid < FIT_J * 3) {
    const int c = tid / 3, r = tid % 3;
    sh.b[c][r] = c ? sh.J[c][r] - sh.J[sh.parent[c]][r] : 0.0f;
  }
  __syncthreads();
  if (tid < FIT_J * 3) {
    const int c = tid / 3, r = tid % 3;
    const float* g = sh.G[c ? sh.parent[c] : 0] + 3 * r;
    sh.gb[c][r] = fmaf(g[0], sh.b[c][0], fmaf(g[1], sh.b[c][1], g[2] * sh.b[c][2]));
  }
}

// x = T + [S | P] coef for the lane's vertices, into the sample's workspace rows
__device__ __forceinline__ void blend(const FitShared& sh, const float* __restrict__ vt, const float* __restrict__ dirs, int V,
                                      float* __restrict__ x) {
  for (int v = threadIdx.x; v < V; v += FIT_NT) {
    float a0 = vt[(unsigned)v], a1 = vt[(unsigned)(V + v)], a2 = vt[(unsigned)(2 * V + v)];
#pragma unroll 4
    for (int k = 0; k < FIT_K; ++k) {
      const float c = sh.coef[k];
      a0 = fmaf(dirs[(unsigned)((3 * k + 0) * V + v)], c, a0);  // (32-bit offsets: 3 V 220 < 2^31, checked on the host)
      a1 = fmaf(dirs[(unsigned)((3 * k + 1) * V + v)], c, a1);
      a2 = fmaf(dirs[(unsigned)((3 * k + 2) * V + v)], c, a2);
    }
    x[v] = a0, x[V + v] = a1, x[2 * V + v] = a2;
  }
}

// e_v = y_v - (trans + J_0 + sum_j w_vj G_j (x_v - J_j) + sum_{c >= 1} W_vc G_parent(c) b_c) for the lane's vertices
__device__ __forceinline__ void residual_pass(const FitShared& sh, const float* __restrict__ wts, const float* __restrict__ sub,
                                              const float* __restrict__ y, const float* __restrict__ x, int V, float* __restrict__ e) {
  for (int v = threadIdx.x; v < V; v += FIT_NT) {
    const float x0 = x[v], x1 = x[V + v], x2 = x[2 * V + v];
    float a0 = sh.trans[0] + sh.J[0][0], a1 = sh.trans[1] + sh.J[0][1], a2 = sh.trans[2] + sh.J[0][2];
    for (int j = 0; j < FIT_J; ++j) {
      const float W = sub[(unsigned)(j * V + v)];
      if (W == 0.0f) continue;  // (the subtree weight bounds the joint's own weight: nothing of j reaches this vertex)
      const float w = wts[(unsigned)(j * V + v)];
      const float* g = sh.G[j];
      const float d0 = x0 - sh.J[j][0], d1 = x1 - sh.J[j][1], d2 = x2 - sh.J[j][2];
      a0 = fmaf(w, fmaf(g[0], d0, fmaf(g[1], d1, g[2] * d2)), a0);
      a1 = fmaf(w, fmaf(g[3], d0, fmaf(g[4], d1, g[5] * d2)), a1);
      a2 = fmaf(w, fmaf(g[6], d0, fmaf(g[7], d1, g[8] * d2)), a2);
      if (j) a0 = fmaf(W, sh.gb[j][0], a0), a1 = fmaf(W, sh.gb[j][1], a1), a2 = fmaf(W, sh.gb[j][2], a2);
    }
    e[v] = y[3 * (size_t)v + 0] - a0, e[V + v] = y[3 * (size_t)v + 1] - a1, e[2 * V + v] = y[3 * (size_t)v + 2] - a2;
  }
}

// m_vj = w_vj (x_v - J_j) + sum_{c child of j} W_vc b_c
__device__ __forceinline__ void joint_term(const FitShared& sh, const float* __restrict__ wts,
                                           const float* __restrict__ sub, int j, int v, int V, float x0, float x1, float x2, float* m) {
  const float w = wts[(unsigned)(j * V + v)];
  m[0] = w * (x0 - sh.J[j][0]), m[1] = w * (x1 - sh.J[j][1]), m[2] = w * (x2 - sh.J[j][2]);
  for (int q = sh.off[j]; q < sh.off[j + 1]; ++q) {
    const int c = sh.list[q];
    const float W = sub[(unsigned)(c * V + v)];
    m[0] = fmaf(W, sh.b[c][0], m[0]), m[1] = fmaf(W, sh.b[c][1], m[1]), m[2] = fmaf(W, sh.b[c][2], m[2]);
  }
}

// Lane 0: the rotation nearest to C = sums[0..9) (row-major) into G_j, or the degenerate rule.  U and V are completed as right-handed
// frames (third column = cross product of the first two), which is U diag(1, 1, det(U V^T)) V^T without a determinant.
__device__ void procrustes_step(FitShared& sh, int j) {
  double A[3][3], Vm[3][3], nrm[3];
  bool finite = true;
  for (int i = 0; i < 9; ++i) {
    A[i / 3][i % 3] = sh.sums[i];
    finite = finite && isfinite(sh.sums[i]);
  }
  if (finite) jacobi_svd3(A, Vm);
  for (int c = 0; c < 3; ++c) nrm[c] = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c];
  int ord[3] = {0, 1, 2};  // descending singular values
  for (int i = 0; i < 2; ++i)
    for (int k = i + 1; k < 3; ++k)
      if (nrm[ord[k]] > nrm[ord[i]]) {
        const int t = ord[i];
        ord[i] = ord[k];
        ord[k] = t;
      }
  const double s1 = sqrt(nrm[ord[0]]), s2 = sqrt(nrm[ord[1]]);
  if (!finite || !(s1 > 0.0) || !(s2 > 1e-6 * s1)) {
    sh.status |= PMCE_SMPL_FIT_DEGENERATE_JOINT;
    return;
  }
  double u[3][3], v[3][3];
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 3; ++i) {
      u[c][i] = A[i][ord[c]];
      v[c][i] = Vm[i][ord[c]];
    }
  normalise3(u[0], 0.0);
  const double d01 = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
  for (int i = 0; i < 3; ++i) u[1][i] -= d01 * u[0][i];
  normalise3(u[1], 0.0);
  cross3(u[0], u[1], u[2]);
  cross3(v[0], v[1], v[2]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sh.G[j][3 * r + c] = (float)(u[0][r] * v[0][c] + u[1][r] * v[1][c] + u[2][r] * v[2][c]);
}

// The shape Jacobian of one vertex: M[r][k], r < 3, k < 10.
__device__ __forceinline__ void shape_jacobian(const FitShared& sh, const float* __restrict__ dirs, const float* __restrict__ wts,
                                               const float* __restrict__ sub, const float* __restrict__ j_shapedirs, int v, int V,
                                               float (&M)[3][10]) {
  float gb[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) gb[i] = 0.0f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 10; ++k) M[r][k] = j_shapedirs[r * 10 + k];  // J_S0
  for (int j = 0; j < FIT_J; ++j) {
    const float W = sub[(unsigned)(j * V + v)];
    if (W == 0.0f) continue;
    const float w = wts[(unsigned)(j * V + v)];
#pragma unroll
    for (int i = 0; i < 9; ++i) gb[i] = fmaf(w, sh.G[j][i], gb[i]);
#pragma unroll
    for (int i = 0; i < 30; ++i) M[i / 10][i % 10] = fmaf(-w, sh.Q[j][i], M[i / 10][i % 10]);
    if (j) {
#pragma unroll
      for (int i = 0; i < 30; ++i) M[i / 10][i % 10] = fmaf(W, sh.E[j][i], M[i / 10][i % 10]);
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const float s0 = dirs[(unsigned)((3 * k + 0) * V + v)], s1 = dirs[(unsigned)((3 * k + 1) * V + v)],
                s2 = dirs[(unsigned)((3 * k + 2) * V + v)];
#pragma unroll
    for (int r = 0; r < 3; ++r) M[r][k] += fmaf(gb[3 * r], s0, fmaf(gb[3 * r + 1], s1, gb[3 * r + 2] * s2));
  }
}

constexpr int ne_row_offset(int i) { return 14 * i - i * (i - 1) / 2; }

// Rows I0..I1-1 of the normal equations into sums[]: row i holds N[i][i..9], then sum_v M_v[r][i] for r = 0..2 (N[i][10 + r]), then the
// right-hand side sum_v M_v[:, i] . e_v.  The pass that takes row 9 also takes the three sums of e (the right-hand side of d trans).
template <int I0, int I1>
__device__ __forceinline__ void normal_rows(FitShared& sh, const float* __restrict__ dirs, const float* __restrict__ wts,
                                            const float* __restrict__ sub, const float* __restrict__ j_shapedirs, int V,
                                            const float* __restrict__ e) {
  constexpr int N = ne_row_offset(I1) - ne_row_offset(I0) + (I1 == 10 ? 3 : 0);
  double a[N];
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = 0.0;
  for (int v = threadIdx.x; v < V; v += FIT_NT) {
    float M[3][10];
    shape_jacobian(sh, dirs, wts, sub, j_shapedirs, v, V, M);
    const double e0 = e[v], e1 = e[V + v], e2 = e[2 * V + v];
    int k = 0;
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      const double m0 = M[0][i], m1 = M[1][i], m2 = M[2][i];
#pragma unroll
      for (int c = i; c < 10; ++c) a[k++] += m0 * (double)M[0][c] + m1 * (double)M[1][c] + m2 * (double)M[2][c];
      a[k++] += m0;
      a[k++] += m1;
      a[k++] += m2;
      a[k++] += m0 * e0 + m1 * e1 + m2 * e2;
    }
    if (I1 == 10) {
      a[k++] += e0;
      a[k++] += e1;
      a[k++] += e2;
    }
  }
  block_sum<N>(a, sh, sh.sums + ne_row_offset(I0));
}

// Lane 0: the 13 x 13 system from sums[] by Cholesky -> sol[0..13) = (d beta, d trans), or zeros and the status bit.
__device__ void solve_shape(FitShared& sh, int V) {
  double N[13][13], rhs[13];
  for (int i = 0; i < 13; ++i)
    for (int k = 0; k < 13; ++k) N[i][k] = 0.0;
  for (int i = 0; i < 10; ++i) {
    const double* row = sh.sums + ne_row_offset(i);
    for (int c = i; c < 10; ++c) N[i][c] = N[c][i] = row[c - i];
    for (int r = 0; r < 3; ++r) N[i][10 + r] = N[10 + r][i] = row[10 - i + r];
    rhs[i] = row[13 - i];
  }
  for (int r = 0; r < 3; ++r) {
    N[10 + r][10 + r] = (double)V;
    rhs[10 + r] = sh.sums[ne_row_offset(10) + r];
  }
  bool ok = true;
  for (int i = 0; i < 13 && ok; ++i) {  // N = L L^T, L in the lower triangle
    for (int k = 0; k <= i; ++k) {
      double s = N[i][k];
      for (int q = 0; q < k; ++q) s -= N[i][q] * N[k][q];
      if (k == i) {
        if (!(s > 0.0) || !isfinite(s)) {
          ok = false;
          break;
        }
        N[i][i] = sqrt(s);
      } else {
        N[i][k] = s / N[k][k];
      }
    }
  }
  for (int i = 0; i < 13 && ok; ++i) {  // L z = rhs
    double s = rhs[i];
    for (int q = 0; q < i; ++q) s -= N[i][q] * rhs[q];
    rhs[i] = s / N[i][i];
  }
  for (int i = 12; i >= 0 && ok; --i) {  // L^T d = z
    double s = rhs[i];
    for (int q = i + 1; q < 13; ++q) s -= N[q][i] * rhs[q];
    rhs[i] = s / N[i][i];
  }
  for (int i = 0; i < 13; ++i) ok = ok && isfinite(rhs[i]);
  if (!ok) sh.status |= PMCE_SMPL_FIT_SINGULAR_SHAPE;
  for (int i = 0; i < 13; ++i) sh.sol[i] = ok ? rhs[i] : 0.0;
}

__global__ __launch_bounds__(FIT_NT) void smpl_fit_kernel(const float* __restrict__ vt, const float* __restrict__ dirs,
                                                          const float* __restrict__ wts, const float* __restrict__ sub,
                                                          const float* __restrict__ j_template, const float* __restrict__ j_shapedirs,
                                                          FitTree tr, const float* __restrict__ verts,
                                                          const float* __restrict__ init_rotmats, const float* __restrict__ init_betas,
                                                          const float* __restrict__ init_trans, const int* __restrict__ sample_index,
                                                          int n_sweeps, int fit_shape, float* __restrict__ rotmats,
                                                          float* __restrict__ pose, float* __restrict__ betas, float* __restrict__ trans,
                                                          float* __restrict__ residual, int* __restrict__ status,
                                                          float* __restrict__ history, float* __restrict__ ws, int B, int V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fit_lds[];
  FitShared& sh = *reinterpret_cast<FitShared*>(fit_lds);
  float* e = reinterpret_cast<float*>(fit_lds + sizeof(FitShared));  // [3][V]
  const int s = sample_index ? sample_index[blockIdx.x] : (int)blockIdx.x;
  if ((unsigned)s >= (unsigned)B) return;  // block-uniform: a list entry out of range owns no row
  const int tid = threadIdx.x;
  const float* y = verts + (size_t)s * V * 3;
  float* x = ws + (size_t)s * V * 3;

  // the means of y and of the template (the cold start's translation), and whether every coordinate of y is finite
  {
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int v = tid; v < V; v += FIT_NT) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float yc = y[3 * (size_t)v + c];
        bad |= !isfinite(yc);
        a[c] += (double)yc;
        a[3 + c] += (double)vt[(unsigned)(c * V + v)];
      }
    }
    if (tid == 0) sh.status = 0;
    __syncthreads();
    if (bad) sh.status = PMCE_SMPL_FIT_NONFINITE;  // (every writer writes the same word)
    __syncthreads();
    if (sh.status) {  // block-uniform: the cold start, an infinite residual, the bit
      if (tid < FIT_J * 9) rotmats[(size_t)s * (FIT_J * 9) + tid] = (tid % 9) % 4 == 0 ? 1.0f : 0.0f;
      if (tid < FIT_J * 3) pose[(size_t)s * (FIT_J * 3) + tid] = 0.0f;
      if (tid < 10) betas[(size_t)s * 10 + tid] = 0.0f;
      if (tid < 3) trans[(size_t)s * 3 + tid] = 0.0f;
      if (history)
        for (int i = tid; i < n_sweeps; i += FIT_NT) history[(size_t)s * n_sweeps + i] = INFINITY;
      if (tid == 0) residual[s] = INFINITY, status[s] = PMCE_SMPL_FIT_NONFINITE;
      return;
    }
    block_sum<6>(a, sh, sh.sums);
  }
  // the state: the caller's, or the cold start (I, 0, mean y - mean T)
  if (tid < FIT_J * 9) sh.R[tid / 9][tid % 9] = init_rotmats ? init_rotmats[(size_t)s * (FIT_J * 9) + tid] : ((tid % 9) % 4 == 0 ? 1.0f : 0.0f);
  if (tid < 220) sh.coef[tid] = (tid < 10 && init_betas) ? init_betas[(size_t)s * 10 + tid] : 0.0f;
  if (tid < 3) sh.trans[tid] = init_trans ? init_trans[(size_t)s * 3 + tid] : (float)(sh.sums[tid] / V - sh.sums[3 + tid] / V);
  if (tid == 0) sh.status = 0;
#pragma unroll
  for (int i = 0; i < FIT_J; ++i)  // (uniform indices: the argument stays in scalar registers)
    if (tid == i) sh.parent[i] = tr.parent[i], sh.off[i] = tr.off[i], sh.list[i] = tr.list[i];
  if (tid == FIT_J) sh.off[FIT_J] = tr.off[FIT_J];
  __syncthreads();
  if (tid < 9) sh.G[0][tid] = sh.R[0][tid];
  __syncthreads();
  for (int j = 1; j < FIT_J; ++j) {  // G_j = G_parent(j) R_j, joints in order (parent < child)
    if (tid < 9) {
      const int r = tid / 3, c = tid % 3;
      const float* gp = sh.G[sh.parent[j]] + 3 * r;
      sh.G[j][tid] = fmaf(gp[0], sh.R[j][c], fmaf(gp[1], sh.R[j][3 + c], gp[2] * sh.R[j][6 + c]));
    }
    __syncthreads();
  }
  pose_tables(sh);
  joint_tables(sh, j_template, j_shapedirs);
  __syncthreads();
  blend(sh, vt, dirs, V, x);
  residual_pass(sh, wts, sub, y, x, V, e);

  for (int sweep = 0; sweep < n_sweeps; ++sweep) {
    // 2: the joints in index order.  Round j takes the previous joint's new rotation out of e and puts this joint's old one in.
    for (int j = 0; j <= FIT_J; ++j) {
      double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int v = tid; v < V; v += FIT_NT) {
        const float x0 = x[v], x1 = x[V + v], x2 = x[2 * V + v];
        float r0 = e[v], r1 = e[V + v], r2 = e[2 * V + v], m[3];
        if (j > 0) {
          joint_term(sh, wts, sub, j - 1, v, V, x0, x1, x2, m);
          const float* g = sh.G[j - 1];
          r0 -= fmaf(g[0], m[0], fmaf(g[1], m[1], g[2] * m[2]));
          r1 -= fmaf(g[3], m[0], fmaf(g[4], m[1], g[5] * m[2]));
          r2 -= fmaf(g[6], m[0], fmaf(g[7], m[1], g[8] * m[2]));
        }
        if (j < FIT_J) {
          joint_term(sh, wts, sub, j, v, V, x0, x1, x2, m);
          const float* g = sh.G[j];
          r0 += fmaf(g[0], m[0], fmaf(g[1], m[1], g[2] * m[2]));
          r1 += fmaf(g[3], m[0], fmaf(g[4], m[1], g[5] * m[2]));
          r2 += fmaf(g[6], m[0], fmaf(g[7], m[1], g[8] * m[2]));
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            a[c] += (double)r0 * (double)m[c];
            a[3 + c] += (double)r1 * (double)m[c];
            a[6 + c] += (double)r2 * (double)m[c];
          }
        }
        e[v] = r0, e[V + v] = r1, e[2 * V + v] = r2;
      }
      if (j == FIT_J) break;
      block_sum<9>(a, sh, sh.sums);
      if (tid == 0) procrustes_step(sh, j);
      __syncthreads();
    }
    // 3: the pose map of the new rotations, the residual with it, then (beta, trans)
    __syncthreads();
    pose_tables(sh);
    joint_tables(sh, j_template, j_shapedirs);  // (the joints have not moved; G_parent b has)
    __syncthreads();
    blend(sh, vt, dirs, V, x);
    residual_pass(sh, wts, sub, y, x, V, e);
    if (fit_shape) {
      for (int i = tid; i < FIT_J * 30; i += FIT_NT) {
        const int j = i / 30, r = (i % 30) / 10, k = i % 10;
        const float* js = j_shapedirs + j * 30;
        const float* g = sh.G[j] + 3 * r;
        sh.Q[j][10 * r + k] = fmaf(g[0], js[k], fmaf(g[1], js[10 + k], g[2] * js[20 + k]));
        float ev = 0.0f;
        if (j) {
          const float* jp = j_shapedirs + sh.parent[j] * 30;
          const float* gp = sh.G[sh.parent[j]] + 3 * r;
          ev = fmaf(gp[0], js[k] - jp[k], fmaf(gp[1], js[10 + k] - jp[10 + k], gp[2] * (js[20 + k] - jp[20 + k])));
        }
        sh.E[j][10 * r + k] = ev;
      }
      __syncthreads();
      normal_rows<0, 2>(sh, dirs, wts, sub, j_shapedirs, V, e);
      normal_rows<2, 4>(sh, dirs, wts, sub, j_shapedirs, V, e);
      normal_rows<4, 7>(sh, dirs, wts, sub, j_shapedirs, V, e);
      normal_rows<7, 10>(sh, dirs, wts, sub, j_shapedirs, V, e);
      if (tid == 0) solve_shape(sh, V);
    } else {
      double a[3] = {0.0, 0.0, 0.0};
      for (int v = tid; v < V; v += FIT_NT) a[0] += (double)e[v], a[1] += (double)e[V + v], a[2] += (double)e[2 * V + v];
      block_sum<3>(a, sh, sh.sums);
      if (tid < 13) sh.sol[tid] = tid < 10 ? 0.0 : sh.sums[tid - 10] / V;
    }
    __syncthreads();
    float db = 0.0f;
    if (tid < 10 && fit_shape) {
      const float old = sh.coef[tid];
      const float nw = (float)((double)old + sh.sol[tid]);
      db = nw - old;
      sh.coef[tid] = nw;
    } else if (tid >= 10 && tid < 13) {
      sh.trans[tid - 10] = (float)((double)sh.trans[tid - 10] + sh.sol[tid]);
    }
    __syncthreads();
    // 4: the state has moved along the shape directions only - x follows, then e and its mean length
    if (fit_shape) {
      if (tid < 10) sh.sol[tid] = (double)db;  // (what the betas moved by in fp32)
      joint_tables(sh, j_template, j_shapedirs);
      __syncthreads();
      for (int v = tid; v < V; v += FIT_NT) {
        float a0 = x[v], a1 = x[V + v], a2 = x[2 * V + v];
#pragma unroll
        for (int k = 0; k < 10; ++k) {
          const float c = (float)sh.sol[k];
          a0 = fmaf(dirs[(unsigned)((3 * k + 0) * V + v)], c, a0);
          a1 = fmaf(dirs[(unsigned)((3 * k + 1) * V + v)], c, a1);
          a2 = fmaf(dirs[(unsigned)((3 * k + 2) * V + v)], c, a2);
        }
        x[v] = a0, x[V + v] = a1, x[2 * V + v] = a2;
      }
    }
    residual_pass(sh, wts, sub, y, x, V, e);
    {
      double a[1] = {0.0};
      for (int v = tid; v < V; v += FIT_NT) {
        const float e0 = e[v], e1 = e[V + v], e2 = e[2 * V + v];
        a[0] += (double)sqrtf(fmaf(e0, e0, fmaf(e1, e1, e2 * e2)));
      }
      block_sum<1>(a, sh, sh.sums);
      if (tid == 0) {
        const float res = (float)(sh.sums[0] / V);
        if (history) history[(size_t)s * n_sweeps + sweep] = res;
        if (sweep == n_sweeps - 1) residual[s] = res;
      }
    }
  }
  // the results: local rotations (R is current: step 3 of the last sweep), their axis-angle form, betas, trans, status
  if (tid < FIT_J * 9) rotmats[(size_t)s * (FIT_J * 9) + tid] = sh.R[tid / 9][tid % 9];
  if (tid < FIT_J) {
    float aa[3];
    rotmat_to_angle_axis(sh.R[tid], aa);
    float* p = pose + (size_t)s * (FIT_J * 3) + 3 * tid;
    p[0] = aa[0], p[1] = aa[1], p[2] = aa[2];
  }
  if (tid < 10) betas[(size_t)s * 10 + tid] = sh.coef[tid];
  if (tid < 3) trans[(size_t)s * 3 + tid] = sh.trans[tid];
  if (tid == 0) status[s] = sh.status;
}

}  // namespace

extern "C" int pmce_smpl_fit_max_verts(void) { return FIT_MAX_V; }

extern "C" size_t pmce_smpl_fit_workspace_bytes(int B, int V) {
  if (B < 1 || V < 1 || V > FIT_MAX_V) {
    pmce_set_error("smpl_fit_workspace_bytes: B must be >= 1 and V in 1..%d (got %d, %d)", FIT_MAX_V, B, V);
    return 0;
  }
  return (((size_t)B * V * 3 * sizeof(float)) + 15) & ~(size_t)15;
}

extern "C" int pmce_smpl_fit(const float* v_template_t, const float* dirs_t, const float* weights_t, const float* subtree_weights_t,
                             const float* j_template, const float* j_shapedirs, const int* parents_host, int n_joints,
                             const float* verts, const float* init_rotmats, const float* init_betas, const float* init_trans,
                             const int* sample_index, int n, int n_sweeps, int fit_shape, float* rotmats, float* pose, float* betas,
                             float* trans, float* residual, int* status, float* history, void* workspace, size_t workspace_bytes,
                             int B, int V, hipStream_t stream) {
  const char* what = "smpl_fit";
  PMCE_REQUIRE(V >= 1, "%s: V must be >= 1 (got %d)", what, V);
  PMCE_REQUIRE(V <= FIT_MAX_V,
               "%s: V = %d does not fit: the residual of a sample (12 V bytes) is kept in LDS, and %d bytes of it hold at most %d vertices",
               what, V, FIT_LDS_TOTAL, FIT_MAX_V);
  PMCE_REQUIRE(B >= 1, "%s: B must be >= 1 (got %d)", what, B);
  PMCE_REQUIRE(n_sweeps >= 1, "%s: n_sweeps must be >= 1 (got %d)", what, n_sweeps);
  PMCE_REQUIRE(n_joints == FIT_J, "%s: the kinematic tree must have %d joints (got %d)", what, FIT_J, n_joints);
  PMCE_REQUIRE(parents_host, "%s: null parents", what);
  FitTree tr;
  tr.parent[0] = 0;  // (the root's entry is not read: SMPL files hold 2^32 - 1 there)
  for (int i = 1; i < FIT_J; ++i) {
    PMCE_REQUIRE(parents_host[i] >= 0 && parents_host[i] < i, "%s: the parent of joint %d must be in [0, %d) (got %d)", what, i, i,
                 parents_host[i]);
    tr.parent[i] = parents_host[i];
  }
  int fill = 0;
  for (int j = 0; j < FIT_J; ++j) {
    tr.off[j] = fill;
    for (int c = 1; c < FIT_J; ++c)
      if (tr.parent[c] == j) tr.list[fill++] = c;
  }
  tr.off[FIT_J] = fill;
  for (int i = fill; i < FIT_J; ++i) tr.list[i] = 0;
  PMCE_REQUIRE(v_template_t && dirs_t && weights_t && subtree_weights_t && j_template && j_shapedirs, "%s: null model table", what);
  PMCE_REQUIRE(verts && rotmats && pose && betas && trans && residual && status && workspace, "%s: null pointer", what);
  if (sample_index) {
    PMCE_REQUIRE(n >= 1 && n <= B, "%s: with sample_index n must be in 1..B = %d (got %d)", what, B, n);
  } else {
    PMCE_REQUIRE(n == B, "%s: without sample_index n must equal B (got %d, %d)", what, n, B);
  }
  const size_t need = (((size_t)B * V * 3 * sizeof(float)) + 15) & ~(size_t)15;
  if (workspace_bytes < need) {
    pmce_set_error("%s: workspace of %zu bytes, %zu needed for B = %d, V = %d", what, workspace_bytes, need, B, V);
    return PMCE_ERR_WORKSPACE;
  }
  PMCE_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  PMCE_REQUIRE((long long)V * 3 * 220 < (1ll << 31), "%s: V = %d is too large", what, V);
  static std::atomic<unsigned long long> done{0};
  PMCE_TRY(pmce_opt_in_lds(reinterpret_cast<const void*>(&smpl_fit_kernel), FIT_LDS_TOTAL, done, what));
  const size_t lds = sizeof(FitShared) + (size_t)V * 12;
  hipLaunchKernelGGL(smpl_fit_kernel, dim3(n), dim3(FIT_NT), lds, stream, v_template_t, dirs_t, weights_t, subtree_weights_t, j_template,
                     j_shapedirs, tr, verts, init_rotmats, init_betas, init_trans, sample_index, n_sweeps, fit_shape, rotmats, pose,
                     betas, trans, residual, status, history, static_cast<float*>(workspace), B, V);
  return pmce_check_launch(what);
}
