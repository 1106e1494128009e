// ViTPose's network as one call: normalised person patches -> keypoint heatmaps.  The structure is that of ViTPose's published ViT
// backbone (patch embedding with padding 2, no class token, `depth` pre-norm blocks, last_norm) and TopdownHeatmapSimpleHead (two
// ConvTranspose2d(4, 2, 1) + BatchNorm + ReLU, a 1 x 1 convolution), with the hyper-parameters of the demo's config
// (pose_detector/ViTPose_huge_coco_256x192.py).  Host code only: the table of tensors and the launch sequence on the operators of
// gemm_split_f16.hip, conv.hip, vit_attention.hip, layernorm_rows.hip and deconv_gather.hip (the weights' storage: net_weights.hpp).
// Three tensors arrive prepared by the host (pmce_amd/vitpose.py, in fp64 rounded once): the position table pos_embed[1:] + pos_embed[:1],
// and each deconvolution as the weight of its product with the BatchNorm scale folded in, plus the folded BatchNorm bias.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "net_weights.hpp"
#include "../../include/pmce_hip.h"

namespace {

using pmce_net::CONV;
using pmce_net::Kind;
using pmce_net::LINEAR;
using pmce_net::LINEAR_F16;
using pmce_net::PLAIN;

struct Tensor : pmce_net::Param {
  std::string name;
};

constexpr int MAX_N = 256;
constexpr int PATCH = 16, PATCH_PAD = 2;
constexpr float LN_EPS = 1e-6f;

}  // namespace

struct pmce_vitpose {
  int H, W, C, depth, heads, F1, F2, K;
  int Hp, Wp, N;
  int precision;  // 0: every product in the three-product split form; 1: the blocks' products and attention as ONE f16 product (gemm_f16.hip)
  std::vector<Tensor> t;
  pmce_net::Arena arena;

  // floats per image: the token stream, the normalised planes, the attention planes, then max(body, head)
  size_t body_floats() const { return (size_t)N * 3 * C + (size_t)N * 4 * C; }
  size_t head_floats() const { return (size_t)N * 16 * F1 + (size_t)4 * N * F1 + (size_t)4 * N * 16 * F2 + (size_t)16 * N * F2; }
  size_t image_floats() const { return (size_t)3 * N * C + (body_floats() > head_floats() ? body_floats() : head_floats()); }
};

extern "C" int pmce_vitpose_create(int H, int W, int C, int depth, int heads, int F1, int F2, int K, pmce_vitpose** out) {
  return pmce_vitpose_create_precision(H, W, C, depth, heads, F1, F2, K, 0, out);
}

extern "C" int pmce_vitpose_precision(const pmce_vitpose* v) { return v ? v->precision : -1; }

extern "C" int pmce_vitpose_create_precision(int H, int W, int C, int depth, int heads, int F1, int F2, int K, int precision, pmce_vitpose** out) {
  PMCE_REQUIRE(out, "vitpose_create: null pointer");
  PMCE_REQUIRE(precision == 0 || precision == 1, "vitpose_create: precision must be 0 (split_f16) or 1 (f16) (got %d)", precision);
  PMCE_REQUIRE(H >= PATCH && W >= PATCH && H % PATCH == 0 && W % PATCH == 0, "vitpose_create: the image (%d x %d) must be whole 16 x 16 patches", H, W);
  const int Hp = H / PATCH, Wp = W / PATCH, N = Hp * Wp;
  PMCE_REQUIRE(N <= 192, "vitpose_create: the image (%d x %d) has %d tokens, at most 192 are supported", H, W, N);
  PMCE_REQUIRE(C >= 32 && C % 32 == 0 && C <= 2048, "vitpose_create: embed_dim must be a multiple of 32 in 32..2048 (got %d)", C);
  PMCE_REQUIRE(depth >= 1, "vitpose_create: depth must be at least 1 (got %d)", depth);
  PMCE_REQUIRE(heads >= 1 && C % heads == 0 && (C / heads == 64 || C / heads == 80),
               "vitpose_create: embed_dim / num_heads must be 64 or 80 (got embed_dim=%d num_heads=%d)", C, heads);
  PMCE_REQUIRE(F1 >= 32 && F1 % 32 == 0 && F1 <= 2048, "vitpose_create: the first deconvolution's filters must be a multiple of 32 in 32..2048 (got %d)", F1);
  PMCE_REQUIRE(F2 >= 32 && F2 % 32 == 0 && F2 <= 2048, "vitpose_create: the second deconvolution's filters must be a multiple of 32 in 32..2048 (got %d)", F2);
  PMCE_REQUIRE(K >= 1 && K <= 64, "vitpose_create: the number of keypoints must be in 1..64 (got %d)", K);
  pmce_vitpose* v = new pmce_vitpose();
  v->H = H; v->W = W; v->C = C; v->depth = depth; v->heads = heads; v->F1 = F1; v->F2 = F2; v->K = K;
  v->Hp = Hp; v->Wp = Wp; v->N = N;
  v->precision = precision;
  const Kind block_linear = precision == 1 ? LINEAR_F16 : LINEAR;
  auto add = [&](const std::string& name, Kind kind, int rank, int s0, int s1 = 0, int s2 = 0, int s3 = 0) {
    v->t.push_back({pmce_net::Param(kind, rank, s0, s1, s2, s3), name});
  };
  auto lin = [&](const std::string& p, int nout, int nin) {
    add(p + ".weight", block_linear, 2, nout, nin);
    add(p + ".bias", PLAIN, 1, nout);
  };
  auto norm = [&](const std::string& p) {
    add(p + ".weight", PLAIN, 1, C);
    add(p + ".bias", PLAIN, 1, C);
  };
  add("backbone.pos_embed", PLAIN, 2, N, C);  // pos_embed[1:] + pos_embed[:1]
  add("backbone.patch_embed.proj.weight", CONV, 4, C, 3, PATCH, PATCH);
  add("backbone.patch_embed.proj.bias", PLAIN, 1, C);
  for (int i = 0; i < depth; ++i) {
    const std::string p = "backbone.blocks." + std::to_string(i);
    norm(p + ".norm1");
    lin(p + ".attn.qkv", 3 * C, C);
    lin(p + ".attn.proj", C, C);
    norm(p + ".norm2");
    lin(p + ".mlp.fc1", 4 * C, C);
    lin(p + ".mlp.fc2", C, 4 * C);
  }
  norm("backbone.last_norm");
  add("keypoint_head.deconv_layers.0.weight", LINEAR, 2, 16 * F1, C);  // the product form, BatchNorm scale folded
  add("keypoint_head.deconv_layers.1.bias", PLAIN, 1, F1);             // the folded BatchNorm bias
  add("keypoint_head.deconv_layers.3.weight", LINEAR, 2, 16 * F2, F1);
  add("keypoint_head.deconv_layers.4.bias", PLAIN, 1, F2);
  add("keypoint_head.final_layer.weight", LINEAR, 2, K, F2);
  add("keypoint_head.final_layer.bias", PLAIN, 1, K);
  *out = v;
  return PMCE_OK;
}

extern "C" void pmce_vitpose_destroy(pmce_vitpose* v) { delete v; }

extern "C" int pmce_vitpose_tensor_count(const pmce_vitpose* v) { return v ? (int)v->t.size() : 0; }

extern "C" const char* pmce_vitpose_tensor_name(const pmce_vitpose* v, int i) {
  return v && i >= 0 && i < (int)v->t.size() ? v->t[i].name.c_str() : nullptr;
}

extern "C" int pmce_vitpose_tensor_shape(const pmce_vitpose* v, int i, int* shape4) {
  PMCE_REQUIRE(v && shape4 && i >= 0 && i < (int)v->t.size(), "vitpose_tensor_shape: bad arguments");
  for (int d = 0; d < 4; ++d) shape4[d] = v->t[i].shape[d];
  return v->t[i].rank;
}

extern "C" int pmce_vitpose_set_tensor(pmce_vitpose* v, const char* name, const float* dev_ptr) {
  PMCE_REQUIRE(v && name && dev_ptr, "vitpose_set_tensor: null pointer");
  PMCE_REQUIRE(!v->arena.ready(), "vitpose_set_tensor: the network is finalized");
  PMCE_REQUIRE((reinterpret_cast<uintptr_t>(dev_ptr) & 15) == 0, "vitpose_set_tensor: tensor '%s' must be 16-byte aligned", name);
  for (Tensor& x : v->t)
    if (x.name == name) {
      x.src = dev_ptr;
      return PMCE_OK;
    }
  pmce_set_error("vitpose_set_tensor: no tensor named '%s'", name);
  return PMCE_ERR_ARG;
}

extern "C" int pmce_vitpose_finalize_on(pmce_vitpose* v, pmce_stream_t stream) {
  PMCE_REQUIRE(v, "vitpose_finalize: null pointer");
  std::vector<pmce_net::Param*> params;
  for (Tensor& x : v->t) params.push_back(&x);
  auto label = [&](size_t i) { return "tensor '" + v->t[i].name + "'"; };
  return pmce_net::finalize("vitpose_finalize", params, label, v->arena, stream);
}

extern "C" size_t pmce_vitpose_workspace_bytes(const pmce_vitpose* v, int n) {
  if (!v || n < 1 || n > MAX_N) {
    pmce_set_error("vitpose_workspace_bytes: n must be in 1..%d (got %d)", MAX_N, n);
    return 0;
  }
  return (size_t)n * v->image_floats() * sizeof(float);
}

extern "C" int pmce_vitpose_forward(const pmce_vitpose* v, const float* patches, long long sn, long long sc, long long sy, long long sx, int n,
                                    float* heat, float* feat, void* workspace, size_t workspace_bytes, pmce_stream_t stream) {
  PMCE_REQUIRE(v && patches && heat && workspace, "vitpose_forward: null pointer");
  PMCE_REQUIRE(v->arena.ready(), "vitpose_forward: the network is not finalized");
  PMCE_REQUIRE(n >= 1 && n <= MAX_N, "vitpose_forward: n must be in 1..%d (got %d)", MAX_N, n);
  PMCE_TRY(pmce_net::check_workspace("vitpose_forward", workspace, workspace_bytes, pmce_vitpose_workspace_bytes(v, n)));
  const int C = v->C, N = v->N, F1 = v->F1, F2 = v->F2;
  const int M = n * N;
  float* ws = static_cast<float*>(workspace);
  float* X = ws;                         // the token stream, fp32 [M][C]
  float* XN = X + (size_t)M * C;         // LayerNorm results, planes [M][C]
  float* AO = XN + (size_t)M * C;        // attention results, planes [M][C]
  float* rest = AO + (size_t)M * C;
  float* QKV = rest;                     // fp32 [M][3C]
  float* HID = QKV + (size_t)M * 3 * C;  // planes [M][4C]
  float* Y1 = rest;                      // the head reuses the blocks' buffers: fp32 [M][16 F1]
  float* G1 = Y1 + (size_t)M * 16 * F1;  // planes [4M][F1]
  float* Y2 = G1 + (size_t)4 * M * F1;   // fp32 [4M][16 F2]
  float* G2 = Y2 + (size_t)4 * M * 16 * F2;  // planes [16M][F2]

  // the table's order (pmce_vitpose_create): 3 leading tensors, 12 per block, last_norm, the head's 6
  enum { NORM1 = 0, QKV_W = 2, QKV_B, PROJ_W, PROJ_B, NORM2, FC1_W = 8, FC1_B, FC2_W, FC2_B, PER_BLOCK };
  const Tensor* const tab = v->t.data();
  const Tensor* const tail = tab + 3 + PER_BLOCK * v->depth;  // last_norm (2), deconv 0 weight, bias, deconv 3 weight, bias, final weight, bias
  // C[rows][nout] = act(A W^T + bias) (+ R); A pre-split; b = the bias tensor or null
  auto product = [&](const Tensor* w, const Tensor* b, const float* A, const float* R, float* out, int rows, int act, int c_packed) {
    return pmce_gemm_nt_split_f16(A, nullptr, w->dev, 1, w->wscale, b ? b->dev : nullptr, R, out, rows, w->shape[0], w->shape[1], w->shape[1],
                                  w->shape[0], act, 1, c_packed, 0, 0, 0, stream);
  };
  // wb: a LayerNorm's weight, its bias follows
  auto ln = [&](const Tensor* wb, const float* add, float* out1, float* out, int split) {
    return pmce_layernorm_rows_f32(X, M, C, add, N, out1, wb[0].dev, wb[1].dev, LN_EPS, out, split, stream);
  };

  // the patch embedding reads the patches through the caller's strides; its NHWC result is the token matrix
  PMCE_TRY(pmce_conv2d_split_f16(patches, sn, sc, sy, sx, n, 3, v->H, v->W, tab[1].dev, tab[1].wscale, tab[2].dev, nullptr, X, C, PATCH, PATCH, PATCH,
                                 PATCH_PAD, 0, stream));
  // The blocks' steps through the entries of the network's precision.  XN, AO and HID hold the products' operand form: the planes, or in the
  // f16 mode plain f16 rows in (half of) their fp32-sized slots.
  const bool f16 = v->precision == 1;
  auto block_ln = [&](const Tensor* wb, const float* add, float* out1) {  // LayerNorm of X -> XN in operand form
    return f16 ? pmce_layernorm_rows_f16(X, M, C, add, N, out1, wb[0].dev, wb[1].dev, LN_EPS, XN, stream) : ln(wb, add, out1, XN, 1);
  };
  // out[M][nout] = act(A W^T + bias) (+ R); A in operand form; out fp32, or in operand form (out_operand)
  auto block_product = [&](const Tensor* w, const Tensor* b, const float* A, const float* R, float* out, int act, int out_operand) {
    return f16 ? pmce_gemm_nt_f16(A, w->dev, w->wscale, b->dev, R, out, M, w->shape[0], w->shape[1], w->shape[1], w->shape[0], act, out_operand, nullptr,
                                  stream)
               : product(w, b, A, R, out, M, act, out_operand);
  };
  for (int i = 0; i < v->depth; ++i) {
    const Tensor* b = tab + 3 + PER_BLOCK * i;
    // block 0's norm1 also adds the position table and writes the sum back as the residual stream
    PMCE_TRY(i == 0 ? block_ln(b + NORM1, tab[0].dev, X) : block_ln(b + NORM1, nullptr, nullptr));
    PMCE_TRY(block_product(b + QKV_W, b + QKV_B, XN, nullptr, QKV, 0, 0));
    PMCE_TRY(f16 ? pmce_vit_attention_f16(QKV, AO, n, N, C, v->heads, stream) : pmce_vit_attention_split_f16(QKV, AO, n, N, C, v->heads, stream));
    PMCE_TRY(block_product(b + PROJ_W, b + PROJ_B, AO, X, X, 0, 0));
    PMCE_TRY(block_ln(b + NORM2, nullptr, nullptr));
    PMCE_TRY(block_product(b + FC1_W, b + FC1_B, XN, nullptr, HID, 1, 1));
    PMCE_TRY(block_product(b + FC2_W, b + FC2_B, HID, X, X, 0, 0));
  }
  PMCE_TRY(ln(tail, nullptr, nullptr, XN, 1));
  if (feat) {  // the same rows once more, as fp32 NHWC [n][Hp][Wp][C]
    PMCE_TRY(ln(tail, nullptr, nullptr, feat, 0));
  }
  // the head: product, gather, product, gather, product
  PMCE_TRY(product(tail + 2, nullptr, XN, nullptr, Y1, M, 0, 0));
  PMCE_TRY(pmce_deconv4x4s2_gather_f32(Y1, tail[3].dev, G1, n, v->Hp, v->Wp, F1, 1, stream));
  PMCE_TRY(product(tail + 4, nullptr, G1, nullptr, Y2, 4 * M, 0, 0));
  PMCE_TRY(pmce_deconv4x4s2_gather_f32(Y2, tail[5].dev, G2, n, 2 * v->Hp, 2 * v->Wp, F2, 1, stream));
  return product(tail + 6, tail + 7, G2, nullptr, heat, 16 * M, 0, 0);
}
