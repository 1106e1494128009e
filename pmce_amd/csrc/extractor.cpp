// The demo's feature extractor as one call: the backbone of the reference's HMR (lib/models/spin.py:61-143 - stem, max pool, four stages
// of [3, 4, 6, 3] bottlenecks, the 7 x 7 average; 53 convolutions) on the operators of conv.hip.  Host code only: a table of the 53
// convolutions in the order of the forward and the launch sequence (the weights' storage: net_weights.hpp).  Eval-mode BatchNorm arrives
// folded into each convolution's weight and bias (pmce_amd/extractor.py folds on the host in fp64).
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.hpp"
#include "net_weights.hpp"
#include "../../include/pmce_hip.h"

namespace {

using pmce_net::Param;

struct ConvLayer {
  std::string name;
  int cout, cin, k, stride, pad;
  Param w, b;  // the folded OIHW weight and its bias
};

constexpr int STAGE_PLANES[4] = {64, 128, 256, 512}, STAGE_BLOCKS[4] = {3, 4, 6, 3}, STAGE_STRIDE[4] = {1, 2, 2, 2};
constexpr int SIDE = 224;
constexpr size_t FULL = 112 * 112 * 64;  // floats per image of the largest activation (the stem's output; also 56 x 56 x 256)
constexpr size_t HALF = 56 * 56 * 128;   // of the largest inner activation of a bottleneck (layer2.0.conv1)

}  // namespace

struct pmce_extractor {
  std::vector<ConvLayer> convs;
  pmce_net::Arena arena;
  int precision = 0;  // 0: the three-product split (conv.hip's kernel, fp32 maps); 1: one f16 product (conv_f16.hpp, f16 maps)
};

extern "C" int pmce_extractor_create(pmce_extractor** out) { return pmce_extractor_create_precision(0, out); }

extern "C" int pmce_extractor_precision(const pmce_extractor* e) { return e ? e->precision : -1; }

extern "C" int pmce_extractor_create_precision(int precision, pmce_extractor** out) {
  PMCE_REQUIRE(out, "extractor_create: null pointer");
  PMCE_REQUIRE(precision == 0 || precision == 1, "extractor_create: precision must be 0 (split_f16) or 1 (f16) (got %d)", precision);
  pmce_extractor* e = new pmce_extractor();
  e->precision = precision;
  const pmce_net::Kind kind = precision == 1 ? pmce_net::CONV_F16 : pmce_net::CONV;
  auto add = [&](const std::string& name, int cout, int cin, int k, int stride, int pad) {
    e->convs.push_back({name, cout, cin, k, stride, pad, Param(kind, 4, cout, cin, k, k), Param(pmce_net::PLAIN, 1, cout)});
  };
  add("conv1", 64, 3, 7, 2, 3);
  int inplanes = 64;
  for (int s = 0; s < 4; ++s)
    for (int b = 0; b < STAGE_BLOCKS[s]; ++b) {
      const std::string p = "layer" + std::to_string(s + 1) + "." + std::to_string(b);
      const int planes = STAGE_PLANES[s], stride = b == 0 ? STAGE_STRIDE[s] : 1;
      add(p + ".conv1", planes, inplanes, 1, 1, 0);
      add(p + ".conv2", planes, planes, 3, stride, 1);
      add(p + ".conv3", 4 * planes, planes, 1, 1, 0);
      if (b == 0) add(p + ".downsample.0", 4 * planes, inplanes, 1, stride, 0);
      inplanes = 4 * planes;
    }
  *out = e;
  return PMCE_OK;
}

extern "C" void pmce_extractor_destroy(pmce_extractor* e) { delete e; }

extern "C" int pmce_extractor_conv_count(const pmce_extractor* e) { return e ? (int)e->convs.size() : 0; }

extern "C" const char* pmce_extractor_conv_name(const pmce_extractor* e, int i) {
  return e && i >= 0 && i < (int)e->convs.size() ? e->convs[i].name.c_str() : nullptr;
}

extern "C" int pmce_extractor_conv_shape(const pmce_extractor* e, int i, int* shape4) {
  PMCE_REQUIRE(e && shape4 && i >= 0 && i < (int)e->convs.size(), "extractor_conv_shape: bad arguments");
  const ConvLayer& c = e->convs[i];
  shape4[0] = c.cout; shape4[1] = c.cin; shape4[2] = c.k; shape4[3] = c.k;
  return PMCE_OK;
}

extern "C" int pmce_extractor_set_conv(pmce_extractor* e, const char* name, const float* folded_weight, const float* folded_bias) {
  PMCE_REQUIRE(e && name && folded_weight && folded_bias, "extractor_set_conv: null pointer");
  PMCE_REQUIRE(!e->arena.ready(), "extractor_set_conv: the extractor is finalized");
  for (ConvLayer& c : e->convs)
    if (c.name == name) {
      c.w.src = folded_weight;
      c.b.src = folded_bias;
      return PMCE_OK;
    }
  pmce_set_error("extractor_set_conv: no convolution named '%s'", name);
  return PMCE_ERR_ARG;
}

extern "C" int pmce_extractor_finalize_on(pmce_extractor* e, pmce_stream_t stream) {
  PMCE_REQUIRE(e, "extractor_finalize: null pointer");
  std::vector<Param*> params;
  for (ConvLayer& c : e->convs) {
    params.push_back(&c.w);
    params.push_back(&c.b);
  }
  auto label = [&](size_t i) { return "convolution '" + e->convs[i / 2].name + "'"; };
  return pmce_net::finalize("extractor_finalize", params, label, e->arena, stream);
}

extern "C" size_t pmce_extractor_workspace_bytes(int n) {
  if (n < 1 || n > 4096) {
    pmce_set_error("extractor_workspace_bytes: n must be in 1..4096 (got %d)", n);
    return 0;
  }
  return (size_t)n * (3 * FULL + 2 * HALF) * sizeof(float);
}

extern "C" size_t pmce_extractor_workspace_bytes_for(const pmce_extractor* e, int n) {
  if (!e) {
    pmce_set_error("extractor_workspace_bytes_for: null pointer");
    return 0;
  }
  const size_t bytes = pmce_extractor_workspace_bytes(n);  // the same maps, 2 bytes per element in f16 mode
  return e->precision == 1 ? bytes / 2 : bytes;
}

namespace {

// The launch sequence of a forward on workspace maps of T: float (the three-product convolution, fp32 pools, the taps copied) or _Float16
// (the single-product convolution - the stem rounds the fp32 patches in its gather -, f16 pools, the taps widened exactly to fp32).
template <typename T>
int run_layers(const pmce_extractor* e, const float* patches, long long sn, long long sc, long long sy, long long sx, float* feats, int n,
               float* const* taps, void* workspace, hipStream_t stream) {
  constexpr bool F16 = sizeof(T) == 2;
  T* ws = static_cast<T*>(workspace);
  T* full[3] = {ws, ws + (size_t)n * FULL, ws + 2 * (size_t)n * FULL};
  T* t1 = ws + 3 * (size_t)n * FULL;
  T* t2 = t1 + (size_t)n * HALF;
  // the convolution of layer ci on `x` through its four strides (fp32 for the stem, else T); dense NHWC residual and result of T
  auto conv_at = [&](int ci, const void* x, bool x_fp32, long long xn, long long xc, long long xy, long long xx, int h, int w, const T* res, T* out,
                     bool relu) {
    const ConvLayer& c = e->convs[ci];
    if constexpr (F16)
      return pmce_conv2d_act_f16(x, x_fp32 ? 0 : 1, xn, xc, xy, xx, n, c.cin, h, w, c.w.dev, c.w.wscale, c.b.dev, res, c.cout, out, c.cout, 1,
                                 c.cout, c.k, c.k, c.stride, c.pad, relu ? 1 : 0, 0.f, 0, stream);
    else
      return pmce_conv2d_split_f16(static_cast<const float*>(x), xn, xc, xy, xx, n, c.cin, h, w, c.w.dev, c.w.wscale, c.b.dev, res, out, c.cout,
                                   c.k, c.k, c.stride, c.pad, relu ? 1 : 0, stream);
  };
  // NHWC convolution of layer ci on [n][h][w][cin]
  auto conv = [&](int ci, const T* x, int h, int w, const T* res, T* out, bool relu) {
    const int cin = e->convs[ci].cin;
    return conv_at(ci, x, false, (long long)h * w * cin, 1, (long long)w * cin, cin, h, w, res, out, relu);
  };
  PMCE_TRY(conv_at(0, patches, true, sn, sc, sy, sx, SIDE, SIDE, nullptr, full[0], true));  // the stem reads the patches through the caller's strides
  if constexpr (F16) PMCE_TRY(pmce_maxpool3x3s2_nhwc_f16(full[0], full[1], n, 112, 112, 64, stream));
  else PMCE_TRY(pmce_maxpool3x3s2_nhwc_f32(full[0], full[1], n, 112, 112, 64, stream));
  int cur = 1, side = 56, ci = 1;
  for (int s = 0; s < 4; ++s) {
    for (int b = 0; b < STAGE_BLOCKS[s]; ++b) {
      const int stride = b == 0 ? STAGE_STRIDE[s] : 1, oside = side / stride;
      const int a = (cur + 1) % 3, o = (cur + 2) % 3;
      const T* x = full[cur];
      PMCE_TRY(conv(ci, x, side, side, nullptr, t1, true));
      PMCE_TRY(conv(ci + 1, t1, side, side, nullptr, t2, true));
      const T* res = x;
      if (b == 0) {
        PMCE_TRY(conv(ci + 3, x, side, side, nullptr, full[a], false));
        res = full[a];
      }
      PMCE_TRY(conv(ci + 2, t2, oside, oside, res, full[o], true));
      ci += b == 0 ? 4 : 3;
      cur = o;
      side = oside;
    }
    if (taps[s]) {
      const size_t count = (size_t)n * side * side * 4 * STAGE_PLANES[s];
      if constexpr (F16) {
        PMCE_TRY(pmce_widen_f16_f32(full[cur], taps[s], (long long)count, stream));
      } else if (hipMemcpyAsync(taps[s], full[cur], count * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
        pmce_set_error("extractor_forward: copying the output of layer%d failed", s + 1);
        return PMCE_ERR_LAUNCH;
      }
    }
  }
  if constexpr (F16) return pmce_avgpool_nhwc_f16_f32(full[cur], feats, n, 49, 2048, stream);
  else return pmce_avgpool_nhwc_f32(full[cur], feats, n, 49, 2048, stream);
}

}  // namespace

extern "C" int pmce_extractor_forward(const pmce_extractor* e, const float* patches, long long sn, long long sc, long long sy, long long sx,
                                      float* feats, int n, float* tap1, float* tap2, float* tap3, float* tap4, void* workspace,
                                      size_t workspace_bytes, pmce_stream_t stream) {
  PMCE_REQUIRE(e && patches && feats && workspace, "extractor_forward: null pointer");
  PMCE_REQUIRE(e->arena.ready(), "extractor_forward: the extractor is not finalized");
  PMCE_REQUIRE(n >= 1 && n <= 4096, "extractor_forward: n must be in 1..4096 (got %d)", n);
  PMCE_TRY(pmce_net::check_workspace("extractor_forward", workspace, workspace_bytes, pmce_extractor_workspace_bytes_for(e, n)));
  float* const taps[4] = {tap1, tap2, tap3, tap4};
  return e->precision == 1 ? run_layers<_Float16>(e, patches, sn, sc, sy, sx, feats, n, taps, workspace, stream)
                           : run_layers<float>(e, patches, sn, sc, sy, sx, feats, n, taps, workspace, stream);
}
