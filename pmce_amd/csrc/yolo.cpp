// The tracker's detector as one call: a darknet-style network (convolutional, shortcut, route, upsample and yolo sections; the published
// yolov3.cfg is the table pmce_amd/yolo.py passes) on the convolution of conv.hip and the kernels of yolo.hip.  Host code only: the
// table, the buffer plan made from it and the launch sequence (the weights' storage: net_weights.hpp).  Eval-mode BatchNorm arrives
// folded into each convolution's weight and bias (pmce_amd/yolo.py folds on the host in fp64).
//
// The plan.  A shortcut is the epilogue of the convolution before it (out = from + leaky(conv)), so that convolution has no map of its
// own.  A route with one source is another name for that source.  A route with two sources [upsample, tap] owns ONE buffer of the summed
// width: the upsample writes its slice, and the tap's producer writes the other slice in place through the output pitch - every reader
// of the tap reads it through that pitch.  The detection maps are the caller's.  Every other map is a buffer of the workspace that is
// born at the step that writes it and freed after the step of its last reader (first fit, lowest offset); sizes are counted in units of
// (S / 32)^2 floats per image, so one plan serves every input side and every batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "net_weights.hpp"
#include "../../include/pmce_hip.h"

namespace {

enum { K_CONV = 0, K_SHORTCUT = 1, K_ROUTE = 2, K_UPSAMPLE = 3, K_YOLO = 4 };
constexpr int TABLE_COLS = 9;  // kind, filters, size, stride, batch_normalize, leaky, source 0, source 1, anchor mask
constexpr int BUF_NONE = -1, BUF_CALLER = -2;
constexpr float LEAKY_SLOPE = 0.1f;

struct Layer {
  int kind, filters, size, stride, bn, leaky, src0, src1, mask;
  int C = 0, ds = 0;            // channels; the input side divided by the map's side
  int cin = 0;                  // convolutions
  int fused_into = -1;          // a convolution whose epilogue is the shortcut after it
  int root = -1;                // the layer whose storage this one names (itself unless a one-source route)
  int buf = BUF_NONE, coff = 0, pitch = 0;
  int det = -1;                 // detection convolution: which of the caller's maps
  pmce_net::Param w, b;         // convolutions: the folded OIHW weight and its bias (shaped by plan())
};

struct Buffer {
  long long units = 0, offset = -1;
  int birth = 1 << 30, death = -1;
};

}  // namespace

struct pmce_yolo {
  std::vector<Layer> layers;
  std::vector<Buffer> bufs;
  float anchors[9][2];
  int yolo_layer[3];
  int nc = 0;
  long long total_units = 0;
  int precision = 0;  // 0: the three-product split on fp32 maps; 1: one f16 product on f16 maps (the same plan, 2 bytes per element)
  pmce_net::Arena arena;
};

namespace {

int plan(pmce_yolo* y) {
  std::vector<Layer>& L = y->layers;
  const int n = (int)L.size();
  // ---- channels, sides, fusion, detection maps ----
  int n_yolo = 0;
  for (int i = 0; i < n; ++i) {
    Layer& l = L[i];
    l.root = i;
    switch (l.kind) {
      case K_CONV: {
        PMCE_REQUIRE(l.filters >= 1 && l.filters <= 4096 && (l.size == 1 || l.size == 3) && (l.stride == 1 || l.stride == 2) &&
                         (l.stride == 1 || l.size == 3),
                     "yolo_create: layer %d: a convolution has 1..4096 filters, size 1 or 3, stride 1, or 2 with size 3 (got %d, %d, %d)", i,
                     l.filters, l.size, l.stride);
        l.cin = i == 0 ? 3 : L[i - 1].C;
        PMCE_REQUIRE(i == 0 || (L[i - 1].kind != K_YOLO), "yolo_create: layer %d: a convolution cannot read a yolo layer", i);
        l.C = l.filters;
        l.ds = (i == 0 ? 1 : L[i - 1].ds) * l.stride;
        PMCE_REQUIRE(l.ds <= 32, "yolo_create: layer %d: the map is smaller than 1/32 of the input", i);
        l.w = pmce_net::Param(y->precision == 1 ? pmce_net::CONV_F16 : pmce_net::CONV, 4, l.filters, l.cin, l.size, l.size);
        l.b = pmce_net::Param(pmce_net::PLAIN, 1, l.filters);
        break;
      }
      case K_SHORTCUT: {
        PMCE_REQUIRE(i >= 2 && L[i - 1].kind == K_CONV && l.src0 >= 0 && l.src0 < i - 1 && L[l.src0].kind != K_YOLO && L[l.src0].kind != K_UPSAMPLE,
                     "yolo_create: layer %d: a shortcut follows a convolution and adds an earlier map (from = %d)", i, l.src0);
        PMCE_REQUIRE(L[l.src0].C == L[i - 1].C && L[l.src0].ds == L[i - 1].ds,
                     "yolo_create: layer %d: the shortcut's two maps differ (%d channels at 1/%d, %d at 1/%d)", i, L[l.src0].C, L[l.src0].ds,
                     L[i - 1].C, L[i - 1].ds);
        L[i - 1].fused_into = i;
        l.C = L[i - 1].C;
        l.ds = L[i - 1].ds;
        break;
      }
      case K_ROUTE: {
        PMCE_REQUIRE(l.src0 >= 0 && l.src0 < i && l.src1 < i && L[l.src0].kind != K_YOLO, "yolo_create: layer %d: bad route sources (%d, %d)", i,
                     l.src0, l.src1);
        if (l.src1 < 0) {
          PMCE_REQUIRE(L[l.src0].kind != K_UPSAMPLE, "yolo_create: layer %d: a route to an upsample alone is not supported", i);
          l.C = L[l.src0].C;
          l.ds = L[l.src0].ds;
          l.root = L[l.src0].root;
        } else {
          PMCE_REQUIRE(l.src0 == i - 1 && L[l.src0].kind == K_UPSAMPLE && (L[l.src1].kind == K_CONV || L[l.src1].kind == K_SHORTCUT) &&
                           L[l.src1].ds == L[l.src0].ds,
                       "yolo_create: layer %d: a two-source route joins the upsample before it with a convolution's or shortcut's map of the "
                       "same side (got %d, %d)", i, l.src0, l.src1);
          l.C = L[l.src0].C + L[l.src1].C;
          l.ds = L[l.src0].ds;
        }
        break;
      }
      case K_UPSAMPLE: {
        PMCE_REQUIRE(i >= 1 && L[i - 1].kind == K_CONV && L[i - 1].ds >= 2 && l.stride == 2,
                     "yolo_create: layer %d: an upsample (x2 only) follows a convolution", i);
        l.C = L[i - 1].C;
        l.ds = L[i - 1].ds / 2;
        break;
      }
      case K_YOLO: {
        PMCE_REQUIRE(n_yolo < 3, "yolo_create: layer %d: more than three yolo layers", i);
        PMCE_REQUIRE(i >= 1 && L[i - 1].kind == K_CONV && !L[i - 1].bn && !L[i - 1].leaky && L[i - 1].filters == 3 * (5 + y->nc),
                     "yolo_create: layer %d: a yolo layer follows a linear convolution with a bias and %d filters", i, 3 * (5 + y->nc));
        PMCE_REQUIRE(l.mask > 0 && l.mask < 512 && __builtin_popcount(l.mask) == 3, "yolo_create: layer %d: the mask selects three of nine anchors", i);
        L[i - 1].det = n_yolo;
        y->yolo_layer[n_yolo++] = i;
        l.C = L[i - 1].C;
        l.ds = L[i - 1].ds;
        break;
      }
      default:
        pmce_set_error("yolo_create: layer %d: unknown kind %d", i, l.kind);
        return PMCE_ERR_ARG;
    }
  }
  PMCE_REQUIRE(n_yolo == 3, "yolo_create: the table has %d yolo layers, three are needed", n_yolo);
  PMCE_REQUIRE(L[0].kind == K_CONV, "yolo_create: layer 0 must be a convolution");
  // ---- who reads whom (by layer, before names are resolved) ----
  std::vector<std::vector<int>> readers(n);
  for (int i = 0; i < n; ++i) {
    const Layer& l = L[i];
    if ((l.kind == K_CONV || l.kind == K_UPSAMPLE || l.kind == K_YOLO || l.kind == K_SHORTCUT) && i > 0) readers[i - 1].push_back(i);
    if (l.kind == K_SHORTCUT || l.kind == K_ROUTE) readers[l.src0].push_back(i);
    if (l.kind == K_ROUTE && l.src1 >= 0) readers[l.src1].push_back(i);
  }
  for (int i = 0; i < n; ++i) {
    const Layer& l = L[i];
    if (l.kind == K_CONV && l.fused_into >= 0)
      PMCE_REQUIRE(readers[i].size() == 1, "yolo_create: layer %d feeds a shortcut and is read elsewhere too: not supported", i);
    if (l.kind == K_CONV && l.det >= 0) PMCE_REQUIRE(readers[i].size() == 1, "yolo_create: layer %d: a detection map is read by its yolo layer only", i);
    if (l.kind == K_UPSAMPLE)
      PMCE_REQUIRE(readers[i].size() == 1 && L[readers[i][0]].kind == K_ROUTE && L[readers[i][0]].src1 >= 0,
                   "yolo_create: layer %d: an upsample is read by the two-source route after it only", i);
    if (l.kind == K_CONV && l.det < 0) PMCE_REQUIRE(l.filters % 4 == 0, "yolo_create: layer %d: a body convolution has a multiple of 4 filters", i);
  }
  // ---- storage: a buffer per map, one per concatenation ----
  std::vector<int> concat_of(n, -1);  // the two-source route a layer is the tap of
  for (int i = 0; i < n; ++i)
    if (L[i].kind == K_ROUTE && L[i].src1 >= 0) {
      PMCE_REQUIRE(concat_of[L[i].src1] < 0, "yolo_create: layer %d is the tap of two concatenations: not supported", L[i].src1);
      concat_of[L[i].src1] = i;
    }
  y->bufs.clear();
  auto new_buf = [&](long long units) {
    Buffer b;
    b.units = units;
    y->bufs.push_back(b);
    return (int)y->bufs.size() - 1;
  };
  auto units_of = [&](int C, int ds) { return (long long)C * (32 / ds) * (32 / ds); };
  for (int i = 0; i < n; ++i) PMCE_REQUIRE(32 % L[i].ds == 0, "yolo_create: layer %d: the side ratio %d does not divide 32", i, L[i].ds);
  for (int i = 0; i < n; ++i)  // the concatenations first: their parts point into them
    if (L[i].kind == K_ROUTE && L[i].src1 >= 0) {
      L[i].buf = new_buf(units_of(L[i].C, L[i].ds));
      L[i].coff = 0;
      L[i].pitch = L[i].C;
    }
  for (int i = 0; i < n; ++i) {
    Layer& l = L[i];
    if (l.kind == K_YOLO || (l.kind == K_CONV && l.fused_into >= 0)) continue;
    if (l.kind == K_CONV && l.det >= 0) {
      l.buf = BUF_CALLER;
      l.pitch = l.C;
    } else if (l.kind == K_UPSAMPLE) {
      const Layer& r = L[i + 1];
      l.buf = r.buf; l.coff = 0; l.pitch = r.C;
    } else if ((l.kind == K_CONV || l.kind == K_SHORTCUT) && concat_of[i] >= 0) {
      const Layer& r = L[concat_of[i]];
      l.buf = r.buf; l.coff = L[r.src0].C; l.pitch = r.C;
    } else if (l.kind == K_CONV || l.kind == K_SHORTCUT) {
      l.buf = new_buf(units_of(l.C, l.ds));
      l.coff = 0; l.pitch = l.C;
    }
  }
  for (int i = 0; i < n; ++i)  // one-source routes: the name of their (already resolved) source
    if (L[i].kind == K_ROUTE && L[i].src1 < 0) {
      const Layer& s = L[L[i].root];
      L[i].buf = s.buf; L[i].coff = s.coff; L[i].pitch = s.pitch;
    }
  // ---- lifetimes: the step of an operation is the index of the layer it completes ----
  auto touch = [&](int layer, int step, bool write) {
    const int b = L[layer].buf;
    if (b < 0) return;
    Buffer& bf = y->bufs[b];
    if (write) bf.birth = std::min(bf.birth, step);
    bf.death = std::max(bf.death, step);
  };
  for (int i = 0; i < n; ++i) {
    const Layer& l = L[i];
    if (l.kind == K_CONV && l.fused_into < 0) {
      if (i > 0) touch(i - 1, i, false);
      touch(i, i, true);
    } else if (l.kind == K_SHORTCUT) {
      touch(i - 2, i, false);
      touch(l.src0, i, false);
      touch(i, i, true);
    } else if (l.kind == K_UPSAMPLE) {
      touch(i - 1, i, false);
      touch(i, i, true);
    }
  }
  // ---- first fit in the order of birth; a buffer is freed after the step of its last reader ----
  std::vector<int> order(y->bufs.size());
  for (size_t b = 0; b < order.size(); ++b) order[b] = (int)b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return y->bufs[a].birth < y->bufs[b].birth; });
  y->total_units = 0;
  std::vector<int> placed;
  for (int b : order) {
    Buffer& nb = y->bufs[b];
    PMCE_REQUIRE(nb.birth <= nb.death, "yolo_create: a map is read before it is written");
    std::vector<std::pair<long long, long long>> busy;
    for (int o : placed)
      if (y->bufs[o].death >= nb.birth) busy.push_back({y->bufs[o].offset, y->bufs[o].offset + y->bufs[o].units});
    std::sort(busy.begin(), busy.end());
    long long at = 0;
    for (const auto& iv : busy) {
      if (at + nb.units <= iv.first) break;
      at = std::max(at, iv.second);
    }
    nb.offset = at;
    placed.push_back(b);
    y->total_units = std::max(y->total_units, at + nb.units);
  }
  return PMCE_OK;
}

}  // namespace

extern "C" int pmce_yolo_create(const int* table, int n_layers, const float* anchors18, int num_classes, pmce_yolo** out) {
  return pmce_yolo_create_precision(table, n_layers, anchors18, num_classes, 0, out);
}

extern "C" int pmce_yolo_precision(const pmce_yolo* y) { return y ? y->precision : -1; }

extern "C" int pmce_yolo_create_precision(const int* table, int n_layers, const float* anchors18, int num_classes, int precision, pmce_yolo** out) {
  PMCE_REQUIRE(table && anchors18 && out, "yolo_create: null pointer");
  PMCE_REQUIRE(precision == 0 || precision == 1, "yolo_create: precision must be 0 (split_f16) or 1 (f16) (got %d)", precision);
  PMCE_REQUIRE(n_layers >= 4 && n_layers <= 4096, "yolo_create: the table has 4..4096 layers (got %d)", n_layers);
  PMCE_REQUIRE(num_classes >= 1 && num_classes <= 255, "yolo_create: num_classes must be in 1..255 (got %d)", num_classes);
  pmce_yolo* y = new pmce_yolo();
  y->nc = num_classes;
  y->precision = precision;
  for (int a = 0; a < 9; ++a)
    for (int k = 0; k < 2; ++k) {
      y->anchors[a][k] = anchors18[2 * a + k];
      if (!(y->anchors[a][k] > 0.f && y->anchors[a][k] < 1e6f)) {
        pmce_set_error("yolo_create: anchor %d must be positive and finite", a);
        delete y;
        return PMCE_ERR_ARG;
      }
    }
  y->layers.resize(n_layers);
  for (int i = 0; i < n_layers; ++i) {
    const int* t = table + i * TABLE_COLS;
    Layer& l = y->layers[i];
    l.kind = t[0]; l.filters = t[1]; l.size = t[2]; l.stride = t[3]; l.bn = t[4]; l.leaky = t[5]; l.src0 = t[6]; l.src1 = t[7]; l.mask = t[8];
  }
  const int rc = plan(y);
  if (rc != PMCE_OK) {
    delete y;
    return rc;
  }
  *out = y;
  return PMCE_OK;
}

extern "C" void pmce_yolo_destroy(pmce_yolo* y) { delete y; }

extern "C" int pmce_yolo_layer_count(const pmce_yolo* y) { return y ? (int)y->layers.size() : 0; }

extern "C" int pmce_yolo_conv_shape(const pmce_yolo* y, int i, int* shape4) {
  PMCE_REQUIRE(y && shape4 && i >= 0 && i < (int)y->layers.size() && y->layers[i].kind == K_CONV, "yolo_conv_shape: layer %d is not a convolution", i);
  const Layer& l = y->layers[i];
  shape4[0] = l.filters; shape4[1] = l.cin; shape4[2] = l.size; shape4[3] = l.size;
  return PMCE_OK;
}

extern "C" int pmce_yolo_layer_plan(const pmce_yolo* y, int i, long long* plan8) {
  PMCE_REQUIRE(y && plan8 && i >= 0 && i < (int)y->layers.size(), "yolo_layer_plan: bad arguments");
  const Layer& l = y->layers[i];
  plan8[0] = l.C; plan8[1] = l.ds; plan8[2] = l.buf; plan8[3] = l.coff; plan8[4] = l.pitch;
  plan8[5] = l.buf >= 0 ? y->bufs[l.buf].offset : -1;
  plan8[6] = l.buf >= 0 ? y->bufs[l.buf].units : 0;
  plan8[7] = l.buf >= 0 ? y->bufs[l.buf].death : -1;
  return PMCE_OK;
}

extern "C" long long pmce_yolo_workspace_units(const pmce_yolo* y) { return y ? y->total_units : 0; }

extern "C" int pmce_yolo_set_conv(pmce_yolo* y, int layer, const float* folded_weight, const float* folded_bias) {
  PMCE_REQUIRE(y && folded_weight && folded_bias, "yolo_set_conv: null pointer");
  PMCE_REQUIRE(!y->arena.ready(), "yolo_set_conv: the network is finalized");
  PMCE_REQUIRE(layer >= 0 && layer < (int)y->layers.size() && y->layers[layer].kind == K_CONV, "yolo_set_conv: layer %d is not a convolution", layer);
  y->layers[layer].w.src = folded_weight;
  y->layers[layer].b.src = folded_bias;
  return PMCE_OK;
}

extern "C" int pmce_yolo_finalize_on(pmce_yolo* y, pmce_stream_t stream) {
  PMCE_REQUIRE(y, "yolo_finalize: null pointer");
  std::vector<pmce_net::Param*> params;
  std::vector<int> layer_of;
  for (size_t i = 0; i < y->layers.size(); ++i) {
    Layer& l = y->layers[i];
    if (l.kind != K_CONV) continue;
    params.push_back(&l.w);
    params.push_back(&l.b);
    layer_of.insert(layer_of.end(), 2, (int)i);
  }
  auto label = [&](size_t i) { return "the convolution of layer " + std::to_string(layer_of[i]); };
  return pmce_net::finalize("yolo_finalize", params, label, y->arena, stream);
}

extern "C" size_t pmce_yolo_workspace_bytes(const pmce_yolo* y, int n, int S) {
  if (!y || n < 1 || n > 1024 || S < 32 || S > 1024 || S % 32 != 0) {
    pmce_set_error("yolo_workspace_bytes: n must be in 1..1024 and the side a multiple of 32 in 32..1024 (got n=%d S=%d)", n, S);
    return 0;
  }
  return (size_t)n * (size_t)y->total_units * (size_t)(S / 32) * (size_t)(S / 32) * (y->precision == 1 ? 2 : sizeof(float));
}

namespace {

// The launch sequence of a forward on workspace maps of T: float (the three-product convolution) or _Float16 (the single-product one:
// the stem rounds the fp32 images in its gather, shortcuts add an f16 residual).  The detection maps are the caller's, fp32 in both.
template <typename T>
int run_layers(const pmce_yolo* y, const float* images, long long sn, long long sc, long long sy, long long sx, int n, int S,
               float* const* maps, void* workspace, hipStream_t stream) {
  constexpr bool F16 = sizeof(T) == 2;
  T* ws = static_cast<T*>(workspace);
  const size_t unit = (size_t)n * (size_t)(S / 32) * (size_t)(S / 32);
  const std::vector<Layer>& L = y->layers;
  auto at = [&](int i) -> T* { return ws + unit * (size_t)y->bufs[L[i].buf].offset + L[i].coff; };  // first channel of layer i's workspace map
  // the convolution of layer ci, its result (and an optional residual) where layer `dst` lives
  auto conv = [&](int ci, int dst, int res) {
    const Layer& c = L[ci];
    const Layer& o = L[dst];
    const void* x = images;
    long long xn = sn, xc = sc, xy = sy, xx = sx;
    int side = S;
    if (ci > 0) {
      const Layer& in = L[ci - 1];
      side = S / in.ds;
      x = at(ci - 1);
      xc = 1; xx = in.pitch; xy = (long long)side * in.pitch; xn = (long long)side * side * in.pitch;
    }
    const bool det = o.buf == BUF_CALLER;
    void* out = det ? static_cast<void*>(maps[o.det] + o.coff) : static_cast<void*>(at(dst));
    const void* r = res >= 0 ? at(res) : nullptr;
    const long long ldr = res >= 0 ? L[res].pitch : 0;
    const int pad = (c.size - 1) / 2, act = c.leaky ? 2 : 0;
    if constexpr (F16)
      return pmce_conv2d_act_f16(x, ci > 0 ? 1 : 0, xn, xc, xy, xx, n, c.cin, side, side, c.w.dev, c.w.wscale, c.b.dev, r, ldr, out, o.pitch,
                                 det ? 0 : 1, c.filters, c.size, c.size, c.stride, pad, act, LEAKY_SLOPE, 1, stream);
    else
      return pmce_conv2d_act_split_f16(static_cast<const float*>(x), xn, xc, xy, xx, n, c.cin, side, side, c.w.dev, c.w.wscale, c.b.dev,
                                       static_cast<const float*>(r), ldr, static_cast<float*>(out), o.pitch, c.filters, c.size, c.size, c.stride,
                                       pad, act, LEAKY_SLOPE, 1, stream);
  };
  for (int i = 0; i < (int)L.size(); ++i) {
    const Layer& l = L[i];
    if (l.kind == K_CONV && l.fused_into < 0) PMCE_TRY(conv(i, i, -1));
    else if (l.kind == K_SHORTCUT) PMCE_TRY(conv(i - 1, i, l.src0));
    else if (l.kind == K_UPSAMPLE) {
      const Layer& in = L[i - 1];
      if constexpr (F16) PMCE_TRY(pmce_upsample2x_nhwc_f16(at(i - 1), in.pitch, at(i), l.pitch, n, S / in.ds, S / in.ds, l.C, stream));
      else PMCE_TRY(pmce_upsample2x_nhwc_f32(at(i - 1), in.pitch, at(i), l.pitch, n, S / in.ds, S / in.ds, l.C, stream));
    }
  }
  return PMCE_OK;
}

}  // namespace

extern "C" int pmce_yolo_forward(const pmce_yolo* y, const float* images, long long sn, long long sc, long long sy, long long sx, int n, int S,
                                 float* map0, float* map1, float* map2, float* rows, void* workspace, size_t workspace_bytes,
                                 pmce_stream_t stream) {
  PMCE_REQUIRE(y && images && map0 && map1 && map2 && workspace, "yolo_forward: null pointer");
  PMCE_REQUIRE(y->arena.ready(), "yolo_forward: the network is not finalized");
  PMCE_REQUIRE(n >= 1 && n <= 1024 && S >= 32 && S <= 1024 && S % 32 == 0,
               "yolo_forward: n must be in 1..1024 and the side a multiple of 32 in 32..1024 (got n=%d S=%d)", n, S);
  PMCE_TRY(pmce_net::check_workspace("yolo_forward", workspace, workspace_bytes, pmce_yolo_workspace_bytes(y, n, S)));
  float* maps[3] = {map0, map1, map2};
  const std::vector<Layer>& L = y->layers;
  PMCE_TRY(y->precision == 1 ? run_layers<_Float16>(y, images, sn, sc, sy, sx, n, S, maps, workspace, stream)
                             : run_layers<float>(y, images, sn, sc, sy, sx, n, S, maps, workspace, stream));
  if (!rows) return PMCE_OK;
  long long pitches[3];
  int grids[3];
  float anchors[18];
  for (int k = 0; k < 3; ++k) {
    const Layer& yl = L[y->yolo_layer[k]];
    pitches[k] = L[y->yolo_layer[k] - 1].pitch;
    grids[k] = S / yl.ds;
    int a = 0;
    for (int bit = 0; bit < 9; ++bit)
      if (yl.mask >> bit & 1) {
        anchors[(k * 3 + a) * 2] = y->anchors[bit][0];
        anchors[(k * 3 + a) * 2 + 1] = y->anchors[bit][1];
        ++a;
      }
  }
  return pmce_yolo_decode_f32(map0, map1, map2, pitches, grids, anchors, n, y->nc, S, rows, stream);
}
