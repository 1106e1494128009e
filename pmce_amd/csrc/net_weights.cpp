// The weight arena of the demo networks (net_weights.hpp).  Host code only.
#include "net_weights.hpp"

#include "../../include/pmce_hip.h"

namespace pmce_net {

static size_t align64(size_t floats) { return (floats + 63) / 64 * 64; }

size_t Param::floats() const {
  size_t f = 1;
  for (int i = 0; i < rank; ++i) f *= (size_t)shape[i];
  return f;
}

size_t Param::planes() const {
  if (kind == LINEAR) return align64(((size_t)shape[0] + 63) / 64 * 64 * (size_t)shape[1]);
  if (kind == LINEAR_F16) return align64(((size_t)pmce_gemm_packed_f16_halves(shape[0], shape[1]) + 1) / 2);
  if (kind == CONV_F16) return align64(((size_t)pmce_conv_packed_halves(shape[0], shape[1], shape[2], shape[3]) + 1) / 2);
  return align64((size_t)pmce_conv_packed_floats(shape[0], shape[1], shape[2], shape[3]));
}

size_t Param::storage() const { return kind == PLAIN ? align64(floats()) : planes() + align64((size_t)shape[0]); }

void Arena::release() {
  if (base) (void)hipFree(base);
  base = nullptr;
}

// places, then packs or copies, every parameter; waits
static int fill(const char* who, const std::vector<Param*>& params, const std::function<std::string(size_t)>& label, float* at, hipStream_t stream) {
  for (size_t i = 0; i < params.size(); ++i) {
    Param& p = *params[i];
    p.dev = at;
    p.wscale = p.kind == PLAIN ? nullptr : at + p.planes();
    at += p.storage();
    if (p.kind == LINEAR) {
      PMCE_TRY(pmce_gemm_pack_split_f16(p.src, p.shape[0], p.shape[1], p.shape[1], p.dev, p.wscale, 1, stream));
    } else if (p.kind == LINEAR_F16) {
      PMCE_TRY(pmce_gemm_pack_f16(p.src, p.shape[0], p.shape[1], p.shape[1], p.dev, p.wscale, stream));
    } else if (p.kind == CONV_F16) {
      PMCE_TRY(pmce_conv_pack_f16(p.src, p.shape[0], p.shape[1], p.shape[2], p.shape[3], p.dev, p.wscale, stream));
    } else if (p.kind == CONV) {
      PMCE_TRY(pmce_conv_pack_split_f16(p.src, p.shape[0], p.shape[1], p.shape[2], p.shape[3], p.dev, p.wscale, stream));
    } else if (hipMemcpyAsync(p.dev, p.src, p.floats() * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
      pmce_set_error("%s: copying %s failed", who, label(i).c_str());
      return PMCE_ERR_LAUNCH;
    }
  }
  if (hipStreamSynchronize(stream) != hipSuccess) {
    pmce_set_error("%s: the packing kernels failed: %s", who, hipGetErrorString(hipGetLastError()));
    return PMCE_ERR_LAUNCH;
  }
  return PMCE_OK;
}

int finalize(const char* who, const std::vector<Param*>& params, const std::function<std::string(size_t)>& label, Arena& arena, hipStream_t stream) {
  PMCE_REQUIRE(!arena.ready(), "%s: already finalized", who);
  size_t floats = 0;
  for (size_t i = 0; i < params.size(); ++i) {
    PMCE_REQUIRE(params[i]->src, "%s: %s was not set", who, label(i).c_str());
    floats += params[i]->storage();
  }
  const hipError_t rc = hipMalloc(reinterpret_cast<void**>(&arena.base), floats * sizeof(float));
  if (rc != hipSuccess) {
    arena.base = nullptr;
    pmce_set_error("%s: hipMalloc(%zu bytes) for the weights failed: %s", who, floats * sizeof(float), hipGetErrorString(rc));
    return PMCE_ERR_WORKSPACE;
  }
  const int frc = fill(who, params, label, arena.base, stream);
  if (frc != PMCE_OK) {
    arena.release();
    return frc;
  }
  for (Param* p : params) p->src = nullptr;
  return PMCE_OK;
}

int check_workspace(const char* who, const void* ptr, size_t got, size_t need) {
  PMCE_REQUIRE((reinterpret_cast<uintptr_t>(ptr) & 15) == 0 && got >= need, "%s: the workspace must be 16-byte aligned and hold %zu bytes (got %zu)",
               who, need, got);
  return PMCE_OK;
}

}  // namespace pmce_net
