// What a demo network's handle (extractor.cpp, vitpose.cpp, yolo.cpp) keeps on the device: its parameters in ONE allocation, made by ONE
// finalize.  A network lists its parameters; where a packed tensor lies, how many floats it takes and what happens when a step fails
// is decided here and nowhere else.  (model.cpp is not a client: its arena is the caller's and is shared between models.)
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "common.hpp"

namespace pmce_net {

// PLAIN: copied as it is; LINEAR: [N][K] packed for the three-product GEMM; CONV: OIHW packed for the convolution;
// LINEAR_F16: [N][K] packed for pmce_gemm_nt_f16 (one f16 per weight - half of LINEAR's planes), wscale as for LINEAR;
// CONV_F16: OIHW packed for pmce_conv2d_act_f16 (one f16 per weight - half of CONV's planes), wscale as for CONV
enum Kind { PLAIN, LINEAR, CONV, LINEAR_F16, CONV_F16 };

struct Param {
  Kind kind = PLAIN;
  int rank = 0;
  int shape[4] = {0, 0, 0, 0};
  const float* src = nullptr;  // the caller's tensor (device), read by finalize
  float* dev = nullptr;        // inside the arena: the copy (PLAIN) or the planes
  float* wscale = nullptr;     // packed tensors: one power of two per output row
  Param() = default;
  Param(Kind kind_, int rank_, int s0, int s1 = 0, int s2 = 0, int s3 = 0) : kind(kind_), rank(rank_), shape{s0, s1, s2, s3} {}
  size_t floats() const;   // of the caller's tensor
  size_t planes() const;   // of the arena up to wscale (packed tensors)
  size_t storage() const;  // of the arena in all: every slice starts on a 256-byte boundary
};

// The block that holds every parameter of one handle.  A handle is finalized exactly when its arena holds the block.
struct Arena {
  float* base = nullptr;
  Arena() = default;
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() { release(); }
  bool ready() const { return base != nullptr; }
  void release();
};

// Checks that every src is set (`label(i)` supplies the words in front of "was not set"), allocates the arena, places every parameter,
// packs (LINEAR, CONV and their F16 forms) or copies (PLAIN) it on `stream` in the order of the list, waits - the caller may free its tensors when this
// returns - and clears every src.  A failure after the allocation frees the arena: the handle stays un-finalized and may try again.
int finalize(const char* who, const std::vector<Param*>& params, const std::function<std::string(size_t)>& label, Arena& arena, hipStream_t stream);

// A forward's workspace: 16-byte aligned and at least `need` bytes.
int check_workspace(const char* who, const void* ptr, size_t got, size_t need);

}  // namespace pmce_net
