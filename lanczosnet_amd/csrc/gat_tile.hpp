// What the GAT kernels share (gat.hip: attention and readout; gat_grad.hip: their backward): the envelope,
// the LDS row strides and the host's pointer checks.
#pragma once
#include "common.hpp"

namespace {

constexpr int GN = 32;        // nodes per molecule at most
constexpr int GD = 32;        // head width at most
constexpr int GW = 4;         // waves per workgroup
constexpr int LS = GN + 1;    // row stride of the L and attention blocks (floats): column reads conflict-free
constexpr int WS = GD + 4;    // row stride of a staged Wh / dO block: 16-byte rows for ds_read_b128
constexpr int RP = 16;        // outputs at most

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// [p, p + ((rows - 1) ld + width) floats)
inline bool overlap(const void* p, const void* q, uint64_t rows, int ldp, int ldq, int width) {
  const uintptr_t p0 = (uintptr_t)p, p1 = p0 + ((rows - 1) * (uint64_t)ldp + width) * sizeof(float);
  const uintptr_t q0 = (uintptr_t)q, q1 = q0 + ((rows - 1) * (uint64_t)ldq + width) * sizeof(float);
  return !(p1 <= q0 || q1 <= p0);
}

}  // namespace
