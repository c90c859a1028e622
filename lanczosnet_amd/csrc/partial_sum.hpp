// The second launch of the weight gradients that gat_grad.hip and ggnn_grad.hip leave as per-molecule partials
// in a workspace [B][M]: the B rows added per output in a fixed order.
#pragma once
#include "common.hpp"

namespace {

// out[col] = the sum over the B rows of ws [B][M], col < M, cut into up to five consecutive segments with
// an output pointer each.  Fixed order: four contiguous quarters of the rows, each ascending, then
// ((q0 + q1) + q2) + q3.
struct Segments {
  float* p[5];
  int n[5];
};

__global__ __launch_bounds__(256) void partial_sum_kernel(const float* __restrict__ ws, int B, int64_t M,
                                                          Segments seg) {
  __shared__ float part[4][64];
  const int x = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + x;
  const int q = (B + 3) / 4;
  const int b0 = s * q, b1 = min(B, b0 + q);
  float acc = 0.0f;
  if (col < M)
    for (int b = b0; b < b1; ++b) acc += ws[(int64_t)b * M + col];
  part[s][x] = acc;
  __syncthreads();
  if (s == 0 && col < M) {
    const float v = ((part[0][x] + part[1][x]) + part[2][x]) + part[3][x];
    int64_t off = col;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      if (off >= 0 && off < seg.n[k]) seg.p[k][off] = v;
      off -= seg.n[k];
    }
  }
}

// the launch: `what` names the entry point in an error
inline int sum_partials(const float* ws, int B, int64_t M, const Segments& seg, hipStream_t stream, const char* what) {
  hipLaunchKernelGGL(partial_sum_kernel, dim3((unsigned)((M + 63) / 64)), dim3(256), 0, stream, ws, B, M, seg);
  return lnz::check_launch(what);
}

}  // namespace
