// The sliced-ELL image of a sparse dense-stored A: the compaction pass of the K-step entries
// (csrc/lanczos_large.hip: one workgroup per graph; csrc/lanczos_wide.hip: a graph spread over many
// workgroups).  One implementation, included by both.
#pragma once
#include "common.hpp"
#include "conv_image.hpp"

// A (16.8 MB per graph at N = 2048, re-streamed every Lanczos step) never survives in a cache
// until its next use: non-temporal loads leave L2 / Infinity Cache to the fp64 Krylov basis.
__device__ __forceinline__ float4 lnz_stream_f4(const float* p) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}

namespace {

// ---- sliced-ELL image of a sparse dense-stored A (K-step entry, LNZ_KSTEP_COMPACT) ---------------
// The normalised Laplacian of a G(n, p = 0.01) graph (BASELINE config 5) is 99 % zeros, and the
// K-step recurrence multiplies by it K times.  The dense matrix is therefore read from HBM ONCE, by
// ell_compact_rows_kernel, which gathers the nonzeros of every 64-row slab g into
//   vals[b][g][k][i], cols[b][g][k][i] : entry k of row 64 g + i  (k < cap; zero padded up to
//   widths[b][g] = the slab's longest row rounded up to ELL_UNROLL)
// — 0.4 MB per graph at n = 2048, p = 0.01 instead of 16.8 MB — and the Lanczos steps run on that
// image (MODE 2 below).  A graph with a row of more than `cap` nonzeros raises over[b]; it is left
// to the dense symmetric stream, launched behind (gate).  Skipping an exact zero changes no sum, so
// the result is the dense kernels' up to the order of the fp64 additions.
constexpr int ELL_UNROLL = 8;
struct EllImage {
  const float* vals;
  const uint16_t* cols;
  const int32_t* widths;
  int cap;
};

// One wave per ROW (four rows per workgroup), the whole row requested before the first ballot: lane
// l holds float4 64 u + l of the row, u < 8 — four columns each (PAIR = false), or two columns of
// the two channels of a channels-last [N][N][2] block whose channel 0 is A (PAIR = true: the
// product's collate layout is read in place, its .x / .z are the entries).  Entry k of row 64 g + i
// goes to vals / cols [(g * cap + k) * 64 + i]; the rows of a slab are written by 64 different
// waves, so the slab's width is an atomic max (widths zeroed by the caller) and the zero entries
// up to it are written by ell_pad_kernel behind this launch.  4.3 GB in 0.67 ms (6.4 TB/s); the
// r06 form with one wave per SLAB (a row's ballots behind the previous row's) ran at 4.2 TB/s.
// The same pass can leave the image the large-graph conv gathers from (csrc/conv_sparse.hip,
// lnz_large_sparse_image's format: entries [B][N][ccap] = bf16(value) << 16 | column in the SAME
// entry order, counts, flag bits 0 = the two channels differ somewhere (PAIR only: both are in the
// float4 anyway), 1 = a row beyond ccap) — the collated L is then read from HBM once per batch for
// the Ritz pairs AND the seven conv layers.
struct ConvImageOut {
  unsigned* ent;      // NULL: not wanted
  float* vals;        // NULL: not wanted (the exact-fp32 form's unrounded values)
  int32_t* counts;
  int32_t* flags;
  int cap;
};

template <bool PAIR>
__global__ __launch_bounds__(256) void ell_compact_rows_kernel(
    const float* __restrict__ A, int64_t sb, int64_t sr, int B, int N, int cap,
    float* __restrict__ vals, uint16_t* __restrict__ cols, int32_t* __restrict__ widths,
    int32_t* __restrict__ rowcnt, int32_t* __restrict__ over, ConvImageOut cv) {
  const int lane = threadIdx.x & 63;
  const int64_t rid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (rid >= (int64_t)B * N) return;
  const int b = (int)(rid / N), r = (int)(rid - (int64_t)b * N);
  const int nslab = (N + 63) >> 6, g = r >> 6, i = r & 63;
  const float4* src = reinterpret_cast<const float4*>(A + (int64_t)b * sb + (int64_t)r * sr);
  const int64_t base = (((int64_t)b * nslab + g) * cap) * 64 + i;
  float* vs = vals + base;
  uint16_t* cs = cols + base;
  int k = 0;   // entries of this row so far (wave-uniform)
  unsigned* ce = cv.ent ? cv.ent + rid * cv.cap : nullptr;
  float* cvv = (cv.ent && cv.vals) ? cv.vals + rid * cv.cap : nullptr;
  bool differ = false;
  auto place = [&](const float v, const int col) {
    const bool nz = v != 0.f;
    const unsigned long long m = __ballot(nz);
    if (m == 0ull) return;
    const int pos = k + lane_rank(m);
    if (nz && pos < cap) {
      vs[(int64_t)pos * 64] = v;
      cs[(int64_t)pos * 64] = (uint16_t)col;
    }
    if (ce && nz && pos < cv.cap) {
      ce[pos] = conv_entry(v, col);
      if (cvv) cvv[pos] = v;
    }
    k += __popcll(m);
  };
  const int nq = PAIR ? N >> 1 : N >> 2;   // float4s per row
  for (int q0 = 0; q0 < nq; q0 += 64 * 8) {
    float4 x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int q = q0 + 64 * u + lane;
      x[u] = q < nq ? lnz_stream_f4(reinterpret_cast<const float*>(src + q)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int q = q0 + 64 * u + lane;
      if (PAIR) {
        differ |= (x[u].x != x[u].y) | (x[u].z != x[u].w);
        if (__ballot(x[u].x != 0.f || x[u].z != 0.f) == 0ull) continue;
        place(x[u].x, 2 * q);
        place(x[u].z, 2 * q + 1);
      } else {
        if (__ballot(x[u].x != 0.f || x[u].y != 0.f || x[u].z != 0.f || x[u].w != 0.f) == 0ull) continue;
        place(x[u].x, 4 * q);
        place(x[u].y, 4 * q + 1);
        place(x[u].z, 4 * q + 2);
        place(x[u].w, 4 * q + 3);
      }
    }
  }
  if (ce) {
    const int c = k < cv.cap ? k : cv.cap;
    conv_pad_row(ce, cvv, c, lane);
    const bool any_differ = __ballot(differ) != 0ull;
    if (lane == 0) {
      cv.counts[rid] = c;
      const int f = (any_differ ? 1 : 0) | (k > cv.cap ? 2 : 0);
      if (f) atomicOr(cv.flags, f);
    }
  }
  if (lane == 0) {
    if (k > cap) over[b] = 1;   // (every writer stores the same value)
    const int c = k < cap ? k : cap;
    rowcnt[rid] = c;
    atomicMax(widths + (int64_t)b * nslab + g, (c + ELL_UNROLL - 1) / ELL_UNROLL * ELL_UNROLL);
  }
}

// zero entries from a row's count up to its slab's width (one wave per slab, lane = row)
__global__ __launch_bounds__(256) void ell_pad_kernel(int B, int N, int cap, float* __restrict__ vals,
                                                      uint16_t* __restrict__ cols,
                                                      const int32_t* __restrict__ widths,
                                                      const int32_t* __restrict__ rowcnt) {
  const int lane = threadIdx.x & 63;
  const int nslab = (N + 63) >> 6;
  const int64_t sid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sid >= (int64_t)B * nslab) return;
  const int b = (int)(sid / nslab), g = (int)(sid - (int64_t)b * nslab);
  const int row = 64 * g + lane;
  const int w = widths[sid];
  const int c = row < N ? rowcnt[(int64_t)b * N + row] : 0;
  const int64_t base = sid * cap * 64 + lane;
  for (int k = c; k < w; ++k) {
    vals[base + (int64_t)k * 64] = 0.f;
    cols[base + (int64_t)k * 64] = 0;
  }
}

}  // namespace
