// Large graphs from edge lists: the sliced-ELL image of the K-step recurrence and the row-major
// image of the sparse conv, built straight from a batch of undirected edge lists — bit for bit what
// ell_compact_rows_kernel + ell_pad_kernel (csrc/ell_image.hpp) gather from the dense collated
// L4 = D^-1/2 (I + A) D^-1/2 (csrc/laplacian.hip), without an N x N array on either side.
// Replaces, for unweighted simple graphs with one edge type, utils/data_helper.py:92-116,155-156
// (normalize_adj / get_laplacian 'L4') and dataset/get_graph_data.py:61-72.
//
//   init     zero the cursors, status / over / widths / flags words (one launch instead of five memsets)
//   scatter  one thread per edge: validate BEFORE any indexed access, then claim a slot in each
//            endpoint's staging row through an integer cursor (the cursor's final value is the node's
//            neighbour count) and store the neighbour's column there
//   rows     one wave per row: the staged columns + the diagonal through LDS, each ranked by counting
//            the entries in front of it in the dense compaction's order (order_key below), value (float)((s_i * 1.0) * s_j) with
//            s = 1.0 / sqrt((double)deg), deg = 1 + neighbours (the expression of laplacian.hip:77-79),
//            written at its rank into both images; counts, widths (atomic max), over / flag bit 1
//   finish   a graph with a non-zero status: its image rows emptied; status or over: D, V, info zeroed
//            and the gate word of the Ritz launch raised
// Only integer atomics, and every stored word is a function of the edge SET: the order of the edges
// and of the endpoints changes which staging slot a column lands in, and the ranking undoes that.
// Typed batches (edge_type [n_edges] in [0, E), E = 2 .. 7; dataset/get_graph_data.py:60-72): the same four
// launches write one conv image per operator channel — see edge_typed_rows_kernel below.
#include "edge_image.hpp"
#include "ell_image.hpp"

#include <algorithm>

namespace {

using lnz::EdgeBatch;
using lnz::EdgeConv;
using lnz::EdgeEll;
using lnz::EdgeRitz;

inline int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }

// The dense compaction (ell_compact_rows_kernel, sparse_image_kernel) meets a row's nonzeros in the
// order of its vector loads, not in column order: a wave takes 64 float4s at a time and ballots
// component by component.  On the channels-last pair a float4 is columns 2q, 2q + 1 (x two channels):
// within every 128 columns the even ones come first, then the odd ones (PAIR).  On contiguous rows a
// float4 is columns 4q .. 4q + 3: within every 256 columns, column % 4 == 0 first, then 1, 2, 3 (QUAD).
// Only the 4-byte form walks in column order.  The Lanczos SpMV and the conv gather sum in ENTRY order,
// so an image that stands in for a dense one bit for bit keeps that order: entries are ranked by this
// key (a bijection of the columns).
__device__ __forceinline__ int order_key(int col, int order) {
  if (order == LNZ_EDGE_ORDER_PAIR) return (col & ~127) | ((col & 1) << 6) | ((col & 127) >> 1);
  if (order == LNZ_EDGE_ORDER_QUAD) return (col & ~255) | ((col & 3) << 6) | ((col & 255) >> 2);
  return col;
}

__global__ __launch_bounds__(256) void edge_init_kernel(int B, int N, int nslab, int32_t* __restrict__ cursor,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ over,
                                                        int32_t* __restrict__ widths, int32_t* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < (int64_t)B * N) cursor[t] = 0;
  if (t < B) {
    status[t] = 0;
    if (over) over[t] = 0;
  }
  if (widths && t < (int64_t)B * nslab) widths[t] = 0;
  if (flags && t == 0) flags[0] = 0;
}

// Workgroup (x, b): edges edge_off[b] + 256 x + t, + 256 gridDim.x, ... of graph b.  A graph whose
// offsets or node count are out of range is flagged and left alone (no edge of it is read).
__global__ __launch_bounds__(256) void edge_scatter_kernel(EdgeBatch g, int scap, int32_t* __restrict__ cursor,
                                                           uint16_t* __restrict__ stage,
                                                           int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  const int64_t lo = g.edge_off[b], hi = g.edge_off[b + 1];
  const int n = g.n_nodes[b];
  const bool bad_off = lo < 0 || hi < lo || hi > g.n_edges, bad_n = n < 0 || n > g.N;
  if (bad_off || bad_n) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      atomicOr(status + b, (bad_off ? lnz::kEdgeOffsets : 0) | (bad_n ? lnz::kEdgeNodes : 0));
    return;
  }
  const int2* ev = reinterpret_cast<const int2*>(g.edges);
  const int64_t row0 = (int64_t)b * g.N;
  for (int64_t e = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; e < hi; e += (int64_t)gridDim.x * 256) {
    const int2 uv = ev[e];
    if (uv.x < 0 || uv.x >= n || uv.y < 0 || uv.y >= n) {
      atomicOr(status + b, lnz::kEdgeEndpoint);
      continue;
    }
    if (uv.x == uv.y) {
      atomicOr(status + b, lnz::kEdgeSelfLoop);
      continue;
    }
    // a row of scap or more entries (the diagonal included) overflows every image: scap - 1 slots do
    const int su = atomicAdd(cursor + row0 + uv.x, 1);
    if (su < scap - 1) stage[(row0 + uv.x) * scap + su] = (uint16_t)uv.y;
    const int sv = atomicAdd(cursor + row0 + uv.y, 1);
    if (sv < scap - 1) stage[(row0 + uv.y) * scap + sv] = (uint16_t)uv.x;
  }
}

// One wave per row, four rows per workgroup; lane l holds entries l, l + 64, l + 128, l + 192 of the
// row's unsorted list (staged neighbours, then the diagonal).  The layout written is the one of
// ell_compact_rows_kernel: ELL entry k of row 64 g + i at [(g * cap + k) * 64 + i], conv row
// zero padded to a multiple of eight.  A row beyond a capacity keeps the first of its staged entries
// in the image's order (such an image is not used: over / flag bit 1).
__global__ __launch_bounds__(256) void edge_rows_kernel(EdgeBatch g, int scap, const int32_t* __restrict__ cursor,
                                                        const uint16_t* __restrict__ stage, EdgeEll ell, EdgeConv cv,
                                                        int32_t* __restrict__ status) {
  __shared__ int list[4][lnz::kEdgeMaxCap];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rid = (int64_t)blockIdx.x * 4 + wave;
  const bool valid = rid < (int64_t)g.B * g.N;
  const int b = valid ? (int)(rid / g.N) : 0, r = valid ? (int)(rid - (int64_t)b * g.N) : 0;
  const bool live = valid && status[b] == 0 && r < g.n_nodes[b];   // (status 0: n_nodes[b] is in [0, N])
  const int nnb = live ? cursor[rid] : 0;
  const int k = live ? nnb + 1 : 0;                      // the row's entries
  const int m = live ? min(nnb, scap - 1) : 0;           // ... of which staged neighbours
  const int items = live ? m + 1 : 0;
  int col[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = lane + 64 * u;
    col[u] = t < m ? (int)stage[rid * scap + t] : r;
    if (t < items) list[wave][t] = col[u];
  }
  __syncthreads();
  // rank = the entries in front of this one (dup: the same column twice).  The two images may stand in for
  // dense forms read with different vector loads: a second rank only then (wave-uniform)
  const int order0 = ell.cap ? ell.order : cv.order;
  const bool two = ell.cap && cv.ent && cv.order != ell.order;
  int key0[4], key1[4], rank[4] = {0, 0, 0, 0}, rank1[4] = {0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    key0[u] = order_key(col[u], order0);
    key1[u] = order_key(col[u], cv.order);
  }
  bool dup = false;
  for (int j = 0; j < items; ++j) {
    const int x = list[wave][j];   // (a broadcast read)
    const int x0 = order_key(x, order0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = lane + 64 * u;
      rank[u] += (x0 < key0[u] || (x0 == key0[u] && j < t)) ? 1 : 0;
      dup |= t < items && x == col[u] && j != t;
    }
    if (two) {
      const int x1 = order_key(x, cv.order);
#pragma unroll
      for (int u = 0; u < 4; ++u) rank1[u] += (x1 < key1[u] || (x1 == key1[u] && j < lane + 64 * u)) ? 1 : 0;
    }
  }
  const int nslab = (g.N + 63) >> 6;
  const int64_t ebase = (((int64_t)b * nslab + (r >> 6)) * ell.cap) * 64 + (r & 63);
  unsigned* ce = (valid && cv.ent) ? cv.ent + rid * cv.cap : nullptr;
  float* cvv = (ce && cv.vals) ? cv.vals + rid * cv.cap : nullptr;
  const double si = 1.0 / sqrt((double)(nnb + 1));
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = lane + 64 * u;
    if (t >= items) continue;
    const int c = col[u], pos = rank[u], cpos = two ? rank1[u] : rank[u];
    const int dc = c == r ? nnb : cursor[(int64_t)b * g.N + c];   // (c < n_b: checked before it was staged)
    const double sj = 1.0 / sqrt((double)(dc + 1));
    const float v = (float)((si * 1.0) * sj);
    if (pos < ell.cap) {
      ell.vals[ebase + (int64_t)pos * 64] = v;
      ell.cols[ebase + (int64_t)pos * 64] = (uint16_t)c;
    }
    if (ce && cpos < cv.cap) {
      ce[cpos] = conv_entry(v, c);
      if (cvv) cvv[cpos] = v;
    }
  }
  if (!valid) return;
  if (ce) {
    const int c = k < cv.cap ? k : cv.cap;
    conv_pad_row(ce, cvv, c, lane);
    if (lane == 0) {
      cv.counts[rid] = c;
      if (k > cv.cap) atomicOr(cv.flags, 2);
    }
  }
  if (ell.cap && lane == 0) {
    if (k > ell.cap) ell.over[b] = 1;   // (every writer stores the same value)
    const int c = k < ell.cap ? k : ell.cap;
    ell.rowcnt[rid] = c;
    atomicMax(ell.widths + (int64_t)b * nslab + (r >> 6), (c + ELL_UNROLL - 1) / ELL_UNROLL * ELL_UNROLL);
  }
  if (__ballot(dup) != 0ull && lane == 0) atomicOr(status + b, lnz::kEdgeDuplicate);
}

// One workgroup per graph, behind the rows launch (a duplicate edge is found there, row by row).
__global__ __launch_bounds__(256) void edge_finish_kernel(int B, int N, int nslab, EdgeEll ell, EdgeConv cv, EdgeRitz rz,
                                                          const int32_t* __restrict__ status) {
  const int b = blockIdx.x, t = threadIdx.x;
  const bool bad = status[b] != 0;
  const bool gated = bad || (ell.cap && ell.over[b] != 0);
  if (bad) {
    if (ell.cap) {
      for (int i = t; i < N; i += 256) ell.rowcnt[(int64_t)b * N + i] = 0;
      for (int i = t; i < nslab; i += 256) ell.widths[(int64_t)b * nslab + i] = 0;
    }
    if (cv.ent) {
      for (int i = t; i < N; i += 256) cv.counts[(int64_t)b * N + i] = 0;
      const int64_t words = (int64_t)N * cv.cap, at = (int64_t)b * words;
      for (int64_t i = t; i < words; i += 256) {
        cv.ent[at + i] = 0u;
        if (cv.vals) cv.vals[at + i] = 0.f;
      }
    }
  }
  if (rz.gate && t == 0) rz.gate[b] = gated ? 1 : 0;
  if (gated && rz.D) {
    for (int i = t; i < rz.K; i += 256) rz.D[(int64_t)b * rz.K + i] = 0.f;
    const int64_t words = (int64_t)N * rz.K, at = (int64_t)b * words;
    for (int64_t i = t; i < words; i += 256) rz.V[at + i] = 0.f;
    if (rz.info && t == 0) rz.info[b] = 0;
  }
}


// ---- typed batches: E + 1 conv images (channel 0 = every neighbour, channel 1 + e = the type-e neighbours,
// each with the diagonal and its OWN degrees: L4 of that channel's graph alone, laplacian.hip:44-79), every
// channel in ascending column order — the order the 4-byte form of sparse_image_kernel meets a row of a
// one-channel strided slice L[..., c:c+1] in.  The same four launches; next to the cursor the scatter keeps
// per-type neighbour counts (integer atomicAdd), next to a staged column its type.
constexpr int kDiagType = 15;   // (the diagonal's mark in the rows kernel's list: a member of every channel)

__global__ __launch_bounds__(256) void edge_typed_init_kernel(int B, int N, int E, int32_t* __restrict__ cursor,
                                                              int32_t* __restrict__ tcount,
                                                              int32_t* __restrict__ status,
                                                              int32_t* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < (int64_t)B * N) cursor[t] = 0;
  if (t < (int64_t)B * N * E) tcount[t] = 0;
  if (t < B) status[t] = 0;
  if (t == 0) flags[0] = 0;
}

__global__ __launch_bounds__(256) void edge_typed_scatter_kernel(EdgeBatch g, const int32_t* __restrict__ edge_type,
                                                                 int E, int scap, int32_t* __restrict__ cursor,
                                                                 int32_t* __restrict__ tcount,
                                                                 uint16_t* __restrict__ stage,
                                                                 uint8_t* __restrict__ tstage,
                                                                 int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  const int64_t lo = g.edge_off[b], hi = g.edge_off[b + 1];
  const int n = g.n_nodes[b];
  const bool bad_off = lo < 0 || hi < lo || hi > g.n_edges, bad_n = n < 0 || n > g.N;
  if (bad_off || bad_n) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
      atomicOr(status + b, (bad_off ? lnz::kEdgeOffsets : 0) | (bad_n ? lnz::kEdgeNodes : 0));
    return;
  }
  const int2* ev = reinterpret_cast<const int2*>(g.edges);
  const int64_t row0 = (int64_t)b * g.N;
  for (int64_t e = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; e < hi; e += (int64_t)gridDim.x * 256) {
    const int2 uv = ev[e];
    const int ty = edge_type[e];
    int why = 0;
    if (uv.x < 0 || uv.x >= n || uv.y < 0 || uv.y >= n) why |= lnz::kEdgeEndpoint;
    else if (uv.x == uv.y) why |= lnz::kEdgeSelfLoop;
    if (ty < 0 || ty >= E) why |= lnz::kEdgeType;
    if (why) {   // (nothing of this edge is used as an index)
      atomicOr(status + b, why);
      continue;
    }
    const int su = atomicAdd(cursor + row0 + uv.x, 1);
    if (su < scap - 1) {
      stage[(row0 + uv.x) * scap + su] = (uint16_t)uv.y;
      tstage[(row0 + uv.x) * scap + su] = (uint8_t)ty;
    }
    atomicAdd(tcount + (row0 + uv.x) * E + ty, 1);
    const int sv = atomicAdd(cursor + row0 + uv.y, 1);
    if (sv < scap - 1) {
      stage[(row0 + uv.y) * scap + sv] = (uint16_t)uv.x;
      tstage[(row0 + uv.y) * scap + sv] = (uint8_t)ty;
    }
    atomicAdd(tcount + (row0 + uv.y) * E + ty, 1);
  }
}

// One wave per row, as edge_rows_kernel: every staged entry is ranked twice in ascending column order, among
// all of the row's entries (channel 0) and among those of its own type and the diagonal (channel 1 + type);
// the diagonal's rank in channel 1 + e is the number of type-e neighbours below the row.  (scap == cv.cap)
__global__ __launch_bounds__(256) void edge_typed_rows_kernel(EdgeBatch g, int E, int scap,
                                                              const int32_t* __restrict__ cursor,
                                                              const int32_t* __restrict__ tcount,
                                                              const uint16_t* __restrict__ stage,
                                                              const uint8_t* __restrict__ tstage,
                                                              lnz::EdgeConvChannels cv, int32_t* __restrict__ status) {
  __shared__ int list[4][lnz::kEdgeMaxCap];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rid = (int64_t)blockIdx.x * 4 + wave;
  const int64_t rows = (int64_t)g.B * g.N;
  const bool valid = rid < rows;
  const int b = valid ? (int)(rid / g.N) : 0, r = valid ? (int)(rid - (int64_t)b * g.N) : 0;
  const bool live = valid && status[b] == 0 && r < g.n_nodes[b];
  const int nnb = live ? cursor[rid] : 0;
  const int m = live ? min(nnb, scap - 1) : 0;           // staged neighbours
  const int items = live ? m + 1 : 0;
  int col[4], typ[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = lane + 64 * u;
    col[u] = t < m ? (int)stage[rid * scap + t] : r;
    typ[u] = t < m ? (int)tstage[rid * scap + t] : kDiagType;
    if (t < items) list[wave][t] = col[u] | (typ[u] << 16);
  }
  __syncthreads();
  int rank0[4] = {0, 0, 0, 0}, rankt[4] = {0, 0, 0, 0};
  bool dup = false;
  for (int j = 0; j < items; ++j) {
    const int x = list[wave][j];   // (a broadcast read)
    const int xc = x & 0xffff, xt = x >> 16;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = lane + 64 * u;
      const bool less = xc < col[u] || (xc == col[u] && j < t);
      rank0[u] += less ? 1 : 0;
      rankt[u] += (less && (xt == typ[u] || xt == kDiagType)) ? 1 : 0;
      dup |= t < items && xc == col[u] && j != t;
    }
  }
  if (!valid) return;   // (no barrier below)
  // channel 0: every entry, the degrees of the simple graph
  {
    unsigned* ce = cv.ent + rid * cv.cap;
    float* cvv = cv.vals ? cv.vals + rid * cv.cap : nullptr;
    const double si = 1.0 / sqrt((double)(nnb + 1));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = lane + 64 * u;
      if (t >= items) continue;
      const int c = col[u], pos = rank0[u];
      const int dc = c == r ? nnb : cursor[(int64_t)b * g.N + c];   // (c < n_b: checked before it was staged)
      const float v = (float)((si * 1.0) * (1.0 / sqrt((double)(dc + 1))));
      if (pos < cv.cap) {
        ce[pos] = conv_entry(v, c);
        if (cvv) cvv[pos] = v;
      }
    }
    const int k = live ? nnb + 1 : 0, c = k < cv.cap ? k : cv.cap;
    conv_pad_row(ce, cvv, c, lane);
    if (lane == 0) {
      cv.counts[rid] = c;
      if (k > cv.cap) atomicOr(cv.flags, 2);
    }
  }
  // channel 1 + e: the staged type-e entries and the diagonal, the degrees of the type-e graph
  for (int e = 0; e < E; ++e) {
    int ke = live ? 1 : 0, below = 0;
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      in[u] = lane + 64 * u < m && typ[u] == e;
      ke += __popcll(__ballot(in[u]));
      below += __popcll(__ballot(in[u] && col[u] < r));
    }
    const int64_t at = ((int64_t)(1 + e) * rows + rid) * cv.cap;
    unsigned* ce = cv.ent + at;
    float* cvv = cv.vals ? cv.vals + at : nullptr;
    const int de = live ? tcount[rid * E + e] : 0;
    const double si = 1.0 / sqrt((double)(de + 1));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (!in[u]) continue;
      const int c = col[u], pos = rankt[u];
      const int dc = tcount[((int64_t)b * g.N + c) * E + e];
      const float v = (float)((si * 1.0) * (1.0 / sqrt((double)(dc + 1))));
      if (pos < cv.cap) {
        ce[pos] = conv_entry(v, c);
        if (cvv) cvv[pos] = v;
      }
    }
    if (live && lane == 0 && below < cv.cap) {   // (a live node with no type-e edge: the single entry (i, 1.0f))
      const float v = (float)((si * 1.0) * si);
      ce[below] = conv_entry(v, r);
      if (cvv) cvv[below] = v;
    }
    const int c = ke < cv.cap ? ke : cv.cap;
    conv_pad_row(ce, cvv, c, lane);
    if (lane == 0) cv.counts[(int64_t)(1 + e) * rows + rid] = c;
  }
  if (__ballot(dup) != 0ull && lane == 0) atomicOr(status + b, lnz::kEdgeDuplicate);
}

// One workgroup per (graph, channel): a graph with a non-zero status has its rows emptied in every channel.
__global__ __launch_bounds__(256) void edge_typed_finish_kernel(int B, int N, lnz::EdgeConvChannels cv,
                                                                const int32_t* __restrict__ status) {
  const int b = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  if (status[b] == 0) return;
  const int64_t row0 = ((int64_t)c * B + b) * N;
  for (int i = t; i < N; i += 256) cv.counts[row0 + i] = 0;
  const int64_t words = (int64_t)N * cv.cap, at = row0 * cv.cap;
  for (int64_t i = t; i < words; i += 256) {
    cv.ent[at + i] = 0u;
    if (cv.vals) cv.vals[at + i] = 0.f;
  }
}

}  // namespace

int64_t lnz::edge_scratch_bytes(int B, int N, int stage_cap) {
  return al256((int64_t)B * N * 4) + al256((int64_t)B * N * stage_cap * 2);
}

int lnz::edge_image_build(const char* who, const EdgeBatch& g, const EdgeEll& ell, const EdgeConv& cv,
                          const EdgeRitz& rz, void* scratch, int64_t scratch_bytes, int32_t* status,
                          hipStream_t stream) {
  LNZ_REQUIRE(g.edge_off && g.n_nodes && status && scratch && g.B > 0 && g.N > 0 && g.n_edges >= 0 &&
                  (g.edges || g.n_edges == 0),
              LNZ_EINVAL, "%s: bad arguments (edges, edge_off, n_nodes, status, workspace non-null; B=%d N=%d >= 1)", who,
              g.B, g.N);
  LNZ_REQUIRE(g.N <= kEdgeMaxN && g.B <= 65535, LNZ_ENOTSUP, "%s: N=%d <= %d nodes, B=%d <= 65535 graphs per call", who,
              g.N, kEdgeMaxN, g.B);
  LNZ_REQUIRE((reinterpret_cast<uintptr_t>(g.edges) & 7) == 0 && (reinterpret_cast<uintptr_t>(scratch) & 15) == 0,
              LNZ_EINVAL, "%s: edges must be 8-byte, the workspace 16-byte aligned", who);
  LNZ_REQUIRE(ell.cap == 0 || (ell.cap >= ELL_UNROLL && ell.cap % ELL_UNROLL == 0 && ell.cap <= kEdgeMaxCap), LNZ_EINVAL,
              "%s: row_cap=%d must be a multiple of %d in [%d, %d]", who, ell.cap, ELL_UNROLL, ELL_UNROLL, kEdgeMaxCap);
  LNZ_REQUIRE(!cv.ent || (cv.counts && cv.flags && cv.cap >= 32 && cv.cap % 8 == 0 && cv.cap <= kEdgeMaxCap), LNZ_EINVAL,
              "%s: conv image outputs (conv_row_cap=%d: a multiple of 8 in [32, %d])", who, cv.cap, kEdgeMaxCap);
  LNZ_REQUIRE(ell.cap || cv.ent, LNZ_EINVAL, "%s: no image asked for", who);
  LNZ_REQUIRE((!ell.cap || (ell.order >= 0 && ell.order <= LNZ_EDGE_ORDER_QUAD)) &&
                  (!cv.ent || (cv.order >= 0 && cv.order <= LNZ_EDGE_ORDER_QUAD)),
              LNZ_EINVAL, "%s: entry order %d / %d is not one of LNZ_EDGE_ORDER_*", who, ell.order, cv.order);
  const int scap = edge_stage_cap(ell.cap, cv.ent ? cv.cap : 0);
  LNZ_REQUIRE(scratch_bytes >= edge_scratch_bytes(g.B, g.N, scap), LNZ_EINVAL, "%s: workspace of %lld bytes, %lld needed",
              who, (long long)scratch_bytes, (long long)edge_scratch_bytes(g.B, g.N, scap));
  int32_t* cursor = (int32_t*)scratch;
  uint16_t* stage = (uint16_t*)((char*)scratch + al256((int64_t)g.B * g.N * 4));
  const int nslab = (g.N + 63) / 64;
  const int64_t rows = (int64_t)g.B * g.N;
  hipLaunchKernelGGL(edge_init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, g.B, g.N, nslab, cursor,
                     status, ell.cap ? ell.over : nullptr, ell.cap ? ell.widths : nullptr, cv.ent ? cv.flags : nullptr);
  // ~4 edges per thread on an even batch; a skewed one strides
  const int64_t chunks = std::min<int64_t>(256, std::max<int64_t>(1, (g.n_edges / g.B + 1023) / 1024));
  hipLaunchKernelGGL(edge_scatter_kernel, dim3((unsigned)chunks, (unsigned)g.B), dim3(256), 0, stream, g, scap, cursor,
                     stage, status);
  hipLaunchKernelGGL(edge_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, g, scap, cursor, stage, ell,
                     cv, status);
  hipLaunchKernelGGL(edge_finish_kernel, dim3((unsigned)g.B), dim3(256), 0, stream, g.B, g.N, nslab, ell, cv, rz, status);
  int rc = lnz::check_launch(who);
  if (rc != LNZ_OK || !ell.cap) return rc;
  hipLaunchKernelGGL(ell_pad_kernel, dim3((unsigned)(((int64_t)g.B * nslab + 3) / 4)), dim3(256), 0, stream, g.B, g.N,
                     ell.cap, ell.vals, ell.cols, ell.widths, ell.rowcnt);
  return lnz::check_launch(who);
}

// ---- the conv image alone ----------------------------------------------------------------------------
extern "C" int64_t lnz_laplacian_l4_edges_image_workspace_bytes(int B, int N, int conv_row_cap) {
  if (B <= 0 || N <= 0 || conv_row_cap <= 0) return 0;
  return lnz::edge_scratch_bytes(B, N, conv_row_cap);
}

extern "C" int lnz_laplacian_l4_edges_image(const int32_t* edges, int64_t n_edges, const int64_t* edge_off,
                                            const int32_t* n_nodes, int B, int N, void* workspace,
                                            int64_t workspace_bytes, uint32_t* conv_entries, float* conv_values,
                                            int32_t* conv_counts, int conv_row_cap, int conv_order,
                                            int32_t* conv_flags, int32_t* status, lnz_stream_t stream) {
  const char* who = "lnz_laplacian_l4_edges_image";
  LNZ_REQUIRE(conv_entries, LNZ_EINVAL, "%s: conv_entries is NULL", who);
  const EdgeBatch g{edges, n_edges, edge_off, n_nodes, B, N};
  const EdgeEll noell{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  const EdgeConv cv{conv_entries, conv_values, conv_counts, conv_flags, conv_row_cap, conv_order};
  const EdgeRitz norz{nullptr, nullptr, nullptr, 0, nullptr};
  const int rc = lnz::edge_image_build(who, g, noell, cv, norz, workspace, workspace_bytes, status, (hipStream_t)stream);
  if (rc == LNZ_OK) lnz::note_kernel("edge_rows_kernel");
  return rc;
}

// ---- the conv images of a typed batch --------------------------------------------------------------------
int64_t lnz::edge_typed_scratch_bytes(int B, int N, int E, int cap) {
  const int64_t rows = (int64_t)B * N;
  return al256(rows * 4) + al256(rows * E * 4) + al256(rows * cap * 2) + al256(rows * cap);
}

int lnz::edge_typed_image_build(const char* who, const EdgeBatch& g, const int32_t* edge_type, int E,
                                const EdgeConvChannels& cv, void* scratch, int64_t scratch_bytes, int32_t* status,
                                hipStream_t stream) {
  LNZ_REQUIRE(g.edge_off && g.n_nodes && status && scratch && g.B > 0 && g.N > 0 && g.n_edges >= 0 &&
                  ((g.edges && edge_type) || g.n_edges == 0),
              LNZ_EINVAL,
              "%s: bad arguments (edges, edge_type, edge_off, n_nodes, status, workspace non-null; B=%d N=%d >= 1)", who,
              g.B, g.N);
  LNZ_REQUIRE(E >= 2 && E <= kEdgeMaxTypes, LNZ_ENOTSUP,
              "%s: num_edge_type=%d: 2 .. %d edge types (one type: the untyped entries)", who, E, kEdgeMaxTypes);
  LNZ_REQUIRE(g.N <= kEdgeMaxN && g.B <= 65535, LNZ_ENOTSUP, "%s: N=%d <= %d nodes, B=%d <= 65535 graphs per call", who,
              g.N, kEdgeMaxN, g.B);
  LNZ_REQUIRE((reinterpret_cast<uintptr_t>(g.edges) & 7) == 0 && (reinterpret_cast<uintptr_t>(edge_type) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(scratch) & 15) == 0,
              LNZ_EINVAL, "%s: edges must be 8-byte, edge_type 4-byte, the workspace 16-byte aligned", who);
  LNZ_REQUIRE(cv.ent && cv.counts && cv.flags && cv.cap >= 32 && cv.cap % 8 == 0 && cv.cap <= kEdgeMaxCap, LNZ_EINVAL,
              "%s: conv image outputs (conv_row_cap=%d: a multiple of 8 in [32, %d])", who, cv.cap, kEdgeMaxCap);
  const int64_t need = edge_typed_scratch_bytes(g.B, g.N, E, cv.cap);
  LNZ_REQUIRE(scratch_bytes >= need, LNZ_EINVAL, "%s: workspace of %lld bytes, %lld needed", who,
              (long long)scratch_bytes, (long long)need);
  const int64_t rows = (int64_t)g.B * g.N;
  char* ws = (char*)scratch;
  int32_t* cursor = (int32_t*)ws;
  int32_t* tcount = (int32_t*)(ws + al256(rows * 4));
  uint16_t* stage = (uint16_t*)(ws + al256(rows * 4) + al256(rows * E * 4));
  uint8_t* tstage = (uint8_t*)(ws + al256(rows * 4) + al256(rows * E * 4) + al256(rows * cv.cap * 2));
  hipLaunchKernelGGL(edge_typed_init_kernel, dim3((unsigned)((rows * E + 255) / 256)), dim3(256), 0, stream, g.B, g.N, E,
                     cursor, tcount, status, cv.flags);
  const int64_t chunks = std::min<int64_t>(256, std::max<int64_t>(1, (g.n_edges / g.B + 1023) / 1024));
  hipLaunchKernelGGL(edge_typed_scatter_kernel, dim3((unsigned)chunks, (unsigned)g.B), dim3(256), 0, stream, g, edge_type,
                     E, cv.cap, cursor, tcount, stage, tstage, status);
  hipLaunchKernelGGL(edge_typed_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, g, E, cv.cap, cursor,
                     tcount, stage, tstage, cv, status);
  hipLaunchKernelGGL(edge_typed_finish_kernel, dim3((unsigned)g.B, (unsigned)(E + 1)), dim3(256), 0, stream, g.B, g.N, cv,
                     status);
  return lnz::check_launch(who);
}

extern "C" int64_t lnz_laplacian_l4_typed_edges_images_workspace_bytes(int B, int N, int num_edge_type,
                                                                       int conv_row_cap) {
  if (B <= 0 || N <= 0 || num_edge_type <= 0 || conv_row_cap <= 0) return 0;
  return lnz::edge_typed_scratch_bytes(B, N, num_edge_type, conv_row_cap);
}

extern "C" int lnz_laplacian_l4_typed_edges_images(const int32_t* edges, const int32_t* edge_type, int64_t n_edges,
                                                   const int64_t* edge_off, const int32_t* n_nodes, int B, int N,
                                                   int num_edge_type, void* workspace, int64_t workspace_bytes,
                                                   uint32_t* conv_entries, float* conv_values, int32_t* conv_counts,
                                                   int conv_row_cap, int32_t* conv_flags, int32_t* status,
                                                   lnz_stream_t stream) {
  const char* who = "lnz_laplacian_l4_typed_edges_images";
  const EdgeBatch g{edges, n_edges, edge_off, n_nodes, B, N};
  const lnz::EdgeConvChannels cv{conv_entries, conv_values, conv_counts, conv_flags, conv_row_cap};
  const int rc = lnz::edge_typed_image_build(who, g, edge_type, num_edge_type, cv, workspace, workspace_bytes, status,
                                             (hipStream_t)stream);
  if (rc == LNZ_OK) lnz::note_kernel("edge_typed_rows_kernel");
  return rc;
}
