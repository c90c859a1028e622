// Large-graph spectral convolution on the NONZEROS of the Laplacian (BASELINE.json configs[4]:
// N = 2048 nodes, batch 256, bf16 operands / fp32 accumulate — the normalised Laplacian of a
// G(n, p = 0.01) graph is 99 % zeros) — reference model/lanczos_net_general.py:157-182, the
// node-space term  sum_e L_e (X W_e^T)  of
//
//     X' = relu( sum_e L_e (X W_e^T)  +  V [ sum_s diag(g_s) (V^T X) W_s^T ]  +  b )
//
// The streamed form (csrc/conv_large.hip) reads every entry of the packed operators once per layer:
// 2.1 GB of bf16 per layer and folded channel, 0.47 ms — for products that are zero 99 times in
// 100.  Here the dense fp32 operator is read from HBM ONCE per batch,
//
//   lnz_large_sparse_image   L [B,N,N,C] (any strides) -> the nonzeros of channel 0 row by row:
//                            ent [B][N][cap] u32 = bf16(value) << 16 | column (entry k of a row, any
//                            order but a fixed one; the value rounded exactly as the streamed
//                            form's pack rounds it), counts [B][N]; every other channel is compared
//                            with channel 0 on the way (flags bit 0: differs somewhere — the caller
//                            claimed one operator class, the reference's single-edge-type collate,
//                            dataset/graph_data.py:225-262); flags bit 1: a row holds more than cap
//                            nonzeros.  Either bit sends the batch to the streamed kernels: the
//                            caller checks.
//
// and a layer is  lnz_large_gemm1_rows (Z = X W^T, bf16, row major)  +  lnz_large_spectral  +
// lnz_large_conv with C = 0 (the lift V T + bias on the matrix pipe, no activation)  +
//
//   lnz_large_sparse_conv    X[r][:] = act( X[r][:] + sum_k value[r][k] Z[column[r][k]][:] )
//
// — the streamed form's products (bf16 x bf16, fp32 accumulate) without the zeros, in entry order.
// (The same image falls out of the K-step Lanczos entry's own pass over L: lnz_lanczos_ritz_kstep_image,
// csrc/lanczos_large.hip — the collated Laplacian is then read from HBM once per batch.)
// Several DISTINCT operators (two or more edge types): one image per channel
// (lnz_large_sparse_image_channels, or csrc/edge_image.hip from typed edge lists) and the gather over all
// of them, lnz_large_sparse_conv_channels[_f32] — the same gather kernel over (row, channel) pairs.
// The image's format (entry packing, lane rank, row padding): csrc/conv_image.hpp.
#include "common.hpp"
#include "conv_image.hpp"

#include <type_traits>

namespace {

typedef unsigned short u16;
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int DH = 128;
#ifndef LNZ_SPARSE_ROWS_PER_WAVE   // (tools/experiments/build_variant.sh sweeps)
#define LNZ_SPARSE_ROWS_PER_WAVE 8
#endif
#ifndef LNZ_SPARSE_WAVES
#define LNZ_SPARSE_WAVES 4
#endif
#ifndef LNZ_SPARSE_GS
#define LNZ_SPARSE_GS 8
#endif
// A row's count is rounded up to GS (the image pads rows with zero entries up to a multiple of 8) and
// a turn of the gather is ONE uniform decision followed by a straight line of GS .. 32 loads and their
// FMAs.  With a uniform test in front of every group of GS instead (B = 256, N = 2048, 21.5 entries
// per row): GS = 8 0.275 ms; 4 0.311, 2 0.449, 1 0.700 — every test is a point the loads behind it
// wait at —; 16 0.288, 32 0.347 (padding gathers).  Straight-line turns: GS = 8 0.264, GS = 4 0.265.
constexpr int GS = LNZ_SPARSE_GS;
static_assert(GS == 4 || GS == 8, "the image pads rows to multiples of 8; a turn is at most 8 groups");
constexpr int ROWS_PER_WAVE = LNZ_SPARSE_ROWS_PER_WAVE, WAVES = LNZ_SPARSE_WAVES, TILE_ROWS = ROWS_PER_WAVE * WAVES;

constexpr int MAXR = 8;   // LARGE_MAX_OPERATORS
static_assert(ROWS_PER_WAVE * MAXR <= 64, "a wave's (row, channel) pairs: one count per lane");

// the wave's nonzeros among v (one column per lane) go behind the row's k entries, in lane order
__device__ inline void place_nonzeros(const float v, const int col, int& k, const int cap, unsigned* oe, float* ov) {
  const bool nz = v != 0.0f;   // (a NaN is kept)
  const unsigned long long m = __ballot(nz);
  if (m == 0ull) return;
  const int pos = k + lane_rank(m);
  if (nz && pos < cap) {
    oe[pos] = conv_entry(v, col);
    if (ov) ov[pos] = v;
  }
  k += __popcll(m);
}

// One row of one channel at 4-byte loads and the given column stride, ascending columns -> the row's
// number of nonzeros (those beyond cap are counted, not kept).  COMPARE: channels 1 .. nchk - 1 (sch
// apart) are read next to it and `differ` is raised in a lane that saw one differ from this channel.
template <bool COMPARE>
__device__ inline int strided_row_scan(const float* Lr, const int64_t sc, const int64_t sch, const int nchk,
                                       const int N, const int cap, unsigned* oe, float* ov, bool& differ) {
  const int lane = threadIdx.x & 63;
  int k = 0;   // entries of this row so far (wave-uniform)
  for (int c0 = 0; c0 < N; c0 += 64 * 8) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int col = c0 + 64 * u + lane;
      x[u] = col < N ? Lr[(int64_t)col * sc] : 0.0f;
    }
    if constexpr (COMPARE) {
      for (int c = 1; c < nchk; ++c) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int col = c0 + 64 * u + lane;
          const float y = col < N ? Lr[(int64_t)col * sc + (int64_t)c * sch] : 0.0f;
          differ |= x[u] != y;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) place_nonzeros(x[u], c0 + 64 * u + lane, k, cap, oe, ov);
  }
  return k;
}

// ---- image: one wavefront per row ---------------------------------------------------------------
// FORM 2: channels-last pair of channels (sc == 2, sch == 1, rows 16-byte aligned): a float4 is two
// columns x two channels, 1 KiB contiguous per wave load, eight loads in flight.  FORM 1: one
// operator in contiguous rows (sc == 1 and a single channel or a zero channel stride — an expanded
// view): a float4 is four columns.  FORM 0: 4-byte loads at the given strides.
template <int FORM>
__global__ __launch_bounds__(256) void sparse_image_kernel(
    const float* __restrict__ L, int64_t sb, int64_t sr, int64_t sc, int64_t sch, int B, int N, int C,
    int cap, unsigned* __restrict__ ent, float* __restrict__ vals, int32_t* __restrict__ counts,
    int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t rid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (rid >= (int64_t)B * N) return;
  const int b = (int)(rid / N), r = (int)(rid - (int64_t)b * N);
  const float* Lr = L + (int64_t)b * sb + (int64_t)r * sr;
  unsigned* oe = ent + rid * cap;
  float* ov = vals ? vals + rid * cap : nullptr;   // (the exact-fp32 form's values, optional)
  int k = 0;            // entries of this row so far (wave-uniform)
  bool differ = false;  // a channel differs from channel 0 in this lane's columns
  auto place = [&](const float v, const int col) { place_nonzeros(v, col, k, cap, oe, ov); };
  if constexpr (FORM == 1) {
    const f32x4* src = reinterpret_cast<const f32x4*>(Lr);
    const int nq = N >> 2;   // (N is a multiple of 4 in this form)
    for (int q0 = 0; q0 < nq; q0 += 64 * 8) {
      f32x4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = q0 + 64 * u + lane;
        x[u] = q < nq ? __builtin_nontemporal_load(src + q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = q0 + 64 * u + lane;
        if (__ballot((x[u][0] != 0.0f) | (x[u][1] != 0.0f) | (x[u][2] != 0.0f) | (x[u][3] != 0.0f)) == 0ull)
          continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) place(x[u][c], 4 * q + c);
      }
    }
  } else if constexpr (FORM == 2) {
    const f32x4* src = reinterpret_cast<const f32x4*>(Lr);
    const int nq = N >> 1;   // float4 = columns 2 q, 2 q + 1 (N is even in this form)
    for (int q0 = 0; q0 < nq; q0 += 64 * 8) {
      f32x4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = q0 + 64 * u + lane;
        x[u] = q < nq ? __builtin_nontemporal_load(src + q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = q0 + 64 * u + lane;
        differ |= (x[u][0] != x[u][1]) | (x[u][2] != x[u][3]);
        if (__ballot((x[u][0] != 0.0f) | (x[u][2] != 0.0f)) == 0ull) continue;
        place(x[u][0], 2 * q);
        place(x[u][2], 2 * q + 1);
      }
    }
  } else {
    const int nchk = sch == 0 ? 1 : C;   // (a zero channel stride: one operator by construction)
    k = strided_row_scan<true>(Lr, sc, sch, nchk, N, cap, oe, ov, differ);
  }
  const int cnt = k < cap ? k : cap;
  conv_pad_row(oe, ov, cnt, lane);
  const bool any_differ = __ballot(differ) != 0ull;
  if (lane == 0) {
    counts[rid] = cnt;
    const int f = (any_differ ? 1 : 0) | (k > cap ? 2 : 0);
    if (f) atomicOr(flags, f);
  }
}

// ---- images of all C channels in ONE pass over L (several DISTINCT operators: a typed batch, channel 0 =
// the simple graph, channel 1 + e = edge type e alone, dataset/get_graph_data.py:60-72): one wave per row,
// ascending columns, 4-byte loads at the given strides (the channels of a column sit next to each other:
// every line of the row is fetched from HBM once and serves all channels).  Image c [c][B][N][cap] is, bit
// for bit, what sparse_image_kernel<0> writes for the one-channel slice L[..., c:c+1] — the same row scan,
// without the compare; flags: bit 1 only.
__global__ __launch_bounds__(256) void sparse_image_channels_kernel(
    const float* __restrict__ L, int64_t sb, int64_t sr, int64_t sc, int64_t sch, int B, int N, int C,
    int cap, unsigned* __restrict__ ent, float* __restrict__ vals, int32_t* __restrict__ counts,
    int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = (int64_t)B * N;
  const int64_t rid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (rid >= rows) return;
  const int b = (int)(rid / N), r = (int)(rid - (int64_t)b * N);
  const float* Lr = L + (int64_t)b * sb + (int64_t)r * sr;
  bool over = false, differ = false;   // (differ: never raised here)
  for (int c = 0; c < C; ++c) {
    unsigned* oe = ent + ((int64_t)c * rows + rid) * cap;
    float* ov = vals ? vals + ((int64_t)c * rows + rid) * cap : nullptr;
    const int k = strided_row_scan<false>(Lr + (int64_t)c * sch, sc, 0, 1, N, cap, oe, ov, differ);
    const int cnt = k < cap ? k : cap;
    conv_pad_row(oe, ov, cnt, lane);
    if (lane == 0) counts[(int64_t)c * rows + rid] = cnt;
    over |= k > cap;
  }
  if (lane == 0 && over) atomicOr(flags, 2);
}

// ---- conv: X[r][:] = act( X[r][:] + sum_c sum_k value_c[r][k] Z_c[column_c[r][k]][:] ), R = 1 .. 8 ----
// (the node-space term sum_c L_c (X W_c^T) of model/lanczos_net_general.py:179; R = 1: one operator)
// Workgroup = 32 rows of one graph (4 waves x 8 rows: 0.276 ms; x 16: 0.288, x 32: 0.340 — fewer
// graphs share an L2 at a time); blockIdx -> (graph, tile) deals the tiles
// of a graph to ONE XCD (workgroup i runs on XCD i % 8), whose L2 then holds the graph's Z (512
// KiB).  One row at a time per wave, lanes along the 128 features (one dword = two bf16 features per
// lane and entry: every gather is the 256 contiguous bytes of one node, its offset in an SGPR of a
// buffer load — no vector address arithmetic), the row's entries one coalesced load (lane k <-
// entry k, requested one row ahead) and broadcast by v_readlane; up to 32 gathers go out before the
// first is used.  The launch moves 256 B through the L2 -> L1 path per nonzero: 3.5 GB per layer at
// config 5 = 0.28 ms at ~12 TB/s, and that path is what bounds it (measured: 7 -> 4 vector
// instructions per entry and 8 -> 32 gathers in flight changed nothing; a form with a feature
// quarter of Z staged in LDS and ds_bpermute broadcasts was issue bound at 0.32 ms; the lift V T in
// vector FMAs inside this kernel, T in LDS, cost 0.25 ms against the 0.08 ms of the MFMA launch).
//
// What differs between the two element types of the gather, and nothing else:
//   GatherBf16  the value rides in the entry (bf16(value) << 16 | column), Z [..][N][128] bf16: a lane's
//               dword = features 2 lane, 2 lane + 1; counts rounded up to GS, turns of GS .. 32 entries.
//   GatherF32   the split-precision modes' node-space term in EXACT fp32: the unrounded values beside the
//               entries, Zf [..][N][128] fp32 (= lnz_f32_linear's X W^T): a lane's dwordx2, 512 B through
//               the L2 -> L1 path per nonzero (twice the bf16 form's), no unpacking; counts rounded up to
//               8 (whatever GS is), turns of 8 or 16 entries.
// A turn is ONE uniform decision followed by a straight line of gathers and their FMAs (a test per group
// of eight was a point the loads behind it waited at).
struct GatherBf16 {
  typedef u16 T;
  struct Entry { unsigned e; };
  static constexpr int TURN = 32;
  static __device__ __forceinline__ int round_up(const int cnt) { return (cnt + GS - 1) & ~(GS - 1); }
  static __device__ __forceinline__ Entry load(const unsigned* ent, const float*, const int64_t o, const bool in) {
    return Entry{in ? ent[o] : 0u};
  }
  template <int n>
  static __device__ __forceinline__ void turn(const __amdgpu_buffer_rsrc_t z, const unsigned zoff, const Entry en,
                                              const int k, f32x2& acc) {
    unsigned g[n];
    float s[n];
#pragma unroll
    for (int u = 0; u < n; ++u) {
      const unsigned se = (unsigned)__builtin_amdgcn_readlane((int)en.e, k + u);
      s[u] = __uint_as_float(se & 0xffff0000u);
      g[u] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(z, zoff, (se & 0xffffu) * (DH * 2), 0);
    }
#pragma unroll
    for (int u = 0; u < n; ++u) {
      acc[0] = fmaf(s[u], __uint_as_float(g[u] << 16), acc[0]);
      acc[1] = fmaf(s[u], __uint_as_float(g[u] & 0xffff0000u), acc[1]);
    }
  }
  // entries k .. of the lanes' `left` (> 0, a multiple of GS), TURN of them at most
  static __device__ __forceinline__ void turns(const __amdgpu_buffer_rsrc_t z, const unsigned zoff, const Entry en,
                                               const int k, const int left, f32x2& acc) {
    switch (min(32, left) / GS) {
#define LNZ_TURN(q) case q: if constexpr (q * GS <= 32) turn<(q * GS <= 32 ? q * GS : 32)>(z, zoff, en, k, acc); break;
      LNZ_TURN(1) LNZ_TURN(2) LNZ_TURN(3) LNZ_TURN(4) LNZ_TURN(5) LNZ_TURN(6) LNZ_TURN(7) LNZ_TURN(8)
#undef LNZ_TURN
      default: break;
    }
  }
};

struct GatherF32 {
  typedef float T;
  struct Entry { unsigned e; float v; };
  static constexpr int TURN = 16;
  static __device__ __forceinline__ int round_up(const int cnt) { return (cnt + 7) & ~7; }
  static __device__ __forceinline__ Entry load(const unsigned* ent, const float* vals, const int64_t o, const bool in) {
    Entry en = {0u, 0.0f};
    if (in) {   // (both loads behind ONE test)
      en.e = ent[o];
      en.v = vals[o];
    }
    return en;
  }
  template <int n>
  static __device__ __forceinline__ void turn(const __amdgpu_buffer_rsrc_t z, const unsigned zoff, const Entry en,
                                              const int k, f32x2& acc) {
    f32x2 g[n];
    float s[n];
#pragma unroll
    for (int u = 0; u < n; ++u) {
      const unsigned col = (unsigned)__builtin_amdgcn_readlane((int)en.e, k + u) & 0xffffu;
      s[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(en.v), k + u));
      g[u] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(z, zoff, col * (DH * 4), 0));
    }
#pragma unroll
    for (int u = 0; u < n; ++u) {
      acc[0] = fmaf(s[u], g[u][0], acc[0]);
      acc[1] = fmaf(s[u], g[u][1], acc[1]);
    }
  }
  static __device__ __forceinline__ void turns(const __amdgpu_buffer_rsrc_t z, const unsigned zoff, const Entry en,
                                               const int k, const int left, f32x2& acc) {
    if (left > 8) turn<16>(z, zoff, en, k, acc);
    else turn<8>(z, zoff, en, k, acc);
  }
};

// The schedule, once: the (row, channel) pairs of a wave's eight rows are its sequence — lane q = R rr + c
// holds the count of pair q (at most 64 pairs), the entries of pair q + 1 are requested while pair q is
// gathered, channels ascending and entries in entry order into ONE accumulator per row (X read at c == 0,
// written behind the last channel): the result is a fixed function of the images.  Images [R][B][N][cap],
// counts [R][B][N], Z CLASS MAJOR [R][B][N][128] (one GEMM1 per channel): a graph's R feature blocks are R
// buffers of N rows, the descriptor rebuilt per pair from scalars.  MULTI = false: R = 1 at compile time
// — the pairs are the rows, the channel and the per-pair descriptor fold away.
// SPLIT (the backward's dZ_c = L_c dP, csrc/conv_sparse_grad.hip): the same pairs over ONE source — every
// channel reads the graph's Z [B][N][128] — and one result per pair: the accumulator starts at zero and is
// stored into channel c's block of X [R][B][N][128] behind the pair's own entries (X is written, never
// read; no activation).  Channel c's block is, bit for bit, the R = 1 gather of image c onto zeros.
template <class Elem, bool MULTI, bool SPLIT = false>
__global__ __launch_bounds__(64 * WAVES) void sparse_gather_kernel(
    const unsigned* __restrict__ ent, const float* __restrict__ vals, const int32_t* __restrict__ counts,
    int cap, const typename Elem::T* __restrict__ Z, int B, int N, int operators, int tiles, int relu,
    float* __restrict__ X) {
  typedef typename Elem::T T;
  typedef typename Elem::Entry Entry;
  const int R = MULTI ? operators : 1;
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int b = xcd + 8 * (seq / tiles), tile = seq % tiles;
  if (b >= B) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r0 = tile * TILE_ROWS + wave * ROWS_PER_WAVE;
  if (r0 >= N) return;
  const int nr = min(ROWS_PER_WAVE, N - r0), nq = nr * R;   // (ROWS_PER_WAVE * MAXR <= 64)
  const int64_t rows = (int64_t)B * N, row0 = (int64_t)b * N + r0;
  const int cv = lane < nq ? counts[(int64_t)(lane % R) * rows + row0 + lane / R] : 0;
  // the graph's Z as a buffer: a lane's two features of a node's 128
  const T* Zb = Z + (int64_t)b * N * DH;
  const unsigned zoff = (unsigned)(2 * sizeof(T)) * lane;
  auto entries = [&](const int rr, const int c, const int k0, const int cnt8) -> Entry {
    return Elem::load(ent, vals, ((int64_t)c * rows + row0 + rr) * cap + k0 + lane, k0 + lane < cnt8);
  };
  int cnt8n = Elem::round_up(__builtin_amdgcn_readlane(cv, 0));
  Entry en = entries(0, 0, 0, cnt8n);
  f32x2 acc = {0.0f, 0.0f};
  int rr = 0, c = 0;
  for (int q = 0; q < nq; ++q) {
    const int cnt8 = cnt8n;
    Entry e = en;
    float* xr = X + ((SPLIT ? (int64_t)c * rows : 0) + row0 + rr) * DH + 2 * lane;
    if constexpr (SPLIT) acc = f32x2{0.0f, 0.0f};
    else if (c == 0) acc = *reinterpret_cast<const f32x2*>(xr);
    const int cn = c + 1 < R ? c + 1 : 0, rn = c + 1 < R ? rr : rr + 1;
    if (q + 1 < nq) {   // (uniform) the next pair's entries
      cnt8n = Elem::round_up(__builtin_amdgcn_readlane(cv, q + 1));
      en = entries(rn, cn, 0, cnt8n);
    }
    const __amdgpu_buffer_rsrc_t z_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(Zb + (SPLIT ? 0 : (int64_t)c * rows * DH)), 0, (unsigned)N * DH * (unsigned)sizeof(T), 0x00020000);
    for (int k0 = 0; k0 < cnt8; k0 += 64) {
      if (k0 > 0) e = entries(rr, c, k0, cnt8);   // (rows of more than 64 entries)
      const int m = min(64, cnt8 - k0);
      for (int k = 0; k < m; k += Elem::TURN) Elem::turns(z_rsrc, zoff, e, k, m - k, acc);
    }
    if (SPLIT || cn == 0) {   // the row's last channel (SPLIT: every pair)
      if (!SPLIT && relu) {
        acc[0] = acc[0] > 0.0f ? acc[0] : 0.0f;
        acc[1] = acc[1] > 0.0f ? acc[1] : 0.0f;
      }
      *reinterpret_cast<f32x2*>(xr) = acc;
    }
    rr = rn;
    c = cn;
  }
}

// The gather entries: `who` = the entry's name, whose kernel is named after it (lnz_last_kernel():
// sparse_conv[_channels | _split][_f32]_kernel).  MULTI: R = 2 .. MAXR operators; otherwise R = 1.  SPLIT: Z is
// the one source [B][N][128], X the R results [R][B][N][128].
template <class Elem, bool MULTI, bool SPLIT = false>
int launch_gather(const char* who, const uint32_t* entries, const float* values, const int32_t* counts, int row_cap,
                  const typename Elem::T* Z, int B, int N, int R, int relu, float* X, lnz_stream_t stream) {
  constexpr bool F32 = std::is_same<Elem, GatherF32>::value;
  LNZ_REQUIRE(entries && (values || !F32) && counts && Z && X && B > 0 && N > 0, LNZ_EINVAL, "%s: bad arguments", who);
  if (SPLIT) LNZ_REQUIRE((const void*)Z != (const void*)X, LNZ_EINVAL, "%s: the results must not alias the source", who);
  if (MULTI)
    LNZ_REQUIRE(R >= 2 && R <= MAXR, LNZ_ENOTSUP, "%s: R=%d: 2 .. %d operators (one: lnz_large_sparse_conv%s)", who, R,
                MAXR, F32 ? "_f32" : "");
  if (MULTI && !F32) LNZ_REQUIRE(N <= 65536, LNZ_ENOTSUP, "%s: N=%d > 65536 (16-bit columns)", who, N);
  LNZ_REQUIRE(row_cap >= 32 && row_cap % 8 == 0, LNZ_EINVAL, "%s: row_cap=%d must be a multiple of 8, at least 32", who,
              row_cap);
  if (F32) {
    LNZ_REQUIRE((((uintptr_t)X) & 7) == 0 && (((uintptr_t)Z) & 7) == 0, LNZ_EINVAL,
                "%s: X / Zf must be 8-byte aligned", who);
    if (MULTI)
      LNZ_REQUIRE(N <= 65536 && (int64_t)N * DH * 4 <= 0x7fffffffll, LNZ_ENOTSUP, "%s: N=%d too large", who, N);
    else
      LNZ_REQUIRE((int64_t)N * DH * 4 <= 0x7fffffffll, LNZ_ENOTSUP, "%s: N too large", who);
  } else if (MULTI) {
    LNZ_REQUIRE((((uintptr_t)X) & 7) == 0 && (((uintptr_t)Z) & 3) == 0, LNZ_EINVAL,
                "%s: X must be 8-byte, Z 4-byte aligned", who);
  } else {
    LNZ_REQUIRE((((uintptr_t)X) & 7) == 0, LNZ_EINVAL, "%s: X must be 8-byte aligned", who);
  }
  const int tiles = (N + TILE_ROWS - 1) / TILE_ROWS;
  const int64_t grid = (int64_t)8 * tiles * ((B + 7) / 8);
  LNZ_REQUIRE(grid <= 0x7fffffffll, LNZ_ENOTSUP, "%s: B x N too large", who);
  hipLaunchKernelGGL((sparse_gather_kernel<Elem, MULTI, SPLIT>), dim3((unsigned)grid), dim3(64 * WAVES), 0,
                     (hipStream_t)stream, entries, values, counts, row_cap, Z, B, N, R, tiles, relu, X);
  lnz::note_kernel("%s_kernel", who + sizeof("lnz_large_") - 1);
  return lnz::check_launch(who);
}

}  // namespace

extern "C" int lnz_large_sparse_image(const float* L, int64_t stride_b, int64_t stride_r,
                                      int64_t stride_c, int64_t stride_ch, int B, int N, int C,
                                      int row_cap, uint32_t* entries, float* values,
                                      int32_t* counts, int32_t* flags, lnz_stream_t stream) {
  LNZ_REQUIRE(L && entries && counts && flags && B > 0 && N > 0 && C > 0, LNZ_EINVAL,
              "lnz_large_sparse_image: bad arguments (B=%d N=%d C=%d)", B, N, C);
  LNZ_REQUIRE(N <= 65536, LNZ_ENOTSUP, "lnz_large_sparse_image: N=%d > 65536 (16-bit columns)", N);
  LNZ_REQUIRE(row_cap >= 32 && row_cap % 8 == 0, LNZ_EINVAL,
              "lnz_large_sparse_image: row_cap=%d must be a multiple of 8, at least 32", row_cap);
  const int64_t rows = (int64_t)B * N;
  LNZ_REQUIRE((rows + 3) / 4 <= 0x7fffffffll, LNZ_ENOTSUP, "lnz_large_sparse_image: B x N too large");
  hipStream_t s = (hipStream_t)stream;
  LNZ_REQUIRE(hipMemsetAsync(flags, 0, sizeof(int32_t), s) == hipSuccess, LNZ_ELAUNCH,
              "lnz_large_sparse_image: hipMemsetAsync failed");
  const bool aligned = (((uintptr_t)L) & 15) == 0 && stride_b % 4 == 0 && stride_r % 4 == 0;
  const bool pair = aligned && C == 2 && stride_c == 2 && stride_ch == 1 && N % 2 == 0;
  const bool rows1 = aligned && stride_c == 1 && (C == 1 || stride_ch == 0) && N % 4 == 0;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (pair)
    hipLaunchKernelGGL(sparse_image_kernel<2>, grid, dim3(256), 0, s, L, stride_b, stride_r,
                       stride_c, stride_ch, B, N, C, row_cap, entries, values, counts, flags);
  else if (rows1)
    hipLaunchKernelGGL(sparse_image_kernel<1>, grid, dim3(256), 0, s, L, stride_b, stride_r,
                       stride_c, stride_ch, B, N, C, row_cap, entries, values, counts, flags);
  else
    hipLaunchKernelGGL(sparse_image_kernel<0>, grid, dim3(256), 0, s, L, stride_b, stride_r,
                       stride_c, stride_ch, B, N, C, row_cap, entries, values, counts, flags);
  lnz::note_kernel("sparse_image_kernel<%s>", pair ? "pair" : rows1 ? "rows" : "strided");
  return lnz::check_launch("lnz_large_sparse_image");
}

extern "C" int lnz_large_sparse_image_channels(const float* L, int64_t stride_b, int64_t stride_r,
                                               int64_t stride_c, int64_t stride_ch, int B, int N, int C,
                                               int row_cap, uint32_t* entries, float* values,
                                               int32_t* counts, int32_t* flags, lnz_stream_t stream) {
  LNZ_REQUIRE(L && entries && counts && flags && B > 0 && N > 0 && C > 0, LNZ_EINVAL,
              "lnz_large_sparse_image_channels: bad arguments (B=%d N=%d C=%d)", B, N, C);
  LNZ_REQUIRE(C <= MAXR, LNZ_ENOTSUP, "lnz_large_sparse_image_channels: C=%d > %d operator channels", C, MAXR);
  LNZ_REQUIRE(N <= 65536, LNZ_ENOTSUP, "lnz_large_sparse_image_channels: N=%d > 65536 (16-bit columns)", N);
  LNZ_REQUIRE(row_cap >= 32 && row_cap % 8 == 0, LNZ_EINVAL,
              "lnz_large_sparse_image_channels: row_cap=%d must be a multiple of 8, at least 32", row_cap);
  const int64_t rows = (int64_t)B * N;
  LNZ_REQUIRE((rows + 3) / 4 <= 0x7fffffffll, LNZ_ENOTSUP, "lnz_large_sparse_image_channels: B x N too large");
  hipStream_t s = (hipStream_t)stream;
  LNZ_REQUIRE(hipMemsetAsync(flags, 0, sizeof(int32_t), s) == hipSuccess, LNZ_ELAUNCH,
              "lnz_large_sparse_image_channels: hipMemsetAsync failed");
  hipLaunchKernelGGL(sparse_image_channels_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, L, stride_b,
                     stride_r, stride_c, stride_ch, B, N, C, row_cap, entries, values, counts, flags);
  lnz::note_kernel("sparse_image_channels_kernel");
  return lnz::check_launch("lnz_large_sparse_image_channels");
}

extern "C" int lnz_large_sparse_conv(const uint32_t* entries, const int32_t* counts, int row_cap,
                                     const uint16_t* Z, int B, int N, int relu, float* X,
                                     lnz_stream_t stream) {
  return launch_gather<GatherBf16, false>("lnz_large_sparse_conv", entries, nullptr, counts, row_cap, Z, B, N, 1, relu,
                                          X, stream);
}

extern "C" int lnz_large_sparse_conv_f32(const uint32_t* entries, const float* values,
                                         const int32_t* counts, int row_cap, const float* Zf, int B,
                                         int N, int relu, float* X, lnz_stream_t stream) {
  return launch_gather<GatherF32, false>("lnz_large_sparse_conv_f32", entries, values, counts, row_cap, Zf, B, N, 1,
                                         relu, X, stream);
}

extern "C" int lnz_large_sparse_conv_channels(const uint32_t* entries, const int32_t* counts, int row_cap,
                                              const uint16_t* Z, int B, int N, int R, int relu, float* X,
                                              lnz_stream_t stream) {
  return launch_gather<GatherBf16, true>("lnz_large_sparse_conv_channels", entries, nullptr, counts, row_cap, Z, B, N,
                                         R, relu, X, stream);
}

extern "C" int lnz_large_sparse_conv_channels_f32(const uint32_t* entries, const float* values,
                                                  const int32_t* counts, int row_cap, const float* Zf, int B,
                                                  int N, int R, int relu, float* X, lnz_stream_t stream) {
  return launch_gather<GatherF32, true>("lnz_large_sparse_conv_channels_f32", entries, values, counts, row_cap, Zf, B,
                                        N, R, relu, X, stream);
}

extern "C" int lnz_large_sparse_conv_split_f32(const uint32_t* entries, const float* values,
                                               const int32_t* counts, int row_cap, const float* P, int B,
                                               int N, int R, float* dZ, lnz_stream_t stream) {
  return launch_gather<GatherF32, true, true>("lnz_large_sparse_conv_split_f32", entries, values, counts, row_cap, P, B,
                                              N, R, 0, dZ, stream);
}
