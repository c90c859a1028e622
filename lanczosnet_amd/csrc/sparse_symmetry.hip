// Is the operator of a sparse image symmetric?  (`_dense_symmetric_operators`, model/_large.py)
//
// The backward of the sparse large-graph layer (csrc/conv_sparse_grad.hip) forms dZ = L dP where the maths asks
// for L^T dP.  An image built from an edge list is symmetric by construction; an image built from a tensor a
// caller handed in (lnz_large_sparse_image[_channels], the K-step compaction pass) is whatever the tensor was.
//
//   lnz_large_sparse_image_symmetry   status[r B + b], one word per graph and channel, cleared by the call:
//       bit 0  some entry (i, j, v), k < counts[i], has no entry with column i among the first counts[j]
//              entries of row j;
//       bit 1  the mirror is there and its value is not v: the two match when they have the same sign and their
//              bit patterns, as integers, differ by at most one — one fp32 ulp.  (The reference builds L in
//              float64 and casts: (s_i a) s_j and (s_j a) s_i can round one ulp apart.)
//
// The rows' padding (column 0, value 0 up to a multiple of eight: csrc/conv_image.hpp) is not an entry; a
// diagonal entry is its own mirror.  Entry order within a row is the image kernel's, not ascending (pair or
// quad order by N's parity): the mirror is SEARCHED, not bisected.  Counts are clamped to [0, row_cap] and a
// column at or beyond N is reported as a missing mirror, never followed: the launch is safe on an image
// whose flags are raised (its result is then meaningless), so a caller reads flags and status in one wait.
//
// One wavefront per image row (r, b, i).  The row's entries arrive in one coalesced load; then, eight entries
// at a time (their loads in flight together): the 64 lanes read the first 64 columns of row j out of L2, a
// ballot finds the mirror, and the mirror's value word is fetched and compared.  Rows longer than 64 entries
// (row_cap > 64: N > 2048) go on 64 columns at a time for the entries not found yet.
// The status words: a wave that found a defect ORs its bits into the graph's word with one vector atomic from
// one lane.  An integer OR gives the same word in any order — two calls give the same bits — and a clean image,
// the case that matters, issues none.  (Plain stores would need a word per bit; the interface has one.)
#include "common.hpp"

namespace {

constexpr int GROUP = 8;    // entries whose row reads are in flight together (rows are padded to multiples of 8)
constexpr int MAXR = 8;     // LARGE_MAX_OPERATORS

__device__ inline bool within_one_ulp(unsigned a, unsigned b) {
  if ((a ^ b) >> 31) return false;
  const int d = (int)(a & 0x7fffffffu) - (int)(b & 0x7fffffffu);
  return d >= -1 && d <= 1;
}

__global__ __launch_bounds__(256) void sparse_image_symmetry_kernel(
    const unsigned* __restrict__ ent, const float* __restrict__ vals, const int32_t* __restrict__ counts,
    int cap, int64_t rows, int N, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int64_t rid = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (rid >= rows) return;
  const int64_t rb = rid / N;                 // r B + b
  const int i = (int)(rid - rb * N);
  const int64_t g0 = rb * N;                  // the graph's first image row
  const int cnt = __builtin_amdgcn_readfirstlane(min(max(counts[rid], 0), cap));
  const unsigned* erow = ent + rid * cap;
  const unsigned* vrow = reinterpret_cast<const unsigned*>(vals) + rid * cap;
  int st = 0;                                 // (wave-uniform)
  for (int k0 = 0; k0 < cnt; k0 += 64) {
    const bool live = k0 + lane < cnt;
    const unsigned e = live ? erow[k0 + lane] : 0u;
    const unsigned vb = live ? vrow[k0 + lane] : 0u;
    const int m = min(64, cnt - k0);
    for (int g = 0; g < m; g += GROUP) {
      int j[GROUP], cj[GROUP];
      unsigned ej[GROUP], mv[GROUP];
      int pos[GROUP];
      // (lanes g .. g + 7 exist: g < m <= 64, g a multiple of 8; those at or beyond m hold column 0)
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        j[u] = (int)(__builtin_amdgcn_readlane(e, g + u) & 0xffffu);
        const int jr = j[u] < N ? j[u] : 0;
        cj[u] = min(max(counts[g0 + jr], 0), cap);
      }
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        const int jr = j[u] < N ? j[u] : 0;
        ej[u] = lane < cj[u] ? ent[(g0 + jr) * cap + lane] : 0u;
      }
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        const int jr = j[u] < N ? j[u] : 0;
        unsigned long long hit = __ballot(lane < cj[u] && (int)(ej[u] & 0xffffu) == i);
        int base = 0;
        for (int t0 = 64; hit == 0ull && t0 < cj[u]; t0 += 64) {   // (row_cap > 64 only)
          const unsigned x = t0 + lane < cj[u] ? ent[(g0 + jr) * cap + t0 + lane] : 0u;
          hit = __ballot(t0 + lane < cj[u] && (int)(x & 0xffffu) == i);
          base = t0;
        }
        pos[u] = hit ? base + (int)__builtin_ctzll(hit) : -1;
        // (pos < cj <= cap: inside row j)
        mv[u] = pos[u] >= 0 ? reinterpret_cast<const unsigned*>(vals)[(g0 + jr) * cap + pos[u]] : 0u;
      }
#pragma unroll
      for (int u = 0; u < GROUP; ++u) {
        if (g + u >= m || j[u] == i) continue;          // padding; the diagonal
        if (j[u] >= N || pos[u] < 0)
          st |= 1;
        else if (!within_one_ulp(__builtin_amdgcn_readlane(vb, g + u), mv[u]))
          st |= 2;
      }
    }
  }
  if (st != 0 && lane == 0) atomicOr(status + rb, st);
}

}  // namespace

extern "C" int lnz_large_sparse_image_symmetry(const uint32_t* entries, const float* values,
                                               const int32_t* counts, int row_cap, int R, int B, int N,
                                               int32_t* status, lnz_stream_t stream) {
  const char* who = "lnz_large_sparse_image_symmetry";
  LNZ_REQUIRE(entries && values && counts && status && R > 0 && B > 0 && N > 0, LNZ_EINVAL,
              "%s: bad arguments (R=%d B=%d N=%d; the image's values are required)", who, R, B, N);
  LNZ_REQUIRE(R <= MAXR, LNZ_ENOTSUP, "%s: R=%d > %d operator channels", who, R, MAXR);
  LNZ_REQUIRE(N <= 65536, LNZ_ENOTSUP, "%s: N=%d > 65536 (16-bit columns)", who, N);
  LNZ_REQUIRE(row_cap >= 32 && row_cap % 8 == 0, LNZ_EINVAL, "%s: row_cap=%d must be a multiple of 8, at least 32",
              who, row_cap);
  const int64_t rows = (int64_t)R * B * N;
  LNZ_REQUIRE((rows + 3) / 4 <= 0x7fffffffll, LNZ_ENOTSUP, "%s: R x B x N too large", who);
  hipStream_t s = (hipStream_t)stream;
  LNZ_REQUIRE(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)R * B, s) == hipSuccess, LNZ_ELAUNCH,
              "%s: hipMemsetAsync failed", who);
  hipLaunchKernelGGL(sparse_image_symmetry_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, entries, values,
                     counts, row_cap, rows, N, status);
  lnz::note_kernel("sparse_image_symmetry_kernel");
  return lnz::check_launch(who);
}
