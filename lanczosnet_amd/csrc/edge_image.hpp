// The images of the large-graph path built from a batch of EDGE LISTS (csrc/edge_image.hip): what
// ell_compact_rows_kernel + ell_pad_kernel (csrc/ell_image.hpp) gather from the dense collated
// Laplacian, with no N x N array anywhere.  Shared by the K-step entries that run on the images
// (csrc/lanczos_large.hip, csrc/lanczos_wide.hip).
#pragma once
#include "common.hpp"

namespace lnz {

// reasons a graph's `status` word collects (bits; 0 = the graph is fine)
constexpr int kEdgeEndpoint = 1;    // an endpoint outside [0, n_b)
constexpr int kEdgeSelfLoop = 2;    // an edge (i, i)
constexpr int kEdgeDuplicate = 4;   // an edge listed twice (either orientation)
constexpr int kEdgeOffsets = 8;     // edge_off[b] .. edge_off[b + 1] is not a range inside the edge array
constexpr int kEdgeNodes = 16;      // n_nodes[b] outside [0, N]
constexpr int kEdgeType = 32;       // (typed batches) an edge type outside [0, E)
constexpr int kEdgeMaxCap = 256;    // row capacities served (a wave ranks 4 entries per lane)
constexpr int kEdgeMaxN = 16384;

struct EdgeBatch {
  const int32_t* edges;      // [n_edges][2] local node ids, each undirected edge once
  int64_t n_edges;
  const int64_t* edge_off;   // [B + 1]
  const int32_t* n_nodes;    // [B]
  int B, N;
};
struct EdgeEll {             // the sliced-ELL image of the K-step recurrence (cap = 0: not wanted)
  float* vals;
  uint16_t* cols;
  int32_t* widths;
  int32_t* rowcnt;
  int32_t* over;             // [B] a row of this graph holds more than `cap` entries
  int cap;
  int order;                 // LNZ_EDGE_ORDER_*: the entry order within a row
};
struct EdgeConv {            // the row-major conv image (ent = NULL: not wanted)
  uint32_t* ent;
  float* vals;               // optional
  int32_t* counts;
  int32_t* flags;            // one word: bit 1 = a row beyond `cap`
  int cap;
  int order;                 // LNZ_EDGE_ORDER_*
};
struct EdgeRitz {            // the outputs of the Ritz launch behind the build (D = NULL: none)
  float* D;
  float* V;
  int32_t* info;             // optional
  int K;
  int32_t* gate;             // [B] out: over[b] | (status[b] != 0) — such a graph's D, V, info are zeroed here
};

// cursor [B][N] int32 + staged columns [B][N][stage_cap] u16
int64_t edge_scratch_bytes(int B, int N, int stage_cap);
inline int edge_stage_cap(int row_cap, int conv_row_cap) { return row_cap > conv_row_cap ? row_cap : conv_row_cap; }

// Four launches on `stream`: init, scatter (one thread per edge), rows (one wave per row), finish;
// then ell_pad_kernel when the ELL image is wanted.  Argument errors: negative code, nothing launched.
int edge_image_build(const char* who, const EdgeBatch& g, const EdgeEll& ell, const EdgeConv& cv,
                     const EdgeRitz& rz, void* scratch, int64_t scratch_bytes, int32_t* status,
                     hipStream_t stream);

// ---- typed batches: edge_type [n_edges] in [0, E), one conv image per operator channel ----------------
constexpr int kEdgeMaxTypes = 7;    // E + 1 <= 8 operator channels (LARGE_MAX_OPERATORS)

struct EdgeConvChannels {    // E + 1 conv images, channel major, each in EdgeConv's row format
  uint32_t* ent;             // [E + 1][B][N][cap]
  float* vals;               // [E + 1][B][N][cap], optional
  int32_t* counts;           // [E + 1][B][N]
  int32_t* flags;            // one word: bit 1 = a row of channel 0 beyond `cap` (the others are subsets + diagonal)
  int cap;
};

// cursor [B][N] int32 + per-type neighbour counts [B][N][E] int32 + staged columns [B][N][cap] u16 + staged
// types [B][N][cap] u8
int64_t edge_typed_scratch_bytes(int B, int N, int E, int cap);

// Four launches on `stream`: init, scatter, rows, finish.  Every channel in ascending column order.
int edge_typed_image_build(const char* who, const EdgeBatch& g, const int32_t* edge_type, int E,
                           const EdgeConvChannels& cv, void* scratch, int64_t scratch_bytes, int32_t* status,
                           hipStream_t stream);

}  // namespace lnz
