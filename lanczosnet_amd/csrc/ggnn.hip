// The GGNN baseline (reference model/ggnn.py:137-197, config/qm8_ggnn.yaml): all num_prop gated
// propagation steps and the gated masked-mean readout in ONE launch.
//
// lnz_ggnn_forward — with the state S [rows, D], channels c = 0 .. C-1 (C = num_bond_type + 1) and the
// message hidden width 128 (hard-coded in the reference), per step
//     H_c  = relu(S W1_c^T + b1_c)                         [rows, 128]
//     M_c  = H_c W2_c^T + b2_c                             [rows, D]
//     A_c  = Â_c M_c per molecule, Â_c = (L[.., c] != 0)            ('sum')
//                                  Â_c = (L[.., c] != 0) / (row degree + FLT_EPSILON)   ('avg')
//     gi   = sum_c A_c W_ih[:, cD:(c+1)D]^T + b_ih ;  gh = S W_hh^T + b_hh             [rows, 3D]
//     r, z = sigmoid(gi_r + gh_r), sigmoid(gi_z + gh_z) ;  n = tanh(gi_n + r * gh_n)
//     S'   = (1 - z) * n + z * S
// and after the last step y = (Wo s + bo) * sigmoid(wg s + bg), score = mean of y over the rows with
// mask != 0 (all N rows without a mask; no masked row: 0 / 0 = NaN like the reference's empty mean).
// lnz_ggnn_forward_states is the same kernel template with one more pointer: it also leaves the state
// trajectory [num_prop + 1][B N][D], all the backward (ggnn_grad.hip) keeps of the forward.
// Every one of the N rows of a molecule takes part in the propagation: a padded row evolves under
// GRU(0, h).  L is only ever compared with zero (a NaN or a negative entry is an edge), never written.
//
// Shape as built.  A workgroup of eight waves (512 threads) owns a tile of floor(R / N) whole
// molecules = at most R rows, packed densely, R = 64 or 32 (below); their state stays in LDS from the
// first step to the readout, nothing of it goes to HBM between steps.  L is read once, through its
// four strides, into per-row bit masks (bit j of row i of channel c) and the 'avg' reciprocal
// denominators.  The GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fma chain) in the
// transposed form of f32_linear.hip: the A operand is a 16-byte fragment of a weight row read from
// global memory (L2 resident: 2.5 MB at the yaml shape), the B operand a 16-byte fragment of a state
// row read from LDS, so a lane ends up with four consecutive features of one row.  The weight
// fragments of a product run two (gates) or four 16-column blocks ahead of its MFMAs.  Wave w owns the
// 16 hidden columns 16 w .. of H_c and, where 16 w < D, the 16 features 16 w .. of M_c and of the three
// gates: its gi accumulators (r; z; n: 3 x R / 16 row tiles x 4 registers = 48 per lane at R = 64)
// live in registers across the channel loop, channel c's product (a k-ordered chain of D terms of its
// own, 48 more registers) is added into them, and the [rows, C 128] message hidden never exists as a
// whole.  gh = S W_hh^T follows the channel loop, in front of the GRU cell.  The aggregate Â_c M_c
// runs on the VALU over the set bits only, j ascending.  Three barriers per channel, two per step.
// LDS at D = 128, R = 64: S, M_c, A_c 64 x 132 floats each + H_c 64 x 132 + masks = 139,520 B (the
// per-device dynamic-LDS grant of common.hpp), one workgroup per CU; R = 32: 69,760 B.  At most 254
// VGPRs at R = 64, no scratch (the table: DESIGN.md §4.12).  No atomics, no cross-workgroup traffic, every
// sum in a fixed order: bit-reproducible.  sigmoid = 1 / (1 + expf(-x)) and tanhf stay finite and correct at |x| >= 100.
//
// Tile height: a tile's 15 steps take the same time whatever the batch, so R = 64 (half the weight
// reads per row) serves batches that fill the chip and R = 32 batches whose 32-row tiles all fit in one
// round of the compute units (tile_rows = 0 chooses; a row's arithmetic and bits are the same in
// both).  The prologue, the step (LNZ_GGNN_TILE_STEP: the message block, the gates, the cell), the state store and the
// readout (gated_readout) are ggnn_tile.hpp's, shared to the letter with ggnn_grad.hip, mpnn.hip and gpnn.hip;
// this file keeps the LDS layout, the loop over the steps with the trajectory's stores, and the entry points.
// R = 128 (192 accumulator registers per lane at 256 threads) and the folded form F_c =
// W_ih[:, c] W2_c were not built.  Measurements: DESIGN.md §4.12.
#include "common.hpp"
#include "ggnn_tile.hpp"

namespace {

// floats of dynamic LDS: S, M, A [GR][D + 4], H [GR][132], bits + inv [8][GR], rowbase [GR]
__host__ __device__ constexpr int ggnn_lds_floats(int D, int GR) {
  return 3 * GR * (D + 4) + GR * HS + 2 * GMAXC * GR + GR;
}

template <int D, int RT, bool TRAJ>
__global__ __launch_bounds__(GNT) void ggnn_forward_kernel(
    const float* __restrict__ state0, const int ld0, const float* __restrict__ L, const int64_t stride_b,
    const int64_t stride_r, const int64_t stride_c, const int64_t stride_ch,
    const unsigned char* __restrict__ mask, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ Wih,
    const float* __restrict__ bih, const float* __restrict__ Whh, const float* __restrict__ bhh,
    const float* __restrict__ Wo, const float* __restrict__ bo, const float* __restrict__ wg,
    const float* __restrict__ bg, const int B, const int N, const int C, const int P, const int num_prop,
    const int avg, float* __restrict__ score, float* __restrict__ state_out, const int ldso,
    float* __restrict__ states) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int GR = 16 * RT;    // rows per tile
  constexpr int SS = D + 4;      // row stride of S, M_c, A_c
  float* const Sb = smem;
  float* const Mb = Sb + GR * SS;
  float* const Ab = Mb + GR * SS;
  float* const Hb = Ab + GR * SS;
  unsigned* const bits = reinterpret_cast<unsigned*>(Hb + GR * HS);   // [c][row]
  float* const inv = reinterpret_cast<float*>(bits + GMAXC * GR);      // [c][row]
  int* const rowbase = reinterpret_cast<int*>(inv + GMAXC * GR);       // first row of the row's molecule

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  const TileSpan ts = tile_span<RT>(B, N);
  const int64_t mol0 = ts.mol0, row0 = ts.mol0 * N;   // first molecule and first global row of the tile
  const int rows = ts.rows;

  // ---- the state, the bit masks and denominators of L, the molecule of every row
  load_state_tile<D, RT>(Sb, state0, row0, ld0, rows);
  load_edge_bits<RT>(bits, L, stride_b, stride_r, stride_c, stride_ch, ts, N, C,
                     [&](const int at, const int degree) { inv[at] = ggnn_edge_weight(avg, degree); });
  set_rowbase<RT>(rowbase, N, rows);
  __syncthreads();

  const MessageTile mt = {Sb, Mb, Ab, Hb, bits, inv, rowbase};

  // the state trajectory [num_prop + 1][B N][D] (TRAJ: lnz_ggnn_forward_states; `states` is null and unread
  // otherwise): S_t at the start of step t, S_T after the last.  A copy of the LDS rows: the arithmetic does
  // not see it, and the instantiation without it is the kernel lnz_ggnn_forward always launched
  const auto put_state = [&](const int t) {
    store_state_tile<D>(states + ((int64_t)t * B + mol0) * N * D, D, Sb, rows);
  };

  for (int step = 0; step < num_prop; ++step) {
    if constexpr (TRAJ) put_state(step);
    LNZ_GGNN_TILE_STEP(D, RT, mt, W1, b1, W2, b2, Wih, bih, Whh, bhh, C);
  }

  // ---- the final state, on request
  if constexpr (TRAJ) put_state(num_prop);
  if (state_out != nullptr) store_state_tile<D>(state_out + row0 * (int64_t)ldso, ldso, Sb, rows);
  // ---- readout, its slots in the H block: H_c is dead
  gated_readout<D>(Sb, Hb, mask, Wo, bo, wg, bg, ts, N, P, score);
}

template <int D, int RT, bool TRAJ>
int launch(const float* state0, int ld0, const float* L, int64_t sb, int64_t sr, int64_t sc, int64_t sch,
           const uint8_t* mask, const float* W1, const float* b1, const float* W2, const float* b2,
           const float* Wih, const float* bih, const float* Whh, const float* bhh, const float* Wo,
           const float* bo, const float* wg, const float* bg, int B, int N, int C, int P, int num_prop, int avg,
           float* score, float* state_out, int ldso, float* states, int grid, hipStream_t s, const char* who) {
  const size_t lds = sizeof(float) * (size_t)ggnn_lds_floats(D, 16 * RT);
  auto kfn = ggnn_forward_kernel<D, RT, TRAJ>;
  LNZ_DYNAMIC_LDS(kfn, lds, "ggnn.hip");
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(GNT), lds, s, state0, ld0, L, sb, sr, sc, sch, mask, W1, b1,
                     W2, b2, Wih, bih, Whh, bhh, Wo, bo, wg, bg, B, N, C, P, num_prop, avg, score, state_out, ldso,
                     states);
  return lnz::check_launch(who);
}

int forward_impl(const char* who, const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                 int64_t stride_c, int64_t stride_ch, const uint8_t* mask, const float* W1, const float* b1,
                 const float* W2, const float* b2, const float* Wih, const float* bih, const float* Whh,
                 const float* bhh, const float* Wo, const float* bo, const float* wg, const float* bg, int B, int N,
                 int C, int D, int P, int num_prop, int avg, float* score, float* state_out, int ldso,
                 float* states, int tile_rows, lnz_stream_t stream) {
  LNZ_REQUIRE(state0 && L && W1 && b1 && W2 && b2 && Wih && bih && Whh && bhh && Wo && bo && wg && bg && score,
              LNZ_EINVAL, "%s: null pointer", who);
  {
    const float* const w[8] = {W1, b1, W2, b2, Wih, bih, Whh, bhh};
    const int rc = check_propagation(who, state0, ld0, state_out, ldso, stride_b, stride_r, stride_c, stride_ch, w, B,
                                     N, C, D, &P, num_prop);
    if (rc != LNZ_OK) return rc;
  }
  {
    const int rc = check_outputs(who, state0, ld0, score, state_out, ldso, states, B, N, D, P, num_prop, tile_rows,
                                 "0 (chosen by the batch), 32 or 64");
    if (rc != LNZ_OK) return rc;
  }
  const int rows_per_tile = choose_tile_rows(B, N, tile_rows);
  const int mpt = rows_per_tile / N;
  const int64_t grid = ((int64_t)B + mpt - 1) / mpt;
  hipStream_t s = (hipStream_t)stream;
  lnz::note_kernel("ggnn_forward_kernel<%d, %d>", D, rows_per_tile / 16);
#define LNZ_GGNN_LAUNCH_(DD, RTT, TR)                                                                              \
  launch<DD, RTT, TR>(state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, mask, W1, b1, W2, b2, Wih, bih, Whh,  \
                      bhh, Wo, bo, wg, bg, B, N, C, P, num_prop, avg ? 1 : 0, score, state_out, ldso, states,        \
                      (int)grid, s, who)
#define LNZ_GGNN_LAUNCH(DD)                                                                               \
  (rows_per_tile == 32 ? (states ? LNZ_GGNN_LAUNCH_(DD, 2, true) : LNZ_GGNN_LAUNCH_(DD, 2, false)) \
                       : (states ? LNZ_GGNN_LAUNCH_(DD, 4, true) : LNZ_GGNN_LAUNCH_(DD, 4, false)))
  LNZ_GGNN_WIDTHS(D, LNZ_GGNN_LAUNCH)
#undef LNZ_GGNN_LAUNCH
#undef LNZ_GGNN_LAUNCH_
}

}  // namespace

extern "C" int lnz_ggnn_forward(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                                int64_t stride_c, int64_t stride_ch, const uint8_t* mask, const float* W1,
                                const float* b1, const float* W2, const float* b2, const float* Wih,
                                const float* bih, const float* Whh, const float* bhh, const float* Wo,
                                const float* bo, const float* wg, const float* bg, int B, int N, int C, int D,
                                int P, int num_prop, int avg, float* score, float* state_out, int ldso,
                                int tile_rows, lnz_stream_t stream) {
  return forward_impl("lnz_ggnn_forward", state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, mask, W1, b1, W2, b2,
                      Wih, bih, Whh, bhh, Wo, bo, wg, bg, B, N, C, D, P, num_prop, avg, score, state_out, ldso, nullptr,
                      tile_rows, stream);
}

extern "C" int lnz_ggnn_forward_states(const float* state0, int ld0, const float* L, int64_t stride_b,
                                       int64_t stride_r, int64_t stride_c, int64_t stride_ch, const uint8_t* mask,
                                       const float* W1, const float* b1, const float* W2, const float* b2,
                                       const float* Wih, const float* bih, const float* Whh, const float* bhh,
                                       const float* Wo, const float* bo, const float* wg, const float* bg, int B,
                                       int N, int C, int D, int P, int num_prop, int avg, float* score,
                                       float* state_out, int ldso, float* states, int tile_rows,
                                       lnz_stream_t stream) {
  LNZ_REQUIRE(states, LNZ_EINVAL, "lnz_ggnn_forward_states: null pointer");
  return forward_impl("lnz_ggnn_forward_states", state0, ld0, L, stride_b, stride_r, stride_c, stride_ch, mask, W1, b1,
                      W2, b2, Wih, bih, Whh, bhh, Wo, bo, wg, bg, B, N, C, D, P, num_prop, avg, score, state_out, ldso,
                      states, tile_rows, stream);
}
