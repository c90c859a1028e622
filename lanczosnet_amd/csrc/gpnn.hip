// The GPNN baseline (reference model/gpnn.py:141-251, config/qm8_gpnn.yaml): all num_prop outer steps —
// gated propagation on the two partition graphs, the state MLP, one GGNN step — and the gated masked-mean
// readout in ONE launch.
//
// lnz_gpnn_forward — with the state S [rows, D], per outer step
//     Sc = S;  num_prop_cluster times:  Sc = part(Sc, Lcl)           (model/gpnn.py:192-213)
//     Sx = S;  num_prop_cut     times:  Sx = part(Sx, Lct)
//     part(X, Lp):  M = relu(X W1_0^T + b1_0) W2_0^T + b2_0          (msg_func[0])
//                   A = Ŵ M per molecule, Ŵ = Lp ('sum'), Ŵ[i, j] = Lp[i, j] / (sum_j Lp[i, j] + FLT_EPSILON) ('avg')
//                   X' = GRUCell_partition(A, X)                      (input D, hidden D)
//     S  = relu([S | Sc | Sx] Ws1^T + bs1) Ws2^T + bs2                (state_func, hidden 512)
//     S  = the GGNN step of ggnn.hip on S with L != 0, msg_func[0 .. C-1] and update_func (GRU, input C D)
// and after the last step the readout of ggnn.hip: y = (Wo s + bo) * sigmoid(wg s + bg), score = mean of y over
// the rows with mask != 0 (all N rows without a mask; no masked row: 0 / 0 = NaN).  Every one of the N rows of a
// molecule takes part.  L is only ever compared with zero (a NaN or a negative entry is an edge); L_cluster and
// L_cut enter BY VALUE.  None of the three is written.  A partition count of 0 hands S itself to the state MLP.
//
// Shape as built.  A workgroup of eight waves owns a tile of floor(32 / N) whole molecules, packed densely; the
// three states S, Sc, Sx and the M, A, H blocks of the message stay in LDS from the first step to the readout.
// The prologue reads L into per-row bit masks (ggnn_tile.hpp) and the two partition graphs into per-row weight
// vectors [row][32] (gpnn_tile.hpp: the 'avg' division is done once, there).  The partition step and the state
// MLP are gpnn_tile.hpp's; the GGNN step and the readout are ggnn_tile.hpp's LNZ_GGNN_TILE_STEP and gated_readout, the
// very text and function ggnn.hip uses.
// All products run on v_mfma_f32_16x16x4_f32 through tile_gemm, weights from global memory (L2 resident: 3.4 MB
// at the yaml shape), states from LDS.  Barriers per outer step with counts (1, 1): 1 behind the two copies,
// 2 x 5 in the partition steps, 9 in the state MLP, 3 C + 2 in the GGNN step.
// LDS at D = 128: five [32][132] state blocks + H [32][132] + two weight blocks [32][32] + masks = 111,744 B, one
// workgroup per CU.  No atomics, no cross-workgroup traffic, every sum in a fixed order: bit-reproducible, and a
// molecule's bits do not depend on its place in the batch.  A 64-row tile (about 224 KB as laid out here) was
// not built.  Registers and measurements: DESIGN.md §4.14.
#include "common.hpp"
#include "gpnn_tile.hpp"

namespace {

// floats of dynamic LDS: S, Sc, Sx, M, A [GR][D + 4], H [GR][132], the partition weights [2][GR][32],
// bits + inv [8][GR], rowbase [GR]
__host__ __device__ constexpr int gpnn_lds_floats(int D, int GR) {
  return 5 * GR * (D + 4) + GR * HS + 2 * GR * GMAXN + 2 * GMAXC * GR + GR;
}

struct GpnnGraphs {
  const float* L;
  int64_t sb, sr, sc, sch;
  const float* Lcl;
  int64_t cl_b, cl_r, cl_c;
  const float* Lct;
  int64_t ct_b, ct_r, ct_c;
};

// the weights of one GRU cell / one two-layer MLP
struct GpnnCell {
  const float *Wih, *bih, *Whh, *bhh;
};
struct GpnnMlp {
  const float *W1, *b1, *W2, *b2;
};

template <int D, int RT>
__global__ __launch_bounds__(GNT) void gpnn_forward_kernel(
    const float* __restrict__ state0, const int ld0, const GpnnGraphs gr, const unsigned char* __restrict__ mask,
    const GpnnMlp msg, const GpnnCell upd, const GpnnCell par, const GpnnMlp stf, const float* __restrict__ Wo,
    const float* __restrict__ bo, const float* __restrict__ wg, const float* __restrict__ bg, const int B,
    const int N, const int C, const int P, const int num_prop, const int num_cluster, const int num_cut,
    const int avg, float* __restrict__ score, float* __restrict__ state_out, const int ldso) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int GR = 16 * RT;    // rows per tile
  constexpr int SS = D + 4;      // row stride of the state blocks
  float* const Sb = smem;
  float* const Scb = Sb + GR * SS;
  float* const Sxb = Scb + GR * SS;
  float* const Mb = Sxb + GR * SS;
  float* const Ab = Mb + GR * SS;
  float* const Hb = Ab + GR * SS;
  float* const wts = Hb + GR * HS;                                      // [2][row][32]
  unsigned* const bits = reinterpret_cast<unsigned*>(wts + 2 * GR * GMAXN);   // [c][row]
  float* const inv = reinterpret_cast<float*>(bits + GMAXC * GR);      // [c][row]
  int* const rowbase = reinterpret_cast<int*>(inv + GMAXC * GR);       // first row of the row's molecule

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, g = lane >> 4;
  const TileSpan ts = tile_span<RT>(B, N);
  const int64_t row0 = ts.mol0 * N;
  const int rows = ts.rows;

  // ---- the state, the bit masks and denominators of L, the weights of the partition graphs
  load_state_tile<D, RT>(Sb, state0, row0, ld0, rows);
  load_edge_bits<RT>(bits, gr.L, gr.sb, gr.sr, gr.sc, gr.sch, ts, N, C,
                     [&](const int at, const int degree) { inv[at] = ggnn_edge_weight(avg, degree); });
  load_partition_weights<RT>(wts, gr.Lcl, gr.cl_b, gr.cl_r, gr.cl_c, gr.Lct, gr.ct_b, gr.ct_r, gr.ct_c, ts, N, avg);
  set_rowbase<RT>(rowbase, N, rows);
  __syncthreads();

  const MessageTile mt = {Sb, Mb, Ab, Hb, bits, inv, rowbase};

  for (int step = 0; step < num_prop; ++step) {
    // ---- within the clusters, then between them: each from the step's S
    if (num_cluster > 0) copy_state_tile<D, RT>(Scb, Sb);
    if (num_cut > 0) copy_state_tile<D, RT>(Sxb, Sb);
    __syncthreads();
    for (int i = 0; i < num_cluster; ++i)
      partition_step<D, RT>(Scb, Mb, Ab, Hb, wts, rowbase, N, rows, msg.W1, msg.b1, msg.W2, msg.b2, par.Wih, par.bih,
                            par.Whh, par.bhh, wave, m, g);
    for (int i = 0; i < num_cut; ++i)
      partition_step<D, RT>(Sxb, Mb, Ab, Hb, wts + GR * GMAXN, rowbase, N, rows, msg.W1, msg.b1, msg.W2, msg.b2,
                            par.Wih, par.bih, par.Whh, par.bhh, wave, m, g);
    // ---- the state MLP
    state_mlp<D, RT>(Sb, num_cluster > 0 ? Scb : Sb, num_cut > 0 ? Sxb : Sb, Hb, stf.W1, stf.b1, stf.W2, stf.b2, wave,
                     m, g);
    // ---- the GGNN step
    LNZ_GGNN_TILE_STEP(D, RT, mt, msg.W1, msg.b1, msg.W2, msg.b2, upd.Wih, upd.bih, upd.Whh, upd.bhh, C);
  }

  // ---- the final state, on request
  if (state_out != nullptr) store_state_tile<D>(state_out + row0 * (int64_t)ldso, ldso, Sb, rows);
  // ---- readout, its slots in the H block: H is dead
  gated_readout<D>(Sb, Hb, mask, Wo, bo, wg, bg, ts, N, P, score);
}

template <int D>
int launch(const float* state0, int ld0, const GpnnGraphs& gr, const uint8_t* mask, const GpnnMlp& msg,
           const GpnnCell& upd, const GpnnCell& par, const GpnnMlp& stf, const float* Wo, const float* bo,
           const float* wg, const float* bg, int B, int N, int C, int P, int num_prop, int num_cluster, int num_cut,
           int avg, float* score, float* state_out, int ldso, int grid, hipStream_t s, const char* who) {
  const size_t lds = sizeof(float) * (size_t)gpnn_lds_floats(D, 32);
  auto kfn = gpnn_forward_kernel<D, 2>;
  LNZ_DYNAMIC_LDS(kfn, lds, "gpnn.hip");
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(GNT), lds, s, state0, ld0, gr, mask, msg, upd, par, stf, Wo, bo,
                     wg, bg, B, N, C, P, num_prop, num_cluster, num_cut, avg, score, state_out, ldso);
  return lnz::check_launch(who);
}

}  // namespace

extern "C" int lnz_gpnn_forward(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                                int64_t stride_c, int64_t stride_ch, const float* L_cluster, int64_t cl_stride_b,
                                int64_t cl_stride_r, int64_t cl_stride_c, const float* L_cut, int64_t ct_stride_b,
                                int64_t ct_stride_r, int64_t ct_stride_c, const uint8_t* mask, const float* W1,
                                const float* b1, const float* W2, const float* b2, const float* Wih,
                                const float* bih, const float* Whh, const float* bhh, const float* Wpih,
                                const float* bpih, const float* Wphh, const float* bphh, const float* Ws1,
                                const float* bs1, const float* Ws2, const float* bs2, const float* Wo,
                                const float* bo, const float* wg, const float* bg, int B, int N, int C, int D,
                                int P, int num_prop, int num_prop_cluster, int num_prop_cut, int avg, float* score,
                                float* state_out, int ldso, int tile_rows, lnz_stream_t stream) {
  const char* const who = "lnz_gpnn_forward";
  LNZ_REQUIRE(state0 && L && L_cluster && L_cut && W1 && b1 && W2 && b2 && Wih && bih && Whh && bhh && Wpih && bpih &&
                  Wphh && bphh && Ws1 && bs1 && Ws2 && bs2 && Wo && bo && wg && bg && score,
              LNZ_EINVAL, "%s: null pointer", who);
  {
    const float* const w[8] = {W1, b1, W2, b2, Wih, bih, Whh, bhh};
    const int rc = check_propagation(who, state0, ld0, state_out, ldso, stride_b, stride_r, stride_c, stride_ch, w, B,
                                     N, C, D, &P, num_prop);
    if (rc != LNZ_OK) return rc;
  }
  LNZ_REQUIRE(num_prop_cluster >= 0 && num_prop_cut >= 0, LNZ_ENOTSUP,
              "%s: num_prop_cluster = %d, num_prop_cut = %d must not be negative", who, num_prop_cluster, num_prop_cut);
  LNZ_REQUIRE(cl_stride_b >= 0 && cl_stride_r >= 0 && cl_stride_c >= 0 && ct_stride_b >= 0 && ct_stride_r >= 0 &&
                  ct_stride_c >= 0,
              LNZ_EINVAL, "%s: negative stride of L_cluster or L_cut", who);
  {
    bool more_aligned = true;
    for (const float* p : {Wpih, bpih, Wphh, bphh, Ws1, bs1, Ws2, bs2}) more_aligned = more_aligned && aligned16(p);
    LNZ_REQUIRE(more_aligned, LNZ_ENOTSUP,
                "%s: the rows of the partition cell's and of state_func's weights must be 16-byte aligned", who);
  }
  {
    const int rc = check_outputs(who, state0, ld0, score, state_out, ldso, nullptr, B, N, D, P, num_prop, tile_rows,
                                 "0 or 32");
    if (rc != LNZ_OK) return rc;
  }
  LNZ_REQUIRE(tile_rows != 64, LNZ_ENOTSUP, "%s: the 64-row tile is not built (three states, M, A and H of 64 rows "
              "exceed the LDS); tile_rows = 0 or 32", who);
  const int mpt = 32 / N;
  const int64_t grid = ((int64_t)B + mpt - 1) / mpt;
  const GpnnGraphs gr = {L,           stride_b,    stride_r, stride_c,    stride_ch,   L_cluster,  cl_stride_b,
                         cl_stride_r, cl_stride_c, L_cut,    ct_stride_b, ct_stride_r, ct_stride_c};
  const GpnnMlp msg = {W1, b1, W2, b2}, stf = {Ws1, bs1, Ws2, bs2};
  const GpnnCell upd = {Wih, bih, Whh, bhh}, par = {Wpih, bpih, Wphh, bphh};
  hipStream_t s = (hipStream_t)stream;
  lnz::note_kernel("gpnn_forward_kernel<%d, 2>", D);
#define LNZ_GPNN_LAUNCH(DD)                                                                                         \
  launch<DD>(state0, ld0, gr, mask, msg, upd, par, stf, Wo, bo, wg, bg, B, N, C, P, num_prop, num_prop_cluster,      \
             num_prop_cut, avg ? 1 : 0, score, state_out, ldso, (int)grid, s, who)
  LNZ_GGNN_WIDTHS(D, LNZ_GPNN_LAUNCH)
#undef LNZ_GPNN_LAUNCH
}
