/*
 * lanczosnet_hip.h — C ABI of the MI355X (gfx950) LanczosNet hot path.
 *
 * The reference (lrjconan/LanczosNetwork) has no FFI in front of this path: the boundary
 * is the Python nn.Module contract.  This header is what a binding for
 * that path binds to; `lanczosnet_amd/_lib.py` is the ctypes binding, INTEGRATION.md shows
 * the reference-side stub.  All pointers are DEVICE pointers unless the name ends in
 * `_host`; all tensors are dense row-major float32 unless stated; `stream` is a
 * hipStream_t (NULL = default stream).  Every entry point is asynchronous on `stream`,
 * returns 0 on success and a negative LNZ_E* code on error (message via lnz_last_error()).
 * Nothing here allocates device memory or synchronises the device.
 *
 * Each entry point cites the reference code it replaces (paths relative to the reference
 * repository root).
 */
#ifndef LANCZOSNET_HIP_H_
#define LANCZOSNET_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7: lnz_midgraph_forward's `sync` grew to B * (num_layer + 1) words (placement words behind the
 *    arrival counters) and its launch is chunked to the resident workgroups; + the K-step entry
 *    (lnz_lanczos_ritz_kstep[_image], _workspace_bytes), the sparse large-graph conv
 *    (lnz_large_sparse_image, lnz_large_pack_vectors, lnz_large_gemm1_rows, lnz_large_sparse_conv[_f32];
 *    lnz_large_conv accepts C = 0), lnz_head_backward, lnz_node_extents, the out-of-place split-pack
 *    entries (lnz_split_laplacian_pack_to, lnz_spectral_gains_rows_split_to), lnz_last_kernel,
 *    lnz_stream_create_cu_masked; the full eigendecomposition (lnz_sym_eigh_topk, _workspace_bytes);
 *    + the wide K-step entry (lnz_lanczos_ritz_kstep_wide, _workspace_bytes: N <= 16384, M <= 256);
 *    + large graphs from edge lists (lnz_lanczos_ritz_kstep_edges, lnz_lanczos_ritz_kstep_wide_edges,
 *    lnz_laplacian_l4_edges_image, each with a _workspace_bytes sibling: no N x N array);
 *    + the backward of the one-operator sparse large-graph layer (lnz_large_grad_project,
 *    lnz_large_grad_spectral, lnz_large_grad_input: additive, the version stays);
 *    + the same backward over R = 2 .. 8 operator channels of a typed batch (lnz_large_sparse_conv_split_f32,
 *    lnz_large_grad_input_channels: additive, the version stays);
 *    + the symmetry check of a sparse image (lnz_large_sparse_image_symmetry: what lets a dense collated batch
 *    take that backward; additive, the version stays);
 *    + the GAT baseline's attention and readout (lnz_gat_attention, lnz_gat_readout: additive, the version
 *    stays);
 *    + their backward (lnz_gat_attention_backward, lnz_gat_readout_backward and the two
 *    _workspace_floats queries: additive, the version stays);
 *    + the GGNN baseline's fused gated propagation and readout (lnz_ggnn_forward: additive, the version
 *    stays);
 *    + its backward (lnz_ggnn_forward_states, lnz_ggnn_backward_step, lnz_ggnn_readout_backward and the
 *    _workspace_floats query: additive, the version stays);
 *    + the MPNN baseline's fused edge-network propagation and Set2Vec readout (lnz_mpnn_forward,
 *    lnz_set2vec_readout: additive, the version stays);
 *    + the backward of that propagation (lnz_mpnn_forward_states, lnz_mpnn_backward_step: additive, the
 *    version stays);
 *    + the GPNN baseline's fused partition propagation, state MLP, gated propagation and readout
 *    (lnz_gpnn_forward: additive, the version stays);
 *    + lnz_forward_args.rare_strips / .no_fold / .rare_debug at the END of the block (the strip forward's folded form of
 *    the rare bond-type channels, on by default: zeros = folded where cheaper; additive, the version
 *    stays — a caller built against the shorter block must zero-fill lnz_forward_args_size() bytes);
 *    + lnz_pack_fold_weights / lnz_pack_fold_weights_size and lnz_forward_args.Wf at the END of the block (the
 *    folded weights of the rare bond-type channels, summed once per weight set instead of in every wave of every
 *    launch; NULL = summed in registers as before, the same bits; additive, the version stays);
 * 6: lnz_forward_args lost Wp16 / w16_off / Wp16_head / Lp16 (gemm_mode 1 is now the split precision
 *    inside the strip kernel: lnz_pack_rows_k8_split; lnz_pack_rows_f16x2 and
 *    lnz_pack_laplacian_f16x2 are gone) and gained dbias_part_cap; + lnz_midgraph_forward,
 *    lnz_spectral_mlp_grad;  5: + the strip plan (lnz_plan_strips, strips / n_strips / strip_cap);
 * 4: + lnz_large_pack_operators_fold, lnz_f32_linear_workspace_floats (stream-K inside
 *    lnz_f32_linear: the partials argument changed its size and gained a zero-on-entry tail);
 * 3: + lnz_f32_linear, lnz_laplacian, the fp64 training kernels of the AdaLanczosNet spectrum
 *    (lnz_ada_graph_laplacian_f64, lnz_ada_lanczos_layer_f64, lnz_ada_t_powers_f64 and their
 *    _backward);  2: + lnz_lanczos_ritz_ws / _workspace_bytes, lnz_f16x3_*. */
#define LNZ_ABI_VERSION 7
#define LNZ_OK 0
#define LNZ_EINVAL (-1)   /* bad argument (shape/limit)            */
#define LNZ_ELAUNCH (-2)  /* HIP launch / runtime error            */
#define LNZ_ENOTSUP (-3)  /* valid request outside the built range */

#define LNZ_TILE 32       /* node tile: one v_mfma_f32_32x32x2_f32 tile per molecule */
#define LNZ_MAX_CHANNELS 32
/* strip plan (lnz_plan_strips): subtiles of 16 node rows per strip, int32 words per strip entry,
 * molecules the planner packs together (larger batches: chunk by chunk) */
#define LNZ_STRIP_SUB 6
#define LNZ_STRIP_INTS 80
#define LNZ_STRIP_MAX_B 2048
#define LNZ_RARE_DEBUG_INTS 512   /* lnz_forward_args.rare_debug: int32 words per strip */

typedef void* lnz_stream_t;

int lnz_abi_version(void);
const char* lnz_last_error(void);
/* The kernel (name with template arguments) the calling thread's last lnz_lanczosnet_forward /
 * _input_grad launch selected — the launchers choose between the strip and 32 x 32-tile kernels by
 * shape and plan; measurements name what ran instead of restating the rule.  The other launchers
 * that choose between kernels or instantiations note theirs the same way (named at each entry). */
const char* lnz_last_kernel(void);

/* ---- R1: graph Laplacian ------------------------------------------------------------
 * L4 = D^-1/2 (I + A) D^-1/2 for the simple graph (channel 0, A = sum_e A_e) and for every
 * bond-type channel e (channel 1+e), written channels-last like the collate output.
 * Replaces utils/data_helper.py:92-116,155-156 (normalize_adj / get_laplacian 'L4'),
 * dataset/get_qm8_data.py:62-75 and the L part of dataset/qm8.py:225-262.
 * adjs [B,N,N,E]; n_nodes [B] (rows/cols >= n are written as exact zeros and never enter a degree,
 * whatever they hold; a count outside [0, N] is clamped to it, as lnz_collate_qm8 clamps);
 * L [B,N,N,E+1].  Arithmetic in fp64 (the reference builds L4 in float64), stored as float32.
 * A row of I + A whose sum is not positive — zero or negative — gives a zero row and column (the
 * reference's inf -> 0 guard covers the zero sum; for a negative one it returns NaN, see below).
 * lnz_last_kernel() names laplacian_l4_kernel<staged> (a graph's adjacency block staged in LDS by
 * 16-byte loads: it fits beside the degrees in 64 KiB, N*N*E is a multiple of 4 and adjs is 16-byte
 * aligned) or laplacian_l4_kernel<direct>; the same bits either way. */
int lnz_laplacian_l4(const float* adjs, const int32_t* n_nodes, int B, int N, int E,
                     float* L, lnz_stream_t stream);
/* Every kind of get_laplacian (utils/data_helper.py:119-166 over normalize_adj :92-116), same
 * layouts: kind 1 .. 7 = 'L1' .. 'L7' (L1 = D - A, L2 = I - D^-1/2 A D^-1/2, L3 = I - D^-1 A,
 * L4 = D^-1/2 (I+A) D^-1/2, L5 = D^-1 (I+A), L6 = D^-alpha A D^-alpha, L7 = D^-1 A; D = row sums of
 * the normalised matrix, D^-x of an isolated node = 0 like the reference's inf guard), alpha only
 * for kind 6 (reference default 0.5).  The reference's offline scripts store L6 / L7 of the simple
 * graph for the ChebyNet / DCNN baselines (dataset/get_qm8_data.py:73-77,
 * dataset/get_graph_data.py:70-75).  n_nodes is clamped to [0, N] as above.  kind 4 is
 * lnz_laplacian_l4 bit for bit wherever every row sum of I + A is >= 0.  For a negative row sum the
 * two differ: lnz_laplacian keeps the reference's pow(d, -1/2) = NaN (that row and column are NaN),
 * lnz_laplacian_l4 writes a zero row and column.  lnz_last_kernel() names laplacian_kind_kernel<kind>. */
int lnz_laplacian(const float* adjs, const int32_t* n_nodes, int B, int N, int E, int kind,
                  double alpha, float* L, lnz_stream_t stream);

/* ---- R2 + R6: Lanczos tridiagonalisation -> tridiagonal eigensolve -> Ritz select ----
 * Per molecule: full-length (m = n) Lanczos with twice-iterated classical Gram-Schmidt and
 * restart on breakdown on the n x n leading block of A; then the eigendecomposition of T:
 *   N <= 32 (the QM8 regime): lane-parallel — T split into unreduced blocks, one eigenvalue per
 *            lane by section search on Sturm counts, its eigenvector by the twisted factorisation
 *            of T - lambda (dlar1v / MRRR vector), near-degenerate copies re-orthogonalised in
 *            lane order, Ritz vectors V = Q*S; the implicit-shift QL sweep only as the fallback
 *            (info += 256);
 *   32 < N <= 192 (the reference's synthetic-graph configuration, dataset/get_graph_data.py:15-49
 *            with config/graph_lanczos_net.yaml: n in [20,100]): one 512-thread workgroup per
 *            graph, A staged once into LDS, the fp64 basis in LDS up to N = 108 and in a workspace
 *            above (lnz_lanczos_ritz_workspace_bytes; without one lnz_lanczos_ritz takes a
 *            stream-ordered allocation for the launch — LNZ_ENOTSUP while the stream is being
 *            captured: use lnz_lanczos_ritz_ws there); eigenvalues by Sturm-count section search
 *            (one per thread), the K selected eigenvectors by twisted factorisation, V = Q S;
 *            the QL sweep, run barrier-free on per-wave copies of T, as the fallback (info += 256);
 * then stable ordering by descending |lambda| (ties: ascending lambda), cut / zero-pad to K.
 * Produces exactly
 * the (D, V) that utils/data_helper.py:197-223 (np.linalg.eigh + mergesort on -|eig|)
 * followed by dataset/qm8.py:264-291 (pad rows to N, cut/pad to K, cast fp32) produce,
 * up to the basis of degenerate eigenspaces and eigenvector sign.  fp64 arithmetic.
 * A is addressed as A[b*stride_b + r*stride_r + c*stride_c] (elements) so channel 0 of a
 * channels-last L [B,N,N,E+1] can be passed without a copy.  N <= 192 (LNZ_ENOTSUP above: only
 * the K-step streamed kernels below apply there, a different function — SURVEY.md F8).
 * D [B,K], V [B,N,K].  info [B] (optional, may be NULL): number of Lanczos restarts, + 256 when
 * the N <= 32 kernel fell back from its parallel tridiagonal eigensolver to the QL sweep. */
int lnz_lanczos_ritz(const float* A, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                     const int32_t* n_nodes, int B, int N, int K, float* D, float* V,
                     int32_t* info, lnz_stream_t stream);

/* The same with an explicit workspace for the fp64 Krylov basis of graphs too large to keep it in
 * LDS next to A (N > 108): lnz_lanczos_ritz_workspace_bytes(B, N) bytes (0 when none is needed).
 * Always takes the workgroup-per-graph kernel (any N <= 192); flags bit 0 places the basis in the
 * workspace even when it would fit in LDS, bit 1 takes the QL sweep instead of the parallel
 * tridiagonal eigensolver, bit 2 the eight-wave Lanczos phase where the wave-level one would run
 * (basis in LDS), bits 3-4 fix the wave-level phase's parts per row group (1: one, 2: two, 3: four)
 * — all used by the tests to cover every variant at one size.
 * The workgroup kernel's eigensolver: T split into unreduced blocks, one eigenvalue per thread by
 * section search on Sturm counts, the eigenvectors of the K SELECTED eigenvalues by the twisted
 * factorisation of T - lambda (one thread per vector), V = Q S; two eigenvalues of one block closer
 * than 1e-8 |T| send the graph to the QL sweep (info += 256), as does K > ~N/2 (no room for the
 * vectors next to T in LDS). */
int64_t lnz_lanczos_ritz_workspace_bytes(int B, int N);
int lnz_lanczos_ritz_ws(const float* A, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                        const int32_t* n_nodes, int B, int N, int K, float* D, float* V,
                        int32_t* info, void* workspace, int64_t workspace_bytes, int flags,
                        lnz_stream_t stream);


/* ---- R9 / R11 beyond the 32-node tile: streamed spectral convolution for large dense graphs ----
 * (BASELINE config 5: LanczosNetGeneral, N = 2048, K = 64, batch 256, bf16 operands / fp32
 * accumulate).  One conv layer of model/lanczos_net_general.py:157-182,
 *     X' = relu( sum_e L_e (X W_e^T) + V [ sum_s diag(g_s) (V^T X) W_s^T ] + b ),
 * as four launches; hidden width 128, input width <= 128, K <= 64, any N.
 * planes = 1: bf16 operands (8-bit mantissa: ~1e-2 after 7 layers).  planes = 3: every fp32
 * operand travels as three bf16 pieces and every product as its six piece products of order
 * <= 2, fp32 accumulate: fp32-grade results from the same kernels (the parity mode).
 * planes = 2: two fp16 pieces per operand and the three products hi hi + hi lo + lo hi (~2^-22;
 * 2/3 of the bytes and half the matrix work of planes = 3).  In this mode the A operands carry a
 * factor 2^10 (lnz_large_pack_operators applies it to L and V; the caller applies it to the
 * weight pieces of Wf) which lnz_large_gemm1 / lnz_large_conv divide out; B operands (X, Zt, Tt)
 * are plain fp16 pieces: |activations| must stay below 65504.
 *   Nk = lnz_large_nk(N) = N rounded up to 64 (the k extent of the packed operands).
 *   lnz_large_pack_operators  once per batch.  L [B,N,N,C] fp32 addressed by element strides
 *                             (channels-last collate layout, dataset/graph_data.py collate) ->
 *                             Lb [planes][B][C][RT][Nk/64][4][64][8] bf16 in fragment-tile order
 *                             (RT = ceil(N/32) row groups; chunk (rg, kb) = 32 rows x 64 k as the
 *                             four v_mfma_f32_16x16x32_bf16 A fragments f = 2 rt + ks, lane =
 *                             16 kq + r15 holding row 32 rg + 16 rt + r15, k 64 kb + 32 ks + 8 kq
 *                             .. + 7);  V [B,N,K] -> Vb [planes][B][RT][4][64][8] likewise.
 *   lnz_large_gemm1           Zt [planes][B][C][128][Nk] bf16 = (X W_c^T)^T for the C node-space
 *                             channels; X [B,N,ldx] fp32 (first din columns used);
 *                             Wf [planes][C][4][dinp/16][64][8] bf16 = the channel blocks of the
 *                             mix weight (dinp = din rounded up to 16, zero padded) in
 *                             v_mfma_f32_32x32x16_bf16 A-fragment order: fragment (c, mt, ks),
 *                             lane l holds W_c[32 mt + (l & 31)][16 ks + 8 (l >> 5) .. + 7].
 *                             Columns n >= N of Zt are NOT written: the caller provides a
 *                             zero-initialised buffer (it can be reused for every layer).
 *   lnz_large_spectral        Tt [planes][B][128][64] bf16 = (sum_s diag(g_s) (V^T X) W_s^T)^T;
 *                             exact fp32 inside (two launches: row-chunked projection V^T X with
 *                             fp32 atomics into Ybuf, then the per-graph mix).  G [B,S,K] = this
 *                             layer's gains (one [B,S,K] slice of lnz_spectral_gains' output);
 *                             Wt = lnz_pack_rows_k8 of W_long [128][S*dinp] fp32, the long-scale
 *                             column blocks of the mix weight, each zero padded to dinp columns;
 *                             Ybuf [B][64][128] fp32 work buffer, ZERO on entry, zero on return.
 *   lnz_large_conv            Xout [B,N,128] fp32 = act( sum_c Lb_c Zt_c^T + Vb Tt^T + bias ).
 * Replaces the per-slice bmm / cat / Linear of model/lanczos_net_general.py:161-182 (and
 * model/lanczos_net.py:157-182 for N > 32). */
int64_t lnz_large_nk(int N);
int lnz_large_pack_operators(const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                             int64_t stride_ch, const float* V, int B, int N, int C, int K,
                             int planes, uint16_t* Lb, uint16_t* Vb, lnz_stream_t stream);
/* The same with CHANNEL FOLDING.  With one edge type (config/graph_lanczos_net.yaml:14) the
 * bond-type channel of the collated L is the simple-graph channel again (dataset/graph_data.py:
 * 225-262), and sum_c L_c X W_c^T = L (X (sum_c W_c)^T) over a class of equal operators: only the
 * n_src DISTINCT channels chan_src_host[0..n_src) (ascending) are packed, Lb [planes][B][n_src]...;
 * lnz_large_gemm1 / lnz_large_conv then run with C = n_src and the caller sums the mix-weight
 * blocks of a class.  chan_rep_host[c] (c < C) = packed slot whose source channel c is CLAIMED to equal
 * (chan_src_host[chan_rep_host[c]] == c: packed itself).  With neq != NULL (one device uint64, zeroed by the
 * caller) the kernel — which has all C values of every entry in hand anyway — verifies: bit
 * 8 c + c' is set when channel c differs from channel c' somewhere, compared for every folded
 * channel against its representative and for every packed channel against the channels packed
 * before it (chan_check_host[c] == 0 exempts channel c, e.g. a zero channel stride; NULL = all).  A
 * failed claim means the caller must repack; packed channels that never differed may be folded in
 * the next batch.  chan_src_host == NULL: identity (C <= 8). */
int lnz_large_pack_operators_fold(const float* L, int64_t stride_b, int64_t stride_r,
                                  int64_t stride_c, int64_t stride_ch, const float* V, int B, int N,
                                  int C, int K, int planes, const int32_t* chan_src_host, int n_src,
                                  const int32_t* chan_rep_host, const int32_t* chan_check_host,
                                  unsigned long long* neq, uint16_t* Lb, uint16_t* Vb,
                                  lnz_stream_t stream);
int lnz_large_gemm1(const float* X, int ldx, int din, const uint16_t* Wf, int B, int N, int C,
                    int planes, uint16_t* Zt, lnz_stream_t stream);
int lnz_large_spectral(const float* X, int ldx, int din, const float* V, const float* G,
                       const float* Wt, int B, int N, int K, int S, int planes, float* Ybuf,
                       uint16_t* Tt, lnz_stream_t stream);
int lnz_large_conv(const uint16_t* Lb, const uint16_t* Vb, const uint16_t* Zt, const uint16_t* Tt,
                   const float* bias, int B, int N, int C, int planes, int relu, float* Xout,
                   lnz_stream_t stream);

/* ---- the same layer on the NONZEROS of the Laplacian (csrc/conv_sparse.hip) --------------------
 * The normalised Laplacian of a large sparse graph (config 5: G(n = 2048, p = 0.01), 99 % zeros) is
 * read from HBM once per batch instead of once per layer; planes = 1 (bf16 operands, fp32
 * accumulate: the streamed form's products without the zeros), one operator class (every channel
 * of L equal to channel 0: the reference's single-edge-type collate, dataset/graph_data.py:225-262).
 * A layer = gemm1_rows + spectral + conv(C = 0, relu = 0) + sparse_conv(relu).
 *   lnz_large_sparse_image   L [B,N,N,C] fp32 by element strides -> entries [B][N][row_cap] u32 =
 *                            bf16(value) << 16 | column (rounded to nearest even, as
 *                            lnz_large_pack_operators rounds), counts [B][N] i32: the nonzeros of
 *                            channel 0 row by row (fixed order; zero padded to a multiple of 8 per
 *                            row); values (optional, NULL to skip): the same entries' fp32
 *                            values [B][N][row_cap].  flags (one device int32, cleared by the call): bit 0 = a
 *                            channel differs from channel 0 somewhere, bit 1 = a row holds more
 *                            than row_cap nonzeros (row_cap a multiple of 8, >= 32; N <= 65536).
 *                            A non-zero flag means the image must NOT be used: the caller reads it
 *                            back and takes lnz_large_pack_operators / lnz_large_conv instead.
 *   lnz_large_pack_vectors   Vb alone, exactly as lnz_large_pack_operators writes it.
 *   lnz_large_gemm1_rows     Z [B][N][128] bf16 = X W^T, row major (Wf: the C = 1, planes = 1 form
 *                            of lnz_large_gemm1's fragments, the class's weight blocks summed).
 *   lnz_large_conv, C = 0    the lift alone: Xout = act( Vb Tt^T + bias ) (Lb, Zt may be NULL).
 *   lnz_large_sparse_conv    X [B,N,128] in place: X[r] = act( X[r] + sum_k value[r][k] Z[column[r][k]] ),
 *                            accumulated in fp32 in entry order.  An exact zero of L contributes
 *                            nothing (the streamed kernels multiply it: 0 x inf = NaN there). */
int lnz_large_sparse_image(const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                           int64_t stride_ch, int B, int N, int C, int row_cap, uint32_t* entries,
                           float* values, int32_t* counts, int32_t* flags, lnz_stream_t stream);
int lnz_large_pack_vectors(const float* V, int B, int N, int K, int planes, uint16_t* Vb,
                           lnz_stream_t stream);
int lnz_large_gemm1_rows(const float* X, int ldx, int din, const uint16_t* Wf, int B, int N,
                         uint16_t* Z, lnz_stream_t stream);
int lnz_large_sparse_conv(const uint32_t* entries, const int32_t* counts, int row_cap,
                          const uint16_t* Z, int B, int N, int relu, float* X, lnz_stream_t stream);
/* The readout on the last large-graph conv state (model/lanczos_net_general.py:185-201 /
 * model/lanczos_net.py:185-194): score [B,P] = mean over the real nodes (mask [B,N] != 0) of
 * (W_h x + b_h) * sigmoid(w_g x + b_g); X [B,N,128] fp32, Whead [P + 1][128] = the output Linear's
 * rows then the gate's, bhead [P + 1]; P <= 16.  One pass over X, deterministic. */
int lnz_large_head(const float* X, const uint8_t* mask, const float* Whead, const float* bhead, int B,
                   int N, int P, float* score, lnz_stream_t stream);
/* lnz_large_spectral (planes = 1) and lnz_large_gemm1_rows in one pass over X: the projection's
 * X tile in LDS also yields Z (the same bits as lnz_large_gemm1_rows). */
int lnz_large_spectral_gemm1_rows(const float* X, int ldx, int din, const float* V, const float* G,
                                  const float* Wt, const uint16_t* Wf, int B, int N, int K, int S,
                                  float* Ybuf, uint16_t* Tt, uint16_t* Z, lnz_stream_t stream);
/* The node-space term of the split-precision modes (planes = 2, 3) in EXACT fp32 on the same image:
 * values [B][N][row_cap] fp32 (lnz_large_sparse_image's optional output: the unrounded entries, in
 * the entries' order), Zf [B][N][128] fp32 = X W^T (lnz_f32_linear on the [B N, din] states):
 * X[r] = act( X[r] + sum_k values[r][k] Zf[column[r][k]] ), fp32 fma in entry order.  A layer =
 * lnz_f32_linear + lnz_large_spectral(planes) + lnz_large_conv(C = 0, planes) + this. */
int lnz_large_sparse_conv_f32(const uint32_t* entries, const float* values, const int32_t* counts,
                              int row_cap, const float* Zf, int B, int N, int relu, float* X,
                              lnz_stream_t stream);
/* The backward of that exact-fp32 layer for ONE symmetric operator (an undirected simple graph's L4
 * given as its image: L^T = L), X' = relu( L Z + V T + b ), Z = X Wn^T, Y = V^T X, T = sum_s
 * diag(g_s) Y W_s^T, from the gradient dX' of its output (model/lanczos_net_general.py:157-182 under
 * runner/graph_runner.py's loss.backward()).  All fp32, K <= 64, S <= 16, hidden width 128.
 *   lnz_large_grad_project   dX [B,N,128] in place: dP = dX' * (Xout > 0), rows >= n_nodes[b] (NULL:
 *                            N) exactly zero whatever they held; db [B,128] = the graph's column sums of
 *                            dP; A [B,K,128] = V^T dP on v_mfma_f32_16x16x4_f32.  part: workspace of
 *                            B * ceil(N / 256) * 65 * 128 floats (per 256-row chunk a partial of A and
 *                            of db, added in ascending chunk order by a second launch: no atomics, the
 *                            same bits every time).
 *   (dZ = L dP is lnz_large_sparse_conv_f32 with relu = 0 onto a zeroed buffer.)
 *   lnz_large_grad_spectral  one workgroup per graph.  A [B,K,128], Y [B,K,ldy] (first d columns), G
 *                            [B,S,K], W [128][ldw]: the mix weight, long-scale block s in columns
 *                            [s d, s d + d).  With U_s = A W_s:  dG [B,K,S] (may be NULL) = <U_s[k],
 *                            Y[k]> = sum_o A[k][o] (Y W_s^T)[k][o];  Q [B,K,S,d] = g_s[k] Y[k];
 *                            dY [B,K,128] = sum_s g_s[k] U_s[k] (columns >= d zero).
 *   lnz_large_grad_input     dX [B,N,128] = dZ Wn + V dY, one fp32 MFMA GEMM over the depth 128 + K:
 *                            dZ [B,N,128], Wn [128][128] (Wn[o][i], columns >= d zero), V [B,N,K], dY
 *                            [B,K,128] (K = 0: V, dY may be NULL); columns >= d of dX are written zero.
 *                            dX must not alias dZ. */
int lnz_large_grad_project(float* dX, const float* Xout, const float* V, const int32_t* n_nodes, int B,
                           int N, int K, float* part, float* A, float* db, lnz_stream_t stream);
int lnz_large_grad_spectral(const float* A, const float* Y, int ldy, const float* G, const float* W, int ldw,
                            int B, int K, int S, int d, float* dG, float* Q, float* dY, lnz_stream_t stream);
int lnz_large_grad_input(const float* dZ, const float* Wn, const float* V, const float* dY, int B, int N,
                         int K, int d, float* dX, lnz_stream_t stream);
/* Several operators on the nonzeros: a batch with num_edge_type >= 2, whose collated L [B,N,N,E+1] holds
 * L4 of the simple graph and of every edge type alone (dataset/get_graph_data.py:60-72), and the
 * node-space term  sum_c L_c (X W_c^T)  of model/lanczos_net_general.py:157-182 on R = E + 1 = 2 .. 8
 * images, CHANNEL MAJOR: entries / values [R][B][N][row_cap], counts [R][B][N], each channel in
 * lnz_large_sparse_image's row format.
 *   lnz_large_sparse_image_channels   one pass over a dense L [B,N,N,C] (C <= 8, any strides): image c
 *                            is bit for bit what lnz_large_sparse_image writes for the slice
 *                            L[..., c:c+1] (ascending columns); flags: bit 1 (a row of some channel
 *                            beyond row_cap) only.
 *   lnz_large_sparse_conv_channels    X[r] = act( X[r] + sum_c sum_k value_c[r][k] Z_c[column_c[r][k]] ),
 *                            channels ascending, entries in entry order, ONE fp32 accumulator: a
 *                            fixed function of the images.  Z CLASS MAJOR [R][B][N][128] bf16
 *                            (lnz_large_gemm1_rows once per channel on that channel's fragments).
 *   lnz_large_sparse_conv_channels_f32  the same in exact fp32: values x Zf [R][B][N][128] fp32
 *                            (lnz_f32_linear once per channel).
 * row_cap a multiple of 8, >= 32; N <= 65536; X 8-byte aligned.  A layer = the one-operator layer with
 * R feature launches and this gather (lnz_large_spectral, lnz_large_conv with C = 0 unchanged).  R = 1:
 * lnz_large_sparse_conv / _f32. */
int lnz_large_sparse_image_channels(const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                                    int64_t stride_ch, int B, int N, int C, int row_cap,
                                    uint32_t* entries, float* values, int32_t* counts, int32_t* flags,
                                    lnz_stream_t stream);
int lnz_large_sparse_conv_channels(const uint32_t* entries, const int32_t* counts, int row_cap,
                                   const uint16_t* Z, int B, int N, int R, int relu, float* X,
                                   lnz_stream_t stream);
int lnz_large_sparse_conv_channels_f32(const uint32_t* entries, const float* values,
                                       const int32_t* counts, int row_cap, const float* Zf, int B, int N,
                                       int R, int relu, float* X, lnz_stream_t stream);
/* The backward of that exact-fp32 layer over the R = E + 1 channels, every L_c symmetric (the L4 of an undirected
 * graph with its own degrees):  X' = relu( sum_c L_c Z_c + V T + b ),  Z_c = X Wn_c^T.  With dP of
 * lnz_large_grad_project:  dZ_c = L_c dP,  dWn_c = dZ_c^T X,  dX = sum_c dZ_c Wn_c + V dY; db, A, dG, Q, dY as
 * for one operator (lnz_large_grad_project, lnz_large_grad_spectral).
 *   lnz_large_sparse_conv_split_f32   dZ [R][B][N][128] fp32: dZ[c] = L_c P for ONE source P [B][N][128]
 *                            fp32 and the R images (channel major, with values).  The same gather kernel in
 *                            the same (row, channel) order; dZ is overwritten, never read, no activation:
 *                            channel c's block is bit for bit lnz_large_sparse_conv_f32 of image c with
 *                            relu = 0 onto zeros.  R = 2 .. 8; P, dZ 8-byte aligned, dZ not P.
 *   lnz_large_grad_input_channels     dX [B,N,128] = sum_c dZ_c Wn_c + V dY, one fp32 MFMA GEMM over the depth
 *                            R 128 + K in ascending order: dZ [R][B][N][128], Wn [R][128][128] (Wn[c][o][i],
 *                            columns >= d zero), V [B,N,K], dY [B,K,128] (K = 0: V, dY may be NULL); columns
 *                            >= d of dX are written zero.  1 <= R <= 8 (R = 1: the bits of
 *                            lnz_large_grad_input), K <= 64, d <= 128.  dX must not alias dZ. */
int lnz_large_sparse_conv_split_f32(const uint32_t* entries, const float* values, const int32_t* counts,
                                    int row_cap, const float* P, int B, int N, int R, float* dZ,
                                    lnz_stream_t stream);
int lnz_large_grad_input_channels(const float* dZ, const float* Wn, const float* V, const float* dY, int B,
                                  int N, int K, int R, int d, float* dX, lnz_stream_t stream);
/* That backward forms dZ = L dP for L^T dP: it asks for symmetric operators.  An image from an edge list is
 * symmetric by construction; of an image built from a caller's tensor this entry says so:
 *   lnz_large_sparse_image_symmetry   entries / values / counts: a one-operator image (R = 1) or R channel-major
 *                            images [R][B][N][row_cap]; values required.  status [R * B] int32, cleared by the
 *                            call; word r B + b: bit 0 = an entry (i, j, v) of graph b, channel r, has no entry with
 *                            column i in row j; bit 1 = the mirror's value is not v — they match when the signs
 *                            agree and the bit patterns, as integers, differ by at most 1 (one fp32 ulp: an L built
 *                            in float64 and cast can round (s_i a) s_j and (s_j a) s_i one ulp apart).  A row's
 *                            padding is not an entry, a diagonal entry is its own mirror; rows are searched (entry
 *                            order is not ascending).  Counts are clamped to row_cap and columns >= N never
 *                            followed: safe on an image whose flags are raised (the result is then meaningless).
 *                            R <= 8, N <= 65536, row_cap a multiple of 8, >= 32.  A fixed function of the image. */
int lnz_large_sparse_image_symmetry(const uint32_t* entries, const float* values, const int32_t* counts,
                                    int row_cap, int R, int B, int N, int32_t* status, lnz_stream_t stream);

/* ---- R6 standalone: batched symmetric tridiagonal eigensolver --------------------------------
 * The step the reference leaves to LAPACK (inside np.linalg.eigh, utils/data_helper.py:201) /
 * ARPACK (:208).  diag [B,M], offdiag [B,M-1] (fp64) -> R [B,M] ascending, Bm [B,M,M] with
 * eigenvectors in columns.  Implicit-shift QL (tql2 recurrences), M <= 64. */
int lnz_tridiag_eigh(const double* diag, const double* offdiag, int B, int M, double* R,
                     double* Bm, lnz_stream_t stream);

/* ---- R2 + R6, large graphs (BASELINE config 5: N = 2048, K = 64) -------------------------------
 * M-step Lanczos (full re-orthogonalisation: classical Gram-Schmidt against every previous vector,
 * a second pass where the first removed more than 1 - 1e-6 of |w|^2 or where the carried bound on
 * the loss of orthogonality asks for it (lnz::CgsBound, csrc/wave.hpp: L1, L2, raw adjacencies and
 * evenly spread spectra need it every few steps, L4 Laplacians almost never); stops once |w| falls
 * to 1e-8 times 2^ceil(log2 max |a_ij|): the Krylov space has become invariant, whatever power of
 * two the matrix is scaled by) -> QL on the M x M tridiagonal -> Ritz vectors V = Q S, top-K by |theta|, zero
 * padded.  The dense A (rows contiguous, 16-byte aligned, row stride stride_r, N %% 4 == 0,
 * N <= 2048) is re-streamed from HBM every step: this is the HBM-bound regime of the path.
 * The reference's counterpart is scipy.sparse.linalg.eigsh(L, k, which='LM')
 * (utils/data_helper.py:205-208, ARPACK, implicitly restarted): converged leading pairs agree,
 * unconverged ones are a different function — see oracle/lanczos_kstep.py.
 * workspace: lnz_lanczos_ritz_large_workspace_bytes(B, N) bytes of device memory (the fp64 Krylov
 * basis, B x 64 x N).  D [B,K], V [B,N,K]; info [B] (optional) = Lanczos steps actually taken. */
int64_t lnz_lanczos_ritz_large_workspace_bytes(int B, int N);
int lnz_lanczos_ritz_large(const float* A, int64_t stride_b, int64_t stride_r, int B, int N,
                           int M, int K, void* workspace, float* D, float* V, int32_t* info,
                           lnz_stream_t stream);
/* The same for a SYMMETRIC A (every Laplacian of utils/data_helper.py:92-130 is), reading only
 * the 256 x 256 chunk blocks (I, J >= I): an off-diagonal block serves w_I += A_IJ q_J and
 * w_J += A_IJ^T q_I, 56 %% of the bytes per Lanczos step at N = 2048.  What lies below the diagonal
 * chunk blocks is never read (numpy.linalg.eigh's UPLO convention, upper).  Deterministic (no
 * atomics); same workspace. */
int lnz_lanczos_ritz_large_sym(const float* A, int64_t stride_b, int64_t stride_r, int B, int N,
                               int M, int K, void* workspace, float* D, float* V, int32_t* info,
                               lnz_stream_t stream);

/* The K-step entry of the product surface: what get_graph_laplacian_eigs computes with
 * use_eigen_decomp=False (utils/data_helper.py:205-208: `eigsh(L, k, which='LM')`, a K-dimensional
 * Krylov method instead of the full decomposition) for graphs beyond the 192 nodes
 * lnz_lanczos_ritz serves, ragged batches included: n_nodes [B] (optional; NULL = every graph has
 * N nodes) are the real node counts of zero-padded matrices (dataset/graph_data.py:222-260); the
 * Krylov vectors stay zero on the padding and the recurrence stops after n_b steps by itself.
 * flags:
 *   LNZ_KSTEP_SYMMETRIC  the dense stream reads only the upper 256 x 256 chunk blocks
 *                        (= lnz_lanczos_ritz_large_sym; otherwise = lnz_lanczos_ritz_large);
 *   LNZ_KSTEP_COMPACT    A is read from HBM ONCE: a first launch (one wavefront per row) gathers the
 *                        nonzeros of every 64-row slab into a sliced-ELL image in the workspace (row_cap entries per
 *                        row at most, a multiple of 8), and the M steps multiply by that image —
 *                        the Laplacian of a G(n, 0.01) graph is 99 %% zeros and skipping an exact
 *                        zero changes no sum.  A graph with a longer row is computed by the dense
 *                        stream in the same call (dense_fallback [B], optional output: 1 for such
 *                        a graph).  The FULL matrix is read (no UPLO convention in this mode).
 * stride_c (elements between the columns of a row): 1, or — with LNZ_KSTEP_COMPACT and a
 * dense_fallback output — 2: A is channel 0 of a channels-last [N][N][2] block, the collated
 * `L[..., 0]` of dataset/graph_data.py:225-262 read in place (N even; one float4 = two columns x
 * two channels).  The dense streams need contiguous rows: with stride_c = 2 a graph flagged in
 * dense_fallback is NOT computed — the caller copies such a batch and calls again.
 * Same algorithm, arithmetic and outputs as lnz_lanczos_ritz_large; the three SpMV variants differ
 * in the order of their fp64 additions only.  Deterministic. */
#define LNZ_KSTEP_SYMMETRIC 1
#define LNZ_KSTEP_COMPACT 2
int64_t lnz_lanczos_ritz_kstep_workspace_bytes(int B, int N, int flags, int row_cap);
int lnz_lanczos_ritz_kstep(const float* A, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                           const int32_t* n_nodes, int B, int N, int M, int K, int flags,
                           int row_cap, void* workspace, int64_t workspace_bytes, float* D, float* V,
                           int32_t* info, int32_t* dense_fallback, lnz_stream_t stream);

/* The same function — utils/data_helper.py:205-208, `eigsh(L, k, which='LM')`; the M-step recurrence
 * of lnz_lanczos_ritz_kstep, Ritz pairs in the same order with the same padding, info [B] = steps
 * taken — for what one workgroup cannot hold: N <= 16384 nodes and K <= M <= 256 Lanczos steps
 * (M <= N; LNZ_ENOTSUP beyond), M > K included: a Krylov space wider than the pairs kept, the knob
 * the reference's ARPACK call has (csrc/lanczos_wide.hip).  A graph is spread over many workgroups;
 * the stages are ordered by launch boundaries (5 M + 8 launches per call), the early stop and the
 * second Gram-Schmidt pass are decided on the device, every sum has a fixed order: deterministic,
 * and a graph's result does not depend on the rest of the batch.  A is always read once into the
 * sliced-ELL image (row_cap as LNZ_KSTEP_COMPACT); a graph with a longer row (dense_fallback [B],
 * optional output) is multiplied from its dense rows in the same call.  stride_c = 1, or 2 with a
 * dense_fallback output: channel 0 of the collated channels-last pair in place — a graph flagged
 * there is NOT computed (the caller copies such a batch and calls again), as above.  Rows 16-byte
 * aligned, N %% 4 == 0, one graph spans less than 4 GiB.  workspace (256-B aligned):
 * lnz_lanczos_ritz_kstep_wide_workspace_bytes(B, N, M, row_cap) bytes, linear in B (0 for
 * non-positive sizes); B <= 65535 per call. */
int64_t lnz_lanczos_ritz_kstep_wide_workspace_bytes(int B, int N, int M, int row_cap);
int lnz_lanczos_ritz_kstep_wide(const float* A, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                                const int32_t* n_nodes, int B, int N, int M, int K, int row_cap,
                                void* workspace, int64_t workspace_bytes, float* D, float* V,
                                int32_t* info, int32_t* dense_fallback, lnz_stream_t stream);

/* The FULL decomposition of get_graph_laplacian_eigs(..., use_eigen_decomp=True)
 * (utils/data_helper.py:197-223: `np.linalg.eigh` of each graph's n_b x n_b block, then the top-K
 * |lambda| cut) for graphs of up to 2048 nodes, ragged batches included (csrc/sym_eigh.hip).
 * A [B][N][N] float32 with arbitrary strides (stride_c = 2: channel 0 of the collated channels-last
 * [N][N][2] Laplacian, read in place); only the LOWER triangle of the n_b x n_b block is read
 * (numpy's UPLO='L'), the strict upper triangle and rows / columns >= n_b never.  n_nodes [B]
 * (optional; NULL = N for every graph).  fp64 Householder tridiagonalisation (blocked, latrd
 * panels), Sturm bisection + inverse iteration on the tridiagonal, blocked back-transformation.
 * Outputs like every Ritz-pair entry: D [B][K], V [B][N][K] in stable descending-|lambda| order
 * over ascending lambda (a negative eigenvalue first on an exact tie), the first entry of largest
 * magnitude of each column positive, D[b][k] = 0 and V[b][:][k] = 0 for k >= n_b, V[b][n_b:][:] = 0.
 * info [B] (optional): 0 = converged; 1 = the input block was not finite (D, V zero); 2 = an
 * inverse iteration did not converge.  Deterministic, and a graph's result does not depend on the
 * rest of the batch.  Limits: N <= 2048, K <= 256 (LNZ_ENOTSUP beyond); K >= 1 and B <= 65535 per
 * call (LNZ_EINVAL otherwise).  The workspace (256-B aligned) grows linearly in B: a caller with a
 * large batch calls once per chunk. */
int64_t lnz_sym_eigh_topk_workspace_bytes(int B, int N, int K);
int lnz_sym_eigh_topk(const float* A, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                      const int32_t* n_nodes, int B, int N, int K, void* workspace,
                      int64_t workspace_bytes, float* D, float* V, int32_t* info, lnz_stream_t stream);

/* The same call leaving the image of lnz_large_sparse_image behind (csrc/conv_sparse.hip): the
 * compaction pass has every entry of the row in hand (and, with stride_c = 2, the second channel of
 * the collated pair), so conv_entries [B][N][conv_row_cap] (+ conv_values, optional: the unrounded
 * fp32 values of the exact form) / conv_counts [B][N] / conv_flags (one
 * int32: bit 0 = the two channels differ somewhere — stride_c = 2 only; with stride_c = 1 the
 * caller vouches for a single operator —, bit 1 = a row beyond conv_row_cap) cost no second read of
 * L: one pass over the collated Laplacian per batch serves the Ritz pairs and all conv layers.
 * LNZ_KSTEP_COMPACT required; conv_row_cap a multiple of 8, at least 32. */
int lnz_lanczos_ritz_kstep_image(const float* A, int64_t stride_b, int64_t stride_r,
                                 int64_t stride_c, const int32_t* n_nodes, int B, int N, int M, int K,
                                 int flags, int row_cap, void* workspace, int64_t workspace_bytes,
                                 float* D, float* V, int32_t* info, int32_t* dense_fallback,
                                 uint32_t* conv_entries, float* conv_values, int32_t* conv_counts,
                                 int conv_row_cap, int32_t* conv_flags, lnz_stream_t stream);

/* ---- large graphs from edge lists (csrc/edge_image.hip) ----------------------------------------
 * The images the K-step recurrence and the sparse conv run on, built from a batch of undirected EDGE
 * LISTS instead of the dense collated Laplacian: no array of N x N elements is read or written.
 * Replaces, for unweighted simple graphs with ONE edge type (the reference's graph configuration,
 * num_edge_type: 1), utils/data_helper.py:92-116,155-156 (normalize_adj / get_laplacian 'L4'),
 * dataset/get_graph_data.py:61-72 (the offline L4 + eigen pairs of every graph) and the `eigsh`
 * branch utils/data_helper.py:205-223.
 *   edges [n_edges][2] int32   local node ids, each undirected edge once, either endpoint order
 *   edge_off [B + 1] int64     graph b owns edges [edge_off[b], edge_off[b + 1])
 *   n_nodes [B] int32          rows >= n_nodes[b] are empty
 * Entry (i, j) = (float)((s_i * 1.0) * s_j), s_i = 1.0 / sqrt((double)deg_i), deg_i = 1 + neighbours
 * — lnz_laplacian_l4's expression —, the diagonal present in every real row.  The recurrence and the
 * gather sum a row in ENTRY order, and the dense compaction meets a row's nonzeros in the order of its
 * vector loads (64 float4s per wave, component by component), so the order is an argument:
 *   LNZ_EDGE_ORDER_ASCENDING  ascending column (lnz_large_sparse_image's 4-byte form: odd N, any strides)
 *   LNZ_EDGE_ORDER_PAIR       within every 128 columns the even ones, then the odd ones (the
 *                             channels-last pair read in place, stride_c = 2: N even / N %% 4 == 0)
 *   LNZ_EDGE_ORDER_QUAD       within every 256 columns, column %% 4 == 0, then 1, 2, 3 (contiguous rows)
 * With the order of the dense form it stands in for, an image is bit for bit the one
 * lnz_lanczos_ritz_kstep_image / lnz_large_sparse_image gathers from the dense L4 of the same
 * graphs, whatever the order of the edges and of their endpoints (integer atomics only).
 * status [B] (output): 0, or the OR of 1 = an endpoint outside [0, n_b), 2 = a self loop, 4 = a
 * duplicate edge, 8 = edge_off[b] .. edge_off[b + 1] is not a range inside the edge array, 16 =
 * n_nodes[b] outside [0, N].  Checked on the device before any indexed access; such a graph's
 * outputs are zeros (counts, entries, D, V, info) and nothing is written outside its own slots.
 * (A duplicate inside a row of more than max(row_cap, conv_row_cap) entries is not looked for: that
 * graph is reported in `fallback` / conv_flags instead.)
 * A row of more than row_cap entries is not an error: fallback [B] (optional output) = 1 and the
 * graph's D, V, info are ZERO — there is no dense A to fall back on; the caller densifies such a
 * batch.  A row of more than conv_row_cap entries raises conv_flags bit 1 (bit 0 never: both channels
 * of a one-edge-type L are one operator by construction).
 * The Ritz pairs are those of lnz_lanczos_ritz_kstep (N <= 2048, K <= M <= 64) /
 * lnz_lanczos_ritz_kstep_wide (N <= 16384, K <= M <= 256) with LNZ_KSTEP_COMPACT on that image: the
 * same step kernels, unchanged.  N %% 4 == 0 (pad the batch); row_cap a multiple of 8 in [8, 256];
 * the conv image is optional (conv_entries NULL: none; else conv_row_cap a multiple of 8 in
 * [32, 256], conv_values optional).  workspace: 256-B aligned, *_workspace_bytes(...) bytes
 * (conv_row_cap = 0 without a conv image). */
#define LNZ_EDGE_ORDER_ASCENDING 0
#define LNZ_EDGE_ORDER_PAIR 1
#define LNZ_EDGE_ORDER_QUAD 2
int64_t lnz_lanczos_ritz_kstep_edges_workspace_bytes(int B, int N, int row_cap, int conv_row_cap);
int lnz_lanczos_ritz_kstep_edges(const int32_t* edges, int64_t n_edges, const int64_t* edge_off,
                                 const int32_t* n_nodes, int B, int N, int M, int K, int row_cap,
                                 int row_order, void* workspace, int64_t workspace_bytes, float* D,
                                 float* V, int32_t* info, int32_t* fallback, uint32_t* conv_entries,
                                 float* conv_values, int32_t* conv_counts, int conv_row_cap,
                                 int conv_order, int32_t* conv_flags, int32_t* status,
                                 lnz_stream_t stream);
int64_t lnz_lanczos_ritz_kstep_wide_edges_workspace_bytes(int B, int N, int M, int row_cap,
                                                          int conv_row_cap);
int lnz_lanczos_ritz_kstep_wide_edges(const int32_t* edges, int64_t n_edges, const int64_t* edge_off,
                                      const int32_t* n_nodes, int B, int N, int M, int K, int row_cap,
                                      int row_order, void* workspace, int64_t workspace_bytes, float* D,
                                      float* V, int32_t* info, int32_t* fallback, uint32_t* conv_entries,
                                      float* conv_values, int32_t* conv_counts, int conv_row_cap,
                                      int conv_order, int32_t* conv_flags, int32_t* status,
                                      lnz_stream_t stream);
/* The conv image alone (lnz_large_sparse_image's format), for callers that already hold (D, V): any
 * N <= 16384; workspace 16-B aligned. */
int64_t lnz_laplacian_l4_edges_image_workspace_bytes(int B, int N, int conv_row_cap);
int lnz_laplacian_l4_edges_image(const int32_t* edges, int64_t n_edges, const int64_t* edge_off,
                                 const int32_t* n_nodes, int B, int N, void* workspace,
                                 int64_t workspace_bytes, uint32_t* conv_entries, float* conv_values,
                                 int32_t* conv_counts, int conv_row_cap, int conv_order,
                                 int32_t* conv_flags, int32_t* status, lnz_stream_t stream);
/* The conv images of a TYPED batch (num_edge_type = E in 2 .. 7: E + 1 <= 8 operator channels), replacing
 * utils/data_helper.py:92-116,155-156,261-293 and dataset/get_graph_data.py:60-72 for unweighted simple
 * graphs whose every node pair carries at most one edge, of one type: edge_type [n_edges] int32 in
 * [0, E) beside `edges`.  Channel 0 = all neighbours + the diagonal (the image lnz_laplacian_l4_edges_image
 * builds for the same edge set), channel 1 + e = the type-e neighbours + the diagonal with
 * deg = 1 + the node's type-e neighbours (a live node without a type-e edge: the single entry (i, 1.0f));
 * CHANNEL MAJOR conv_entries / conv_values [E+1][B][N][conv_row_cap], conv_counts [E+1][B][N], every
 * channel in LNZ_EDGE_ORDER_ASCENDING — bit for bit what lnz_large_sparse_image writes for the slice
 * L[..., c:c+1] of the dense lnz_laplacian_l4 tensor.  status as above, plus 32 = an edge type outside
 * [0, E); the same pair listed twice, with equal or different types, is status 4.  conv_flags bit 1 is
 * decided on channel 0.  Integer atomics only; every word is a function of the typed edge SET.  The Ritz
 * pairs of such a batch are those of channel 0: lnz_lanczos_ritz_kstep_edges / _wide_edges on `edges`
 * alone (conv_entries NULL, row_order LNZ_EDGE_ORDER_QUAD: the dense route copies L[..., 0] of an
 * [B,N,N,E+1] tensor to contiguous rows).  workspace 16-B aligned. */
int64_t lnz_laplacian_l4_typed_edges_images_workspace_bytes(int B, int N, int num_edge_type,
                                                            int conv_row_cap);
int lnz_laplacian_l4_typed_edges_images(const int32_t* edges, const int32_t* edge_type, int64_t n_edges,
                                        const int64_t* edge_off, const int32_t* n_nodes, int B, int N,
                                        int num_edge_type, void* workspace, int64_t workspace_bytes,
                                        uint32_t* conv_entries, float* conv_values, int32_t* conv_counts,
                                        int conv_row_cap, int32_t* conv_flags, int32_t* status,
                                        lnz_stream_t stream);

/* A HIP stream whose kernels run on compute units [first_cu, end_cu) of the current device only
 * (hipExtStreamCreateWithCUMask).  For latency-chain launches that fill a fraction of the chip —
 * the workgroup-per-graph Ritz launch of the reference's graph configuration keeps 64 of 256
 * compute units busy for 0.45 ms — next to the previous batch's forward: on shared compute units
 * the forward's waves stretch the chain to 0.60 ms and the overlap buys nothing; on disjoint ones a
 * batch of the stream takes 0.50 instead of 0.67 ms.  The stream is the caller's
 * (hipStreamDestroy). */
int lnz_stream_create_cu_masked(int first_cu, int end_cu, lnz_stream_t* stream);

/* ---- operand packing (MFMA fragment order) -------------------------------------------
 * W [rows, cols] (leading dimension ld) -> Wp[rt][q][lane][u] =
 *   W[32*rt + (lane&31)][8*q + 4*(lane>>5) + u], zero padded to rows%32==0, cols%8==0.
 * One float4 per lane per (rt, q): the A- or B-operand stream of v_mfma_f32_32x32x2_f32
 * for four consecutive k-steps.  Wp holds lnz_packed_rows_k8_size(rows, cols) floats. */
int64_t lnz_packed_rows_k8_size(int rows, int cols);
int lnz_pack_rows_k8(const float* W, int rows, int cols, int64_t ld, float* Wp,
                     lnz_stream_t stream);
/* The same stream for the split-precision GEMM1 of the strip kernel (lnz_forward_args.gemm_mode =
 * 1): same size (lnz_packed_rows_k8_size; cols a multiple of 32) and the same (rt, 16-k step, lane)
 * indexing, but the two 16-byte slots a lane owns in a 32-k block b hold eight fp16 hi pieces, then
 * the eight lo pieces (x = hi + lo to 22 bits) of W[32 rt + wj][32 b + 8 kq + 0..7] (lane slot
 * 64 (kq >> 1) + 32 (kq & 1) + wj) — the B operands of v_mfma_f32_16x16x32_f16. */
int lnz_pack_rows_k8_split(const float* W, int rows, int cols, int64_t ld, float* Wp,
                           lnz_stream_t stream);
/* Folded weights of the rare bond-type channels for the strip forward (lnz_forward_args.Wf), from the
 * conv pack Wp / w_off (floats, per layer) of a model with hidden width dhid (a multiple of 32), layer-0
 * input width din0 (a multiple of 16), C = n_short + n_long + n_edge channels, 3 <= n_edge:
 *   Wf[layer l][rt][q][lane] (float4) = 0.f + Wp[l][rt][channel n_short + n_long + 2][q][lane] + ... +
 *   Wp[l][rt][channel C - 1][q][lane], element-wise in fp32, channels ascending
 * — one channel's fragment order (rt < dhid / 32, q < din_l / 8, 64 lanes), the layers back to back
 * (dhid * din_l floats each), then 2048 floats of zero slack (the weight ring of the strip kernel reads
 * up to three 16-k steps ahead).  Wf holds lnz_pack_fold_weights_size(num_layer, din0, dhid) floats;
 * every one of them is written. */
int64_t lnz_pack_fold_weights_size(int num_layer, int din0, int dhid);
int lnz_pack_fold_weights(const float* Wp, const int64_t* w_off_host, int num_layer, int din0, int dhid,
                          int n_short, int n_long, int n_edge, float* Wf, lnz_stream_t stream);
/* bias [rows] -> bp[rt][lane][r] = bias[32*rt + (r&3) + 8*(r>>2) + 4*(lane>>5)] (the C/D
 * row of accumulator register r); holds 32*ceil(rows/32)*32 floats. */
int lnz_pack_bias_rows(const float* bias, int rows, float* bp, lnz_stream_t stream);
/* L [B,N,N,C] addressed by element strides -> Lp[b][c][g][lane][u] =
 *   L[b][lane&31][8*g + 4*(lane>>5) + u][c], zero padded to the 32 x 32 tile (N <= 32).
 * Replaces the per-slice `L[:, :, :, ii]` strided-view clones of model/lanczos_net.py:172-178. */
int lnz_pack_laplacian(const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                       int64_t stride_ch, int B, int N, int C, float* Lp, lnz_stream_t stream);
/* Same, plus ident [B] uint32 (may be NULL): bit c is set when channel c of molecule b is an
 * identity on its nodes — the tile is diag(0/1): L4 of a bond type the molecule does not contain
 * (utils/data_helper.py:92-116 on an empty A_e) — so that lnz_lanczosnet_forward can add Z_c
 * instead of multiplying by M_c (lnz_forward_args.ident).  The ident argument of
 * lnz_pack_laplacian_plan / lnz_prepare_batch[_gains] is the same array. */
int lnz_pack_laplacian_ident(const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                             int64_t stride_ch, int B, int N, int C, float* Lp, uint32_t* ident,
                             lnz_stream_t stream);

/* ---- R7 (first half): per-eigenvalue spectral filter gains ----------------------------
 * G[l][b][s][k] = MLP_l([D^p_1 .. D^p_S])_s for every conv layer l — the
 * `spectral_filter[layer_idx]` Sequential (Linear S->128, ReLU, 128->128, ReLU, 128->128,
 * ReLU, 128->S) of model/lanczos_net.py:48-60,110-113, with the powers of :146-149.
 * mlp_pack: per layer, lnz_spectral_mlp_pack_size(S) floats written by
 * lnz_pack_spectral_mlp().  dist_host: S integer exponents (host memory).
 * kind 0 = 'MLP'; kind 1 = plain powers G = D^p (the non-MLP branch, :118-121; mlp_pack unused).
 * D [B,K]; G [num_layer,B,S,K].
 * The pack ends in two images of W0 and W6 for the compact form of the first and the last Linear
 * (the default; LNZ_GAINS_COMPACT=0, read once per process, selects the padded form, which does
 * not read them): behind the prefetch slack, nothing in front of them moved and the size grew by
 * 3072 floats.  lnz_spectral_mlp_pack_source() states where float f of those images comes from:
 * the flat index i into the row-major W0 [128,S], returned as i, or into W6 [S,128], returned
 * as 2^32 + i; -1: the float is zero; -2: f lies outside the two images.  Host only, no GPU. */
int64_t lnz_spectral_mlp_pack_size(int S);
int64_t lnz_spectral_mlp_pack_source(int S, int64_t f);
int lnz_pack_spectral_mlp(const float* W0, const float* b0, const float* W2, const float* b2,
                          const float* W4, const float* b4, const float* W6, const float* b6,
                          int S, float* pack, lnz_stream_t stream);
/* Same packs for ALL conv layers in one launch: ptrs[l*8 + {0..7}] = W0, b0, W2, b2, W4, b4, W6, b6
 * of layer l (host array of device pointers); pack holds num_layer consecutive layer packs. */
int lnz_pack_spectral_mlp_layers(const float* const* ptrs, int num_layer, int S, float* pack,
                                 lnz_stream_t stream);
int lnz_spectral_gains(const float* D, int B, int K, const int32_t* dist_host, int S,
                       int num_layer, int kind, const float* mlp_pack, float* G,
                       lnz_stream_t stream);
/* Same, but (kind 0) only for the rows listed in rows[0 .. *n_rows) (device memory, from
 * lnz_plan_batch); every other entry of G is left untouched — zero-initialise G.  rows NULL =
 * lnz_spectral_gains. */
int lnz_spectral_gains_rows(const float* D, int B, int K, const int32_t* dist_host, int S,
                            int num_layer, int kind, const float* mlp_pack, const int32_t* rows,
                            const int32_t* n_rows, float* G, lnz_stream_t stream);

/* Training: parameter gradients of the spectral-filter MLPs of ALL conv layers from dG (the output of
 * lnz_lanczosnet_gain_grad viewed as [num_layer][B*K][S]) in one launch — replaces autograd through
 * the `spectral_filter[l]` Sequentials (model/lanczos_net.py:95-123,146-149: Linear(S,128), ReLU,
 * Linear(128,128), ReLU, Linear(128,128), ReLU, Linear(128,S)).  ptrs[l*8 + {0..7}] = W0, b0, W2, b2,
 * W4, b4, W6, b6 of layer l as for lnz_pack_spectral_mlp_layers (raw row-major parameters; b6 is not
 * read).  rows / n_rows: the live eigen rows of lnz_plan_batch (NULL, NULL = every row of D); rows
 * of dG outside that list are not read.  Every one of the `parts` workgroups of a layer (parts <=
 * lnz_spectral_mlp_grad_parts(rows upper bound, num_layer, n_cu)) writes ONE partial of T =
 * lnz_spectral_mlp_grad_floats(S) floats into partials [L][parts][T]:
 *   dW0 [128][S] | dW2 [128][128] | dW4 [128][128] | dW6 [S][128] | db0, db2, db4 [3][128] | db6 [S] | pad
 * and the gradients are the sum of a layer's partials over the `parts` index (any fixed order: one
 * reduction for all eight).  S <= 8; exact fp32.
 * Contracts the tests pin (tests/test_gpu_mlp_grad_edges.py): entries of `rows` at or beyond *n_rows
 * are never read; a workgroup whose part index owns no 64-row tile (parts > tiles) writes a partial
 * of zeros, so `partials` needs no initialisation; D and the listed rows of dG must be finite (a
 * row's features are D^p: 0 for an underflowing power, which is a valid input). */
int lnz_spectral_mlp_grad_floats(int S);
int lnz_spectral_mlp_grad_parts(int n_rows_max, int num_layer, int n_cu);
int lnz_spectral_mlp_grad(const float* D, int B, int K, const int32_t* dist_host, int S,
                          int num_layer, const int32_t* rows, const int32_t* n_rows, const float* dG,
                          const float* const* ptrs, int parts, float* partials, lnz_stream_t stream);

/* Training: the embedding table's gradient dE[a][c] = sum over the node rows (b, i) with ids[b][i] == a
 * (clamped to [0, num_atom) as the forward clamps) of dx[b * mol_stride + i * row_stride + c], c <
 * width — autograd's embedding backward (model/lanczos_net.py:154), without atomics: workgroup
 * (a, chunk) writes partials[chunk][a][width], the gradient is their sum over `chunks` (any fixed
 * order).  ids [B, N] int64; width in {16, 32, 64, 128}; strides in floats, multiples of 4.
 * lnz_last_kernel() names embedding_grad_kernel<CPL> (CPL columns per lane: 1 up to width 64, else 2). */
int lnz_embedding_grad(const int64_t* ids, int B, int N, const float* dx, int64_t mol_stride,
                       int64_t row_stride, int width, int num_atom, int chunks, float* partials,
                       lnz_stream_t stream);

/* ... and, riding along with the MLP launch (kind 0), the conversion of the batch's packed Laplacian
 * (lp_floats floats at Lp_split, e.g. B * C * 1024 of lnz_pack_laplacian*) into the form the
 * split-precision forward reads (lnz_forward_args.gemm_mode = 1), IN PLACE: every fragment float4
 * becomes 4 fp16 hi pieces | 4 lo pieces.  The launch sits between the pack and the forward anyway
 * and is bound by the matrix pipe; the conversion's workgroups run behind the MLP's.  Lp_split NULL
 * = lnz_spectral_gains_rows.  lnz_split_laplacian_pack is the same conversion as a launch of its
 * own (models without spectral MLPs).  A converted pack is of no use to gemm_mode 0. */
int lnz_spectral_gains_rows_split(const float* D, int B, int K, const int32_t* dist_host, int S,
                                  int num_layer, int kind, const float* mlp_pack, const int32_t* rows,
                                  const int32_t* n_rows, float* G, float* Lp_split, int64_t lp_floats,
                                  lnz_stream_t stream);
int lnz_split_laplacian_pack(float* Lp, int64_t n_floats, lnz_stream_t stream);
/* The same two conversions OUT OF PLACE, into `dst` (lp_floats * 4 bytes; the same bytes are moved):
 * the fp32 pack stays what it was, and a host that types `dst` as 2-byte elements carries the format
 * in the data's type instead of in a flag beside it (what lanczosnet_amd/ops.py does since r06).
 * dst == Lp is the in-place form above. */
int lnz_spectral_gains_rows_split_to(const float* D, int B, int K, const int32_t* dist_host, int S,
                                     int num_layer, int kind, const float* mlp_pack,
                                     const int32_t* rows, const int32_t* n_rows, float* G,
                                     const float* Lp_split, uint16_t* Lp_dst, int64_t lp_floats,
                                     lnz_stream_t stream);
int lnz_split_laplacian_pack_to(const float* Lp, int64_t n_floats, uint16_t* dst, lnz_stream_t stream);

/* ---- R7 (second half) + R9 + R10: fused LanczosNet forward ------------------------------
 * One workgroup per molecule runs the whole network on chip: embedding gather, then per conv
 * layer  X' = relu( sum_c M_c X W_c^T + b )  with M_c in message order
 *   short  : L[...,0]^p                       (model/lanczos_net.py:164-169)
 *   long   : V diag(G[l,:,s,:]) V^T           (:114-117 + :172-174)
 *   edge   : L[...,e], e = 0..E               (:177-178)
 * evaluated as M_c (X W_c^T) so that `cat` (:180) and the [B,N,N,S] filter stack (:123) never
 * exist, then the head  y = sigmoid(X w_a + b_a) * (X W_o^T + b_o)  (:185-188) and the masked
 * mean over real nodes (:190-194).  fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulate.
 * Also serves LanczosNetGeneral (model/lanczos_net_general.py:156): pass node_feat_f. */
typedef struct lnz_forward_args {
  int32_t B, N, K;            /* batch, padded node count (<= 32), eigen slots (<= 32)      */
  int32_t num_layer;          /* conv layers, head excluded (<= 16)                          */
  int32_t din0, dhid, dout;   /* input width (%8==0, <=128), hidden width (64|128), head P (<=31) */
  int32_t n_short, n_long, n_edge;      /* channel counts (n_edge = E+1)                    */
  int32_t short_dist[8];      /* powers p of the short channels                              */
  const int64_t* node_feat;   /* [B,N] atom ids (embedding path) or NULL                     */
  const float* node_feat_f;   /* [B,N,din0] float features (General path) or NULL           */
  const float* embedding;     /* [num_atom, din0]                                            */
  int32_t num_atom;
  int32_t filter_kind;        /* 0 = LanczosNet diagonal gains, 1 = AdaLanczosNet dense filters    */
  const uint8_t* mask;        /* [B,N] 1 = real node                                         */
  const float* Lp;            /* lnz_pack_laplacian output, C = n_edge                       */
  const float* V;             /* [B,N,K]                                                     */
  const float* G;             /* filter_kind 0: [num_layer,B,n_long,K] from lnz_spectral_gains (V = Ritz
                                 vectors); filter_kind 1: dense [num_layer,B,n_long,K,K] from
                                 lnz_ada_symmetrize_filters (V = Lanczos basis Q): M = Q DD Q^T     */
  const float* Wp;            /* packed conv weights: layer l at Wp + w_off[l]               */
  const float* bias;          /* conv biases: layer l at bias + b_off[l], dhid floats        */
  int64_t w_off[16];
  int64_t b_off[16];
  const float* Wp_head;       /* packed [32, dhid]: rows 0..P-1 = filter[-1], row P = att    */
  const float* bias_head;     /* [32]: b_o (P), b_a, zeros                                   */
  float* score;               /* [B,dout]                                                    */
  float* state_out;           /* optional [B,32,dhid] final node state (debug/tests) or NULL */
  /* ---- gemm_mode = 0 (default): the exact fp32 path.  gemm_mode = 1: opt-in split precision on the
   * STRIP plan (inference forward only; needs `strips`, dhid 128, din0 128 — zero-pad narrower inputs
   * and the layer-0 weight columns —, diagonal gains, no short-diffusion channels): X W_c^T as x_hi
   * w_hi + x_lo w_hi + x_hi w_lo with fp16 pieces (x = hi + lo to 22 bits) on
   * v_mfma_f32_16x16x32_f16, fp32 accumulate; Wp = lnz_pack_rows_k8_split of the same matrices at the
   * same offsets, followed by 32 KiB of slack (the weight ring over-reads 16 KiB); the node state
   * lives in LDS as fp16 hi | lo blocks; the products with the Laplacian blocks and the Ritz blocks
   * (projection, lift) run in the same three-product split: V is the exact kernel's (split once per
   * launch), Lp is the exact kernel's pack converted in place by lnz_spectral_gains_rows_split /
   * lnz_split_laplacian_pack; gains, biases, activations and the head are exact fp32.  Measured
   * 1e-6 .. 2e-6 against float64 (exact path: 2e-7 .. 3e-7); parity bar 1e-5. */
  int32_t gemm_mode;
  const int32_t* plan;        /* optional tile plan (lnz_plan_tiles): [plan_wg_cap][4][3] int32, slot s
                                 of workgroup g = (molecule A, molecule B or -1, split row); NULL =
                                 one tile per molecule, 4 per workgroup, in batch order.  The plan
                                 changes the time, and the scores only by fp32 re-association
                                 (<= 1e-6 relative; tested at 1e-5).  Pair tiles (B >= 0) exist in
                                 every kernel that reads the tile plan: diagonal gains and dense
                                 filters in eigen space, both widths (the strip kernels, gemm_mode 1
                                 among them, read `strips` instead).                                 */
  const int32_t* n_wg;        /* device scalar written by lnz_plan_tiles: workgroups in use          */
  int plan_wg_cap;            /* lnz_plan_wg_cap(B, n_cu): workgroup entries in `plan` (= grid size) */
  /* ---- training (gemm_mode 0, filter_kind 0, dhid 128).  All buffers are
   * molecule-major [.., B, 32, dhid] fp32 and must be ZERO-INITIALISED by the caller (rows a
   * molecule does not own in its tile are never written). */
  float* act_out;             /* lnz_lanczosnet_forward: optional [num_layer,B,32,dhid]; slot l receives
                                 X_{l+1} = relu(conv layer l) — the activations the backward needs  */
  const float* act;           /* input_grad / messages: the act_out of the forward                   */
  float* dy;                  /* input_grad: [num_layer,B,32,dhid]; slot num_layer-1 holds, on entry,
                                 dLoss/dY of the last conv layer (pre-activation); slots l-1 are
                                 written with dLoss/dY_{l-1} for l = num_layer-1 .. 1              */
  float* dx0;                 /* input_grad: [B,32,bwd_din0] dLoss/dX_0 (embedding gradient rows)    */
  int32_t bwd_din0;           /* input_grad: width of X_0 (the model's input_dim, multiple of 32)    */
  const float* x0;            /* messages, layer 0: X_0 [B,32,din0] (rows >= n zero)                 */
  float* msg;                 /* messages: [B*32, C*d] with d = din0 (layer 0) or dhid: row
                                 (b*32 + node), column c*d + i = (M_c X_l)[node][i] — the reference's
                                 cat(msg) (model/lanczos_net.py:164-180)                           */
  int32_t msg_layer;          /* messages: the conv layer l whose messages are built                 */
  const uint32_t* ident;      /* forward, optional [B] (lnz_pack_laplacian_ident): edge-type channels
                                 that are identities on a molecule skip their Laplacian fragments
                                 and GEMM2 (out += Z_c; same bits on the real nodes)               */
  const int64_t* row_off;     /* messages, optional [B]: first row of each molecule in a COMPACT msg
                                 (real nodes only: row_off = exclusive scan of the node counts, rows
                                 >= n are not written); NULL = row b*32 + node                     */
  float* dgains;              /* gain_grad: [num_layer,B,K,n_long] dLoss/dG, ZERO-INITIALISED by the
                                 caller (slots beyond a molecule's row block in a shared tile are
                                 dead, k >= n, and are not written)                                */
  /* ---- input_grad, optional (ABI 4): what the weight / bias gradients need, produced where the
   * values are in registers anyway instead of by separate gather and reduction launches */
  float* dy_compact;          /* [num_layer][dy_compact_rows][dhid]: slots 0 .. num_layer-2 receive
                                 dLoss/dY_l in the COMPACT row numbering of `row_off` (real nodes
                                 only: row_off[molecule] + node) — the row order of the compact
                                 message matrix, so dW_l = dy_compact[l]^T msg_l needs no gather.
                                 Needs row_off.  Slot num_layer-1 (the incoming gradient) is the
                                 caller's.                                                          */
  int64_t dy_compact_rows;    /* rows per slot of dy_compact                                         */
  float* dbias_part;          /* [2 * plan_wg_cap][num_layer][dhid], ZERO-INITIALISED: entry (2 g + h,
                                 l) = column sums of dLoss/dY_l over the node tiles of half h of
                                 workgroup g, for l = 0 .. num_layer-2; their sum over the first
                                 index (any fixed order) is the bias gradient of conv layer l      */
  int32_t dbias_part_cap;     /* entries (first index) of dbias_part; 0 = 2 * plan_wg_cap.  The pass
                                 runs on the strip plan, one entry per strip: a launch whose
                                 strip_cap exceeds it is refused                                   */
  /* ---- strip plan of lnz_plan_strips (ABI 5).  With it the width-128 launches run on strips of
   * 16-row subtiles (conv_strip.hip): the forward (inference and training, both GEMM modes), the
   * input-gradient pass (see dbias_part_cap), the message pass and the gain-gradient pass.  The
   * training forward (act_out), gemm_mode 1, the input-gradient pass and the message pass exist on
   * strips only and are refused without them; an inference forward without strips runs on 32-row
   * tiles, and the gain-gradient pass without strips on 32-row tiles too. */
  const int32_t* strips;      /* [strip_cap][LNZ_STRIP_INTS] int32                                   */
  const int32_t* n_strips;    /* device scalar: strips in use                                        */
  int strip_cap;              /* lnz_strip_cap(B): entries in `strips` (= grid size)                 */
  /* ---- rare bond-type channels of the strip forward (additive, ABI 7).  An edge-type channel e >= 2
   * is the identity on every row its bond type does not touch: L_e = I + D_e.  An
   * inference launch on strips (no act_out, 3 <= n_edge <= 7, diagonal gains, no short channels,
   * gemm_mode 0) runs, per strip of at most 5 subtiles and where it is cheaper, ONE GEMM1 on the
   * weights summed over channels 2 .. n_edge-1 (summed in registers from Wp) and X W_e^T on the rows
   * channel e touches only, scattered through D_e.  The touched rows are found from the pack (a row
   * is touched when its row or column of L_e is not the unit vector; the unit diagonal is 1 on a row the
   * mask keeps and 0 elsewhere, so a node the mask leaves out but L_e keeps goes through the scatter), so
   * any operator is correct and
   * the launch needs no operand the channel loop does not have; the result differs from the channel
   * loop's by a re-association of fp32 sums (a few 1e-7), and is the same with and without `ident`. */
  int32_t* rare_strips;       /* optional device counter (caller zeroes it): + 1 per strip of the launch
                                 that took the folded form                                           */
  int32_t no_fold;            /* 1: every strip runs the channel loop (the form before this addition,
                                 bit for bit)                                                        */
  int32_t* rare_debug;        /* optional test output [strip_cap][LNZ_RARE_DEBUG_INTS], zeroed by the
                                 caller; a strip of at most 5 subtiles writes [0] folded form taken,
                                 [1] virtual subtiles, [2 + f] touched rows of channel 2 + f, [8 + v]
                                 channel of virtual subtile v, [16 + 96 f + i] i-th touched strip row
                                 of channel 2 + f (ascending); [7] 1 where the strip's folded GEMM1
                                 read Wf (below)                                                     */
  const float* Wf;            /* optional: lnz_pack_fold_weights of Wp (the folded weights W_F = sum over
                                 channels 2 .. n_edge-1, per layer, in the fragment order of one channel).
                                 With it a strip that takes the folded form reads W_F through its weight
                                 ring instead of summing it in registers (kernel instantiation
                                 lanczosnet_strip_kernel<0,0,2,..>).  NULL: the in-register
                                 sum (<0,0,1,..>).  Both forms give the same bits.  Must be re-packed
                                 when Wp changes.                                                     */
} lnz_forward_args;
/* Contracts of the forward the tests pin (tests/test_gpu_strip_forward_edges.py,
 * tests/test_gpu_tile_forward_edges.py), for the strip kernels and the 32-row tile kernels alike:
 *  - A molecule's extent is its last node the mask keeps + 1; its eigen slots are k < min(extent, K).  V must be
 *    zero at rows >= extent and slots >= extent (the reference's collate, lnz_lanczos_ritz on the extent).
 *  - Slots k >= extent of G.  filter_kind 0: never read, in any instantiation and either gemm_mode — any bit
 *    pattern there, NaN included, leaves the same bits in every output (lnz_spectral_gains_rows may leave them
 *    uninitialised).  filter_kind 1: rows and columns k >= extent of DD that fall inside the molecule's row block
 *    (strips: its extent rounded up to 4 rows; tiles: its rows of the tile) ARE read and meet the zero rows of
 *    V^T X: any FINITE value leaves the same bits, a non-finite one is not filtered (0 x NaN) —
 *    lnz_ada_symmetrize_filters hands over finite values.
 *  - A node the mask leaves out but L keeps (a hole, or a last node inside the molecule's row block) keeps its
 *    own state and feeds its neighbours; only the head's sum AND count skip it: score = mean over the nodes the
 *    mask keeps.  A molecule with an empty mask has no contract (0 / 0).
 *  - state_out and act_out are zeroed by the caller.  On strips a molecule's rows 0 .. rows4 - 1 are written
 *    (rows4 = extent rounded up to 4, at least 4): real nodes, holes, and padding rows, which hold finite
 *    bias-driven values; rows >= rows4 stay exactly zero.  On tiles a single tile writes all 32 rows of its
 *    molecule, a pair tile rows 0 .. split - 1 of its first and 0 .. 31 - split of its second molecule; the
 *    rest stays zero.  Only the rows the mask keeps carry a meaning for the caller.
 *  - A molecule's outputs depend on its batch position, its neighbours in a strip or tile and the padded N only
 *    through the re-association of fp32 sums (within the float32 reference's own error).
 *  - lnz_last_kernel() names what ran: lanczosnet_strip_kernel<0,0,1,false,false> (a launch that may fold the
 *    rare bond-type channels), <0,0,false,false> (channel loop: no_fold, act_out, n_edge < 3 or > 7), <0,0,true,
 *    false> (short channels), <0,2,false|true,false> (dense filters), <0,0,false,true> (gemm_mode 1); without a
 *    strip plan lanczosnet_forward_kernel<4,10,0,0,1> (width 128, input width a multiple of 64), <4,10,0,0,-1>
 *    (width 128, input width 32 or 96), <2,10,0,0,-1> (width 64), <4,10,2,0,0> / <2,10,2,0,0> (dense filters). */
int lnz_lanczosnet_forward(const lnz_forward_args* args, lnz_stream_t stream);
/* Backward of the conv stack w.r.t. its node-state inputs, in the forward's own structure:
 *   dX_l = sum_c M_c (dY_l W_c),   dY_{l-1} = dX_l * [X_l > 0]
 * (M_c symmetric).  Wp / w_off must hold, per KERNEL layer t = num_layer-1-l, pack_rows_k8 of the
 * per-channel TRANSPOSED mix Wb[i][c*dhid + o] = W_l[o][c*d_l + i] ([d_l, C*dhid]); din0 = dhid;
 * Lp, V, G, mask, plan as in the forward; needs the strip plan (strips, n_strips, strip_cap).
 * Writes dy[0..num_layer-2] and dx0. */
int lnz_lanczosnet_input_grad(const lnz_forward_args* args, lnz_stream_t stream);
/* Gradient w.r.t. the spectral gains (the input of the filter MLPs' backward,
 * model/lanczos_net.py:95-123), in eigen space:
 *   dG[l][b][k][s] = sum_o (V^T dY_l)[k][o] * ((V^T X_l) W_{l,s}^T)[k][o]
 * Reads dy (all num_layer slots, as left by lnz_lanczosnet_input_grad), act / x0 (X_l), V, mask,
 * plan and the FORWARD weight packs Wp / w_off (not the transposed ones); writes dgains.
 * Contracts the tests pin (tests/test_gpu_gain_grad_edges.py): dgains is zero-initialised by the
 * caller and only the slots k < K of a molecule's own rows are written, so a slot k >= n stays or
 * becomes exactly 0 (V[:, :, k] = 0 there); rows of act / x0 / dy at or beyond a molecule's node
 * count may hold any FINITE value (they meet V's zero rows; the forward leaves bias-driven values
 * in a molecule's 4-row padding) — a non-finite value there is not filtered; a non-finite entry of
 * V is staged as 0 in every form (strips and tiles), so it stays with its own molecule.
 * lnz_last_kernel() names the form that ran: lanczosnet_strip_gain_grad_kernel on the strip plan,
 * lanczosnet_gain_grad_kernel<4,1> / <4,0> (din0 % 64 == 0 / otherwise) on the tile plan. */
int lnz_lanczosnet_gain_grad(const lnz_forward_args* args, lnz_stream_t stream);
/* Messages of conv layer msg_layer, msg = cat_c(M_c X_l): with dY_l they give the weight gradient
 * of the reference's Linear(15 d -> 128) as ONE library GEMM, dW_l = dY_l^T msg
 * (model/lanczos_net.py:180-182).  Reads act (or x0 for layer 0), Lp, V, G, mask, plan. */
int lnz_lanczosnet_messages(const lnz_forward_args* args, lnz_stream_t stream);
/* Tile plan for lnz_forward_args.plan.  The forward kernels work on 32-row node tiles; with
 * allow_pairs small molecules (extent of mask [B,N] u8) share a tile: one of <= 8 nodes with one
 * of 17..24 (split row 8), two of <= 16 (split row 16).  The tiles are dealt over W workgroups —
 * W = R * n_cu with R = ceil(tiles / (4 n_cu)) rounds (one workgroup per compute unit and round;
 * W = tiles when there are fewer than n_cu) — in descending cost order, boustrophedon, so every workgroup of the launch gets
 * floor/ceil(tiles/W) tiles of balanced cost.  Pair tiles rely on V[:, :, k] = 0 and D[:, k] = 0
 * for k >= n, which the reference's collate guarantees (dataset/qm8.py:264-291) and
 * lnz_lanczos_ritz produces.  No reference counterpart (the reference pads every molecule to N,
 * dataset/qm8.py:232-262).
 * plan: [lnz_plan_wg_cap(B, n_cu) * 12] int32; n_wg: [1] int32 (device). */
int lnz_plan_wg_cap(int B, int n_cu);
int lnz_plan_tiles(const uint8_t* mask, int B, int N, int n_cu, int allow_pairs, int32_t* plan,
                   int32_t* n_wg, lnz_stream_t stream);
/* lnz_plan_tiles plus the list of eigen slots that carry a Ritz pair: gain_rows [<= B*K] int32 =
 * b*K + k for k < min(n_b, K) (any order), n_gain_rows [1] — input of lnz_spectral_gains_rows,
 * which then skips the MLP for the zero-padded eigen columns (~18 % of the rows for QM8 sizes). */
int lnz_plan_batch(const uint8_t* mask, int B, int N, int n_cu, int allow_pairs, int32_t* plan,
                   int32_t* n_wg, int K, int32_t* gain_rows, int32_t* n_gain_rows,
                   int32_t* strips, int32_t* n_strips, lnz_stream_t stream);
/* Strip plan for lnz_forward_args.strips (the strip kernels, conv_strip.hip): a
 * workgroup runs a strip of up to LNZ_STRIP_SUB subtiles of 16 node rows; a molecule takes
 * ceil(n / 4) * 4 consecutive rows at a 4-aligned start and spans at most two subtiles, so the
 * strip's operators are block diagonal on the subtile diagonal and its neighbours.  Packing: first
 * fit decreasing by size class, stable in batch order (a pure function of the mask); the strip
 * height is the smallest for which the batch fits R strips per compute unit, R = the rounds it
 * needs at full height (one round for B = 1024 QM8 molecules on 256 units).  Against the 32-row
 * tiles of lnz_plan_tiles a QM8-sized batch needs 21 % fewer rows.
 * strips: [lnz_strip_cap(B) * LNZ_STRIP_INTS] int32 — words 0, 1 of an entry = molecules and
 * subtiles of the strip, words 2 + 3 i + {0,1,2} = (molecule, first row, node extent) of its i-th
 * molecule; n_strips [1] int32 (device): strips in use.  N <= 32; batches beyond
 * LNZ_STRIP_MAX_B molecules are planned in chunks of that many (consecutive strip ranges).
 * The strips / n_strips arguments of lnz_plan_batch, lnz_prepare_batch[_prev_gains] and
 * lnz_pack_laplacian_plan (may be NULL) make the same plan inside those launches. */
int lnz_strip_cap(int B);
int lnz_plan_strips(const uint8_t* mask, int B, int N, int n_cu, int32_t* strips,
                    int32_t* n_strips, lnz_stream_t stream);
/* ---- R10 backward: the readout head (model/lanczos_net.py:185-194 under loss.backward(),
 * runner/qm8_runner.py:247).  y = (W_o x + b_o) * sigmoid(w_g x + b_g), score = masked mean of y.
 *   X_last     [B,32,dhid]  the stored last conv state (post ReLU; lnz_lanczosnet_forward act_out)
 *   mask       [B,N] uint8;  grad_score [B,P] = dL/dscore
 *   Whead      [P+1,dhid], bhead [P+1]: output rows, then the gate row — or [P,dhid], [P] with the
 *              gate row given on its own as Wgate [1,dhid], bgate [1] (the module keeps them in two
 *              Linears, model/lanczos_net.py:57,61)
 *   row_off    [B] int64 (optional): first row of molecule b in the compact numbering of dY_compact
 * ->
 *   dY         [B,32,dhid]  dL/d(pre-activation of the last conv layer) (zero on padding / masked rows)
 *   dY_compact [R,dhid]     (optional) the rows below a molecule's node extent, compact
 *   dWhead     [P+1,dhid], dbhead [P+1], dbias_last [dhid] (column sums of dY)
 * workspace: lnz_head_backward_workspace_floats(P, n_wg) floats; n_wg workgroups walk the molecules
 * (the partial sums are added in workgroup order: deterministic; n_wg in 1..4096, clamped to B).
 * dhid = 128, N <= 32, P <= 31.
 * Contracts the tests pin (tests/test_gpu_head_grad_edges.py):
 *  - a molecule with an EMPTY mask contributes nothing: its dY rows are exactly 0 and the parameter
 *    gradients are those of the batch without it (torch autograd gives 0 / 0 = NaN for its score);
 *  - rows of X_last outside the mask (holes, the rows from the node extent to 31) may hold any FINITE
 *    value — their dz is exactly 0, so they enter dWhead as 0 * x; a non-finite value there is not
 *    filtered and would poison dWhead;
 *  - dY_compact receives rows [row_off[b], row_off[b] + extent_b) of every molecule (hole rows
 *    included, bit-equal to dY) and nothing else of it is written;
 *  - dY is computed per molecule: its bits do not depend on n_wg. */
int64_t lnz_head_backward_workspace_floats(int P, int n_wg);
/* Node extents (last real node + 1; the training kernels size a molecule by it), their exclusive
 * prefix sums (first row of a molecule in the compact numbering of the message matrix,
 * lnz_lanczosnet_messages row_off) and their total, from mask [B,N] uint8: extent, row_off [B] int64,
 * total [1] int64.  One launch. */
int lnz_node_extents(const uint8_t* mask, int B, int N, int64_t* extent, int64_t* row_off,
                     int64_t* total, lnz_stream_t stream);
int lnz_head_backward(const float* X_last, const uint8_t* mask, const float* grad_score,
                      const float* Whead, const float* bhead, const float* Wgate, const float* bgate,
                      const int64_t* row_off, int B, int N,
                      int P, int dhid, int n_wg, float* workspace, float* dY, float* dY_compact,
                      float* dWhead, float* dbhead, float* dbias_last, lnz_stream_t stream);
/* ---- R9 + R10 + R11 for graphs of 33..128 nodes: the reference's own graph configuration
 * (config/graph_lanczos_net.yaml, dataset/get_graph_data.py:15-49: n in [20, 100]) — every conv
 * layer of model/lanczos_net_general.py:157-182 (model/lanczos_net.py:157-182), the head and the
 * gated masked mean (:185-194) in ONE launch, exact fp32 (v_mfma_f32_16x16x4_f32).  A graph is
 * spread over four workgroups by output columns (32 each); the layer's state goes through Xwork
 * behind a counter in `sync` the four spin on (csrc/conv_mid.hip).  The four must be resident
 * together: a batch larger than the device holds at once (occupancy x compute units; 64 graphs on
 * an idle MI355X) is issued as consecutive launches.  Whether the four share one L2 is read from
 * the hardware at run time (fence-free exchange only then, agent-scope release / acquire
 * otherwise); every spin is bounded and ends in a trap, i.e. a failed launch, not a hang.
 *   X0     [B,N,din0] fp32   layer-0 state (node features / embedding rows), din0 a multiple of
 *                            16 (zero-padded columns), <= 128
 *   L      [B,N,N,C] fp32    by element strides; C = edge types + 1 channels, 1..2
 *   V, G, mask               as for lnz_lanczosnet_forward: [B,N,K], [num_layer,B,S,K], [B,N]
 *   W      fp32              per layer [128][S + C][din_l] (din_0 = din0, else 128): the mix
 *                            weight's column blocks in the reference's order — long scales, then
 *                            edge types (no short-diffusion channels) —, the layers behind each other
 *   bias   [num_layer,128];  Whead [dout + 1,128], bhead [dout + 1]: head rows, then the gate row
 *   Xwork  [lnz_midgraph_workspace_floats(B, N, num_layer)] fp32: the exchange buffer.  After the
 *          launch it holds every layer's output state, [num_layer][B][NR][128] with NR = N rounded
 *          up to 16: slot l = relu(out_l), the input of layer l + 1 (the last slot: what the head
 *          read; all four workgroups publish their slice of it too).  Rows at or beyond N are zero;
 *          rows between a graph's node count and N carry relu(bias_l), as in the reference.  These
 *          are the stored activations lnz_midgraph_head_grad / _input_grad / _project read.
 *   sync   [B * (num_layer + 1)] int32, ZERO on entry (arrival counters, then placement words)
 *   score  [B,dout]
 * N <= 128, K <= 32, S <= 16, dout <= 31, hidden width 128. */
int64_t lnz_midgraph_workspace_floats(int B, int N, int num_layer);
int lnz_midgraph_forward(const float* X0, const float* L, int64_t stride_b, int64_t stride_r,
                         int64_t stride_c, int64_t stride_ch, const float* V, const float* G,
                         const uint8_t* mask, const float* W, const float* bias, const float* Whead,
                         const float* bhead, int B, int N, int K, int C, int S, int num_layer,
                         int din0, int dout, float* Xwork, int32_t* sync, float* score,
                         lnz_stream_t stream);
/* ---- Training for graphs of 33..128 nodes: loss.backward() (runner/graph_runner.py:216-219) through
 * the head and the conv layers of lnz_midgraph_forward, three launches (csrc/conv_mid_grad.hip).
 * Exact fp32, every sum in a fixed order, no float atomics: bitwise repeatable.  Shapes, strides and
 * limits as for lnz_midgraph_forward; NR = N rounded up to 16; Xwork = that launch's buffer.
 *
 * 1. The readout head (model/lanczos_net_general.py:185-194, model/lanczos_net.py:185-194) on the
 *    stored last state X_last = Xwork slot num_layer - 1 [B,NR,128]: grad_score [B,dout] ->
 *    dOut_last [B,NR,128], the gradient at the last conv layer's pre-activation (zero on masked and
 *    padded rows), and per-graph partials in workspace [lnz_midgraph_head_grad_workspace_floats(B,
 *    dout)]: dWhead [B][dout + 1][128], then dbhead [B][dout + 1] (head rows, then the gate row); the
 *    gradients are their sums over the graphs (any fixed order). */
int64_t lnz_midgraph_head_grad_workspace_floats(int B, int dout);
int lnz_midgraph_head_grad(const float* X_last, const uint8_t* mask, const float* grad_score,
                           const float* Whead, const float* bhead, int B, int N, int dout,
                           float* dOut_last, float* workspace, lnz_stream_t stream);
/* 2. Node-state gradients of the whole conv stack (model/lanczos_net_general.py:157-182,
 *    model/lanczos_net.py:157-182) in ONE launch: the forward kernel's structure and exchange run
 *    on the gradient.  dOut [num_layer][B][NR][128] holds the last layer's slot on entry (launch 1)
 *    and dOut_l = dX_{l+1} . [X_{l+1} > 0] for every layer on return; rows at or beyond a graph's
 *    node count are exactly zero.  Wt: per layer [128 in][S + C][128 out], Wt[i][c][o] = W[o][c][i]
 *    (layer 0: rows at or beyond its input width zero).  The operator channels are not assumed
 *    symmetric.  sync [B * (num_layer + 1)] int32, ZERO on entry, this launch's own (never the
 *    forward's).  dX0 [B,NR,din0] (optional): the gradient at the layer-0 state (the embedding
 *    rows').  folded [B] int32 (optional): 1 where the graph's operator channels are equal. */
int lnz_midgraph_input_grad(float* dOut, const float* Xwork, const float* L, int64_t stride_b,
                            int64_t stride_r, int64_t stride_c, int64_t stride_ch, const float* V,
                            const float* G, const float* Wt, int B, int N, int K, int C, int S,
                            int num_layer, int din0, int32_t* sync, float* dX0, int32_t* folded,
                            lnz_stream_t stream);
/* 3. The operands of the weight gradients and the gain gradients, one workgroup per (graph, layer).
 *    With X_l the layer's input state (X0 [B,N,din0] for layer 0, else Xwork slot l - 1), workspace
 *    [lnz_midgraph_project_workspace_floats(...)] receives, behind each other:
 *      A  [num_layer][B][K][128]      V^T dOut_l
 *      Q  [num_layer][B][K][S][128]   g_s . (V^T X_l)        (columns at or beyond din0 zero in layer 0)
 *      M  [num_layer][B][NR][C][128]  L_c X_l
 *      dG [num_layer][B][K][S]        sum_o A[k][o] ((V^T X_l) W_s^T)[k][o]   (want_dgains != 0)
 *      db [num_layer][B][128]         column sums of dOut_l
 *    so that dW_l = [A_l^T Q_l | dOut_l^T M_l] (the contraction of the long scales runs over the B K
 *    eigen rows, not the B N node rows), db_l = the sum of its partials over the graphs, and dG is
 *    what lnz_spectral_mlp_grad takes.  W: the forward's weights. */
int64_t lnz_midgraph_project_workspace_floats(int B, int N, int K, int C, int S, int num_layer);
int lnz_midgraph_project(const float* dOut, const float* Xwork, const float* X0, const float* L,
                         int64_t stride_b, int64_t stride_r, int64_t stride_c, int64_t stride_ch,
                         const float* V, const float* G, const float* W, int B, int N, int K, int C,
                         int S, int num_layer, int din0, int want_dgains, float* workspace,
                         lnz_stream_t stream);
/* The whole batch preparation in ONE launch: lnz_plan_batch (workgroup 0), lnz_lanczos_ritz on
 * channel 0 of L (workgroups 1..B, dispatched first: they are the long, latency-bound pole) and
 * lnz_pack_laplacian (workgroups B+1..2B) — the two byte movers run in the shadow of the Lanczos
 * wavefronts instead of in front of them.  L [B,N,N,C] with strides (elements); n_nodes [B] as
 * for lnz_lanczos_ritz; outputs as in the three functions.  N <= 32.
 * Lp == NULL (then ident must be NULL too): plan + Ritz pairs only, B + 1 workgroups — the pack is
 * then the caller's lnz_pack_laplacian_ident on a second stream, under the spectral-gains launch
 * (matrix-pipe work that leaves the memory path idle) instead of next to the Lanczos wavefronts. */
int lnz_prepare_batch(const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                      int64_t stride_ch, int B, int N, int C, float* Lp, const uint8_t* mask,
                      const int32_t* n_nodes, int n_cu, int allow_pairs, int32_t* plan,
                      int32_t* n_wg, int K, int32_t* gain_rows, int32_t* n_gain_rows, float* D,
                      float* V, int32_t* info, uint32_t* ident, int32_t* strips, int32_t* n_strips,
                      lnz_stream_t stream);
/* Software pipeline over a STREAM of batches: lnz_prepare_batch of batch k+1 and the spectral
 * gains (kind 0, live rows) of batch k in one launch.  The two are independent — no flags — and
 * complementary: the Lanczos / eigensolve wavefronts are latency bound (one per SIMD, matrix pipes
 * idle), the MLP is matrix-pipe work.  D_prev [B_prev,K], rows_prev / n_rows_prev: outputs of the
 * previous preparation; G_prev [num_layer,B_prev,S,K]: live slots written.  Everything else as in
 * lnz_prepare_batch. */
int lnz_prepare_batch_prev_gains(
    const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c, int64_t stride_ch, int B,
    int N, int C, float* Lp, const uint8_t* mask, const int32_t* n_nodes, int n_cu, int allow_pairs,
    int32_t* plan, int32_t* n_wg, int K, int32_t* gain_rows, int32_t* n_gain_rows, float* D,
    float* V, uint32_t* ident, const float* D_prev, int B_prev, const int32_t* rows_prev,
    const int32_t* n_rows_prev, const int32_t* dist_host, int S, int num_layer,
    const float* mlp_pack, float* G_prev, int32_t* strips, int32_t* n_strips, lnz_stream_t stream);
/* lnz_pack_laplacian + lnz_plan_batch in ONE launch (workgroup B plans while 0..B-1 pack): the two
 * byte movers in front of the Lanczos kernel are independent, and the planner is a single
 * latency-bound workgroup.  Arguments as in the two functions; gain_rows may be NULL. */
int lnz_pack_laplacian_plan(const float* L, int64_t stride_b, int64_t stride_r, int64_t stride_c,
                            int64_t stride_ch, int B, int N, int C, float* Lp,
                            const uint8_t* mask, int n_cu, int allow_pairs, int32_t* plan,
                            int32_t* n_wg, int K, int32_t* gain_rows, int32_t* n_gain_rows,
                            uint32_t* ident, int32_t* strips, int32_t* n_strips,
                            lnz_stream_t stream);
/* sizeof(lnz_forward_args) as compiled into the library — lets a foreign-language binding verify
 * its struct layout before the first call. */
int64_t lnz_forward_args_size(void);

/* ---- R4, R5, R8: AdaLanczosNet stages --------------------------------------------------------
 * lnz_ada_graph_laplacian: Gaussian-kernel learned Laplacian of model/ada_lanczos_net.py:101-137
 *   (dist2 over node embeddings, sigma2 = mean over all N^2 pairs, exp(-d2/sigma2) * adj,
 *   D^-1/2 A D^-1/2 with the zero-row guard); adj = (L0 != 0) as :310-311.  Node features are either
 *   embedding rows gathered by id (node_feat + embedding[num_atom, D]) or float rows node_feat_f
 *   [B,N,D].  L0 addressed by element strides (pass L[...,0] of the channels-last Laplacian).
 *   Le [B,N,N].
 * lnz_ada_lanczos_layer: the in-model Lanczos layer of :139-247, reference exact: fp32,
 *   T_it = min(N,K) steps, sequential Gram-Schmidt applied twice, breakdown mask beta < 1e-4, and
 *   the three quirks of SURVEY.md F6 (alpha of the breakdown step zeroed; its Q column dropped;
 *   NODE rows >= idx_mask zeroed).  q1 [B,N] is the raw start vector (the reference draws
 *   torch.randn(B,N,1) on the CPU generator, :161).  mask [B,N] uint8 or NULL.  T [B,K,K], Q [B,N,K].
 * lnz_ada_t_powers: T^p for the S exponents in dist_host by sequential TT = TT*T (:262-270),
 *   written as torch.cat(T_list, dim=2): Tcat [B, K, S*K] (= the [B, K*K*S] MLP input).
 * lnz_ada_symmetrize_filters: DD [B,K,K,S] (MLP output view, :274-275) ->
 *   DDp [B,S,K,K] = (DD + DD^T)/2 (:278), the dense-filter operand of lnz_lanczosnet_forward. */
int lnz_ada_graph_laplacian(const int64_t* node_feat, const float* embedding, int num_atom,
                            const float* node_feat_f, int D, const float* L0, int64_t stride_b,
                            int64_t stride_r, int64_t stride_c, int B, int N, float* Le,
                            lnz_stream_t stream);
int lnz_ada_lanczos_layer(const float* A, const uint8_t* mask, const float* q1, int B, int N,
                          int K, float* T, float* Q, lnz_stream_t stream);
int lnz_ada_t_powers(const float* T, int B, int K, const int32_t* dist_host, int S, float* Tcat,
                     lnz_stream_t stream);
int lnz_ada_symmetrize_filters(const float* DD, int B, int K, int S, float* DDp,
                               lnz_stream_t stream);

/* Opt-in split-precision operand of the filter MLPs' GEMMs (model/ada_lanczos_net.py:271-272):
 * v = [relu](alpha * X[m][k] + bias[k]), X [M, K] fp32 (leading dimension ldx) ->
 * out [M, 3 Kp] fp16 = [ hi | hi | lo ], hi = fp16(v), lo = fp16(v - hi), columns >= K zero.
 * Against weights laid out [ w_hi | w_lo | w_hi ] ONE fp16 GEMM of depth 3 Kp (fp32 accumulate)
 * gives hi w_hi + hi w_lo + lo w_hi = v w to ~2^-22 relative. */
int lnz_split_f16x3(const float* X, int M, int K, int ldx, const float* bias, float alpha, int relu,
                    int Kp, void* out, lnz_stream_t stream);

/* R5 for training (csrc/ada_lanczos_grad.hip): the same Lanczos layer on an fp64 Laplacian
 * A [B,N,N] (N, K <= 32), outputs T [B,K,K] and Q [B,N,K] in fp64, plus the state its backward needs
 * in `ws` (lnz_ada_lanczos_f64_workspace_doubles(B) doubles: basis vectors, alpha, beta, the valid
 * flags and every Gram-Schmidt coefficient), and the backward: given dLoss/dT, dLoss/dQ (fp64,
 * same shapes) the reverse sweep of the recurrence -> dA [B,N,N] = dLoss/dA.  Replaces torch
 * autograd through model/ada_lanczos_net.py:139-247 (the reference differentiates its own loop of
 * small ATen ops).  mask may be NULL (all nodes real); masks / flags are constants of the gradient. */
/* The stages either side of it for training, fp64 as well.  Learned Laplacian (:101-137) from the
 * embedded node states X [B,N,D] fp32 and the adjacency mask L0 != 0 (strided [B,N,N] view):
 * Le [B,N,N] fp64 + `state` (lnz_ada_laplacian_f64_state_doubles(B, N) doubles: A, dist2, D^-1/2,
 * sigma2); backward: dLe -> dX [B,N,D] fp64.  T powers (:262-270) of the fp64 T: Tcat [B,K,S K] fp32
 * as lnz_ada_t_powers + every power P [B,pmax,K,K] fp64; backward: dTcat (fp32) -> dT [B,K,K] fp64. */
int64_t lnz_ada_laplacian_f64_state_doubles(int B, int N);
int lnz_ada_graph_laplacian_f64(const float* X, int D, const float* L0, int64_t stride_b,
                                int64_t stride_r, int64_t stride_c, int B, int N, double* Le,
                                double* state, lnz_stream_t stream);
int lnz_ada_graph_laplacian_f64_backward(const float* X, int D, int B, int N, const double* state,
                                         const double* dLe, double* dX, lnz_stream_t stream);
int lnz_ada_t_powers_f64(const double* T, int B, int K, const int32_t* dist_host, int S, float* Tcat,
                         double* P, lnz_stream_t stream);
int lnz_ada_t_powers_f64_backward(const double* T, int B, int K, const int32_t* dist_host, int S,
                                  const float* dTcat, const double* P, double* dT, lnz_stream_t stream);
int64_t lnz_ada_lanczos_f64_workspace_doubles(int B);
int lnz_ada_lanczos_layer_f64(const double* A, const uint8_t* mask, const float* q1, int B, int N,
                              int K, double* T, double* Q, double* ws, lnz_stream_t stream);
int lnz_ada_lanczos_layer_f64_backward(const double* A, int B, int N, int K, const double* ws,
                                       const double* dT, const double* dQ, double* dA,
                                       lnz_stream_t stream);

/* The same filter MLPs, hand-written (csrc/f16x3_linear.hip): one launch per Linear,
 *   out = [relu]( alpha * (X W^T) + bias ),   X [M, K], W [N, K],
 * both operands as (hi, lo) fp16 PLANES (x = x_hi + x_lo, w = w_hi + w_lo) and the product as
 * x_hi w_hi + x_hi w_lo + x_lo w_hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation — the four
 * pieces of a k-slice are staged once (global_load_lds, two 64 KB LDS buffers) and feed all three
 * products.  K %% 64 == 0; x planes hold ceil(M / 128) * 128 rows, w planes ceil(N / 128) * 128 rows
 * (zero padded), leading dimensions ldx / ldw in elements (multiples of 8).  Output either as the
 * next Linear's operand, (out_hi, out_lo) fp16 planes with leading dimension ldo (rows >= M are
 * not written), or — the last Linear — as fp32 out_f32 [M, ldo].  lnz_f16x3_split writes the
 * planes of an fp32 matrix (scale * X; rows >= M and columns >= K zero). */
int lnz_f16x3_split(const float* X, int M, int K, int64_t ldx, float scale, int Mp, int Kp,
                    uint16_t* hi, uint16_t* lo, lnz_stream_t stream);
int lnz_f16x3_linear(const uint16_t* x_hi, const uint16_t* x_lo, int ldx, const uint16_t* w_hi,
                     const uint16_t* w_lo, int ldw, const float* bias, float alpha, int relu, int M,
                     int N, int K, uint16_t* out_hi, uint16_t* out_lo, float* out_f32, int ldo,
                     float* partials, lnz_stream_t stream);
/* Split-K for shapes with too few 128 x 128 output tiles to fill the chip (the last Linear, N =
 * 1056: 72 tiles): with `partials` = lnz_f16x3_linear_splits(M, N, K) * M * N floats of scratch the K
 * range is divided over that many workgroups per tile and a second kernel adds the partial tiles in
 * a fixed order (bit-reproducible) before alpha / bias / ReLU; partials = NULL: no split. */
int lnz_f16x3_linear_splits(int M, int N, int K);

/* The filter MLPs in the default exact-fp32 mode, hand-written (csrc/f32_linear.hip; replaces
 * torch.nn.functional.linear + relu of model/ada_lanczos_net.py:271-272 = nn.Sequential of
 * nn.Linear / nn.ReLU): one launch per Linear,
 *   out = [relu]( X W^T + bias ),   X [M, K] (leading dimension ldx), W [N, K] (ldw), out [M, ldo],
 * fp32 accumulation, bias + ReLU in the epilogue;
 * K %% 32 == 0, ldx / ldw multiples of 4 and the base pointers 16-byte aligned (LNZ_ENOTSUP
 * otherwise); any M, N (partial tiles re-read the last row, never store).  bias may be NULL.
 * fp32 operands on v_mfma_f32_16x16x4_f32 (a k-ordered fma chain per output element: the result
 * is bit-identical to hipBLASLt's fp32 GEMM on these shapes), operand slices copied global -> LDS
 * by buffer_load ... lds.  Outputs with too few 128 x 128 tiles to fill the chip (the last Linear,
 * N = 1056: 72 tiles) run STREAM-K inside the one launch: (tile, k-slice) units dealt evenly over
 * lnz_f32_linear_splits(M, N, K) workgroups, partial tiles added by the tile's owner in a fixed
 * order (bit-reproducible).  For those shapes `partials` = lnz_f32_linear_workspace_floats(M, N, K)
 * floats, 16-byte aligned, whose LAST tiles-many words (the tile counters) must be ZERO on entry;
 * they are zero again on return, so one zero-initialised workspace serves every later call on
 * the same stream.  partials = NULL (or _splits == 1): one workgroup per tile. */
int lnz_f32_linear(const float* x, int ldx, const float* w, int ldw, const float* bias, int relu,
                   int M, int N, int K, float* out, int ldo, float* partials, lnz_stream_t stream);
int lnz_f32_linear_splits(int M, int N, int K);
int64_t lnz_f32_linear_workspace_floats(int M, int N, int K);

/* ---- the GAT baseline (model/gat.py, config/qm8_gat.yaml): attention and readout --------------
 * One layer's dense additive attention for all C channels x H heads (replaces model/gat.py:153-175;
 * the projection :150-152 is ONE lnz_f32_linear on the stacked weight [C H Dh, Din]).  Block
 * c H + h of Dh columns of Wh [B N, ldw] is head h of channel c; per block
 *   s1 = Wh a1 + b1, s2 = Wh a2 + b2                                   (att_net_1 / att_net_2)
 *   e[i][j] = leaky_relu(s1[i] + s2[j], 0.2) + L[b, i, j, c]
 *   att[:, j] = softmax over the row index i, per column j             (F.softmax(.., dim=1), :158-160)
 *   out[i] = sum_j att[i][j] Wh[j] + bias ;  ELU if `elu`             (:166-175)
 * written to the same block of out [B N, ldo].  L (element (b, i, j, c) at b stride_b + i stride_r +
 * j stride_c + c stride_ch floats, strides >= 0: a sliced or expanded view is read in place) is ADDED
 * to the logits, it masks nothing — all N rows and columns of the padded batch take part, there is no
 * node count.  a1, a2, bias [C H][Dh], b1, b2 [C H]; `bias` is what the caller resolved (the
 * reference's aliased list reads bias_{h}_{C-1}_{t} for every channel).  out must not alias Wh.
 * 1 <= N <= 32, C <= 8, H <= 16, Dh a multiple of 4 and <= 32, ldw / ldo multiples of 4 (LNZ_ENOTSUP
 * otherwise); Wh, bias, out 16-byte aligned.  Column maximum subtracted, full-precision expf / expm1f,
 * every sum in a fixed order: bit-reproducible.  One workgroup per (molecule, channel), 40 KB of LDS. */
int lnz_gat_attention(const float* Wh, int ldw, const float* L, int64_t stride_b, int64_t stride_r,
                      int64_t stride_c, int64_t stride_ch, const float* a1, const float* b1,
                      const float* a2, const float* b2, const float* bias, int B, int N, int C, int H,
                      int Dh, int elu, float* out, int ldo, lnz_stream_t stream);
/* The last layer's head mean and the gated masked-mean readout in one launch (replaces
 * model/gat.py:177-196): x[i] = (1 / CH) sum of the CH blocks of Dh columns of Hlast [B N, ld], blocks
 * ascending; y[i] = (Wo x[i] + bo) * sigmoid(wg x[i] + bg); score [B, P] = mean of y over the rows with
 * mask != 0 (mask [B, N] u8; NULL: all N rows).  No masked row: NaN, like the reference's empty mean.
 * Wo [P][Dh], bo [P], wg [Dh], bg [1].  N <= 32, Dh <= 32, P <= 16 (LNZ_ENOTSUP otherwise). */
int lnz_gat_readout(const float* Hlast, int ld, const uint8_t* mask, const float* Wo, const float* bo,
                    const float* wg, const float* bg, int B, int N, int CH, int Dh, int P, float* score,
                    lnz_stream_t stream);
/* The backward of lnz_gat_attention (model/gat.py:153-175 under loss.backward()) for every channel and
 * head of one layer.  The attention block P is recomputed from Wh by the forward's own instructions; with
 *   dO = dOut * elu'(.) (elu: 1 where out > 0, else out + 1; out is read for nothing else and may be NULL
 *   when elu = 0), dP[i][j] = dO[i] . Wh[j], t[j] = sum_i P dP, dE = P (dP - t), dZ = dE * (s1[i] + s2[j] > 0
 *   ? 1 : 0.2), ds1[i] = sum_j dZ, ds2[j] = sum_i dZ:
 *   dWh[j] = sum_i P[i][j] dO[i] + ds1[j] a1 + ds2[j] a2                  [B N, ldg], block c H + h
 *   da1 = sum ds1[i] Wh[i], da2 = sum ds2[i] Wh[i], dbias = sum dO[i]    [C H][Dh], summed over the molecules
 *   db1 = sum ds1[i], db2 = sum ds2[i]                                   [C H]
 * L gets no gradient; all N padded rows and columns take part.  dbias is the gradient of the bias AS
 * PASSED (one row per block; the caller adds the rows of an aliased parameter).  The sums over the
 * molecules use no atomics: every workgroup writes its partials to workspace
 * [lnz_gat_attention_backward_workspace_floats(B, C, H, Dh)] (no initialisation needed) and a second
 * launch adds them in a fixed order; every sum inside a block runs in a fixed order: bit-reproducible.
 * The envelope of lnz_gat_attention; ldw / ldo / ldd / ldg multiples of 4 (LNZ_ENOTSUP otherwise); Wh, out,
 * dOut, dWh 16-byte aligned; dWh must alias none of Wh, out, dOut.  One workgroup per (molecule, channel),
 * 60 KB of LDS. */
int64_t lnz_gat_attention_backward_workspace_floats(int B, int C, int H, int Dh);
int lnz_gat_attention_backward(const float* Wh, int ldw, const float* L, int64_t stride_b, int64_t stride_r,
                               int64_t stride_c, int64_t stride_ch, const float* a1, const float* b1,
                               const float* a2, const float* b2, const float* out, int ldo, const float* dOut,
                               int ldd, int B, int N, int C, int H, int Dh, int elu, float* workspace,
                               float* dWh, int ldg, float* da1, float* db1, float* da2, float* db2,
                               float* dbias, lnz_stream_t stream);
/* The backward of lnz_gat_readout (model/gat.py:177-196 under loss.backward()): x, o = Wo x + bo and
 * g = sigmoid(wg x + bg) recomputed as the forward computes them; per row i of the mask (cnt of them; all N
 * without a mask), with dscore [B, P]:
 *   dy = dscore / cnt, do = dy g, dzg = (sum_p dy[p] o[p]) g (1 - g), dx = Wo^T do + wg dzg
 *   dHlast[i, every one of the CH blocks] = dx / CH        [B N, ldg]; exactly 0 on rows outside the mask
 *   dWo [P][Dh] = sum do x^T, dbo [P] = sum do, dwg [Dh] = sum dzg x, dbg [1] = sum dzg   (rows, molecules)
 * The same reduction scheme: per-molecule partials in workspace
 * [lnz_gat_readout_backward_workspace_floats(B, Dh, P)], added in a fixed order by a second launch.
 * A molecule without a masked row (NaN in the forward) is unspecified.  The envelope of lnz_gat_readout;
 * dHlast must not alias Hlast. */
int64_t lnz_gat_readout_backward_workspace_floats(int B, int Dh, int P);
int lnz_gat_readout_backward(const float* Hlast, int ld, const uint8_t* mask, const float* Wo, const float* bo,
                             const float* wg, const float* bg, const float* dscore, int B, int N, int CH,
                             int Dh, int P, float* workspace, float* dHlast, int ldg, float* dWo, float* dbo,
                             float* dwg, float* dbg, lnz_stream_t stream);

/* ---- the GGNN baseline (model/ggnn.py:137-197, config/qm8_ggnn.yaml), csrc/ggnn.hip ----
 * All num_prop gated propagation steps and the readout in ONE launch.  state0 [B N, ld0] is
 * input_func(embedding(node_feat)); with C = num_bond_type + 1 channels, state width D, message hidden
 * width 128, per step on the state S
 *   H_c = relu(S W1_c^T + b1_c), M_c = H_c W2_c^T + b2_c                (msg_func[c]; W1 [C][128][D], W2 [C][D][128])
 *   A_c = Â_c M_c per molecule; Â_c = (L[.., c] != 0), for avg != 0 divided by (row degree + FLT_EPSILON)
 *   S'  = GRUCell(cat_c A_c, S)                                        (Wih [3 D][C D], Whh [3 D][D], gates r, z, n)
 * then y = (Wo s + bo) * sigmoid(wg s + bg) and score [B, P] = mean of y over the rows with mask != 0
 * (mask [B, N] u8; NULL: all N rows; no masked row: NaN).  All N rows of a molecule take part in the
 * propagation.  L (element (b, i, j, c) at b stride_b + i stride_r + j stride_c + c stride_ch floats,
 * strides >= 0) is only compared with zero — a NaN or a negative entry is an edge — and never written.
 * state_out [B N, ldso] (may be NULL) receives the final state.  num_prop = 0: the readout of state0.
 * 1 <= N <= 32, 1 <= C <= 8, D a multiple of 32 and <= 128, 1 <= P <= 16, num_prop >= 0, ld0 / ldso
 * multiples of 4, state0 / state_out / the weights 16-byte aligned (LNZ_ENOTSUP otherwise); null
 * pointers, B or N <= 0, ld0 / ldso below D, negative strides, score or state_out overlapping state0
 * or each other, tile_rows other than 0, 32, 64: LNZ_EINVAL.  A workgroup holds the state of
 * floor(tile_rows / N) molecules in LDS for all steps (139,520 B of dynamic LDS at D = 128 and 64 rows);
 * tile_rows = 0: 32 while the 32-row tiles all fit in one round of the compute units, 64 beyond — a
 * row's arithmetic and bits do not depend on it.  Exact-fp32 MFMA, no atomics, every sum in a fixed
 * order: bit-reproducible. */
int lnz_ggnn_forward(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                     int64_t stride_c, int64_t stride_ch, const uint8_t* mask, const float* W1,
                     const float* b1, const float* W2, const float* b2, const float* Wih, const float* bih,
                     const float* Whh, const float* bhh, const float* Wo, const float* bo, const float* wg,
                     const float* bg, int B, int N, int C, int D, int P, int num_prop, int avg, float* score,
                     float* state_out, int ldso, int tile_rows, lnz_stream_t stream);

/* ---- the GGNN baseline's backward, csrc/ggnn.hip and csrc/ggnn_grad.hip ----
 * lnz_ggnn_forward_states: lnz_ggnn_forward (the same kernel template, arguments, envelope and errors; score
 * and state_out have its bits) that also leaves the state trajectory states [num_prop + 1][B N][D] (row
 * stride D, 16-byte aligned, no overlap with state0, score or state_out): S_t at the start of step t, S_T
 * after the last.  Nothing else is saved: the backward recomputes a step from S_t. */
int lnz_ggnn_forward_states(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                            int64_t stride_c, int64_t stride_ch, const uint8_t* mask, const float* W1,
                            const float* b1, const float* W2, const float* b2, const float* Wih, const float* bih,
                            const float* Whh, const float* bhh, const float* Wo, const float* bo, const float* wg,
                            const float* bg, int B, int N, int C, int D, int P, int num_prop, int avg,
                            float* score, float* state_out, int ldso, float* states, int tile_rows,
                            lnz_stream_t stream);

/* lnz_ggnn_backward_step: one propagation step of backpropagation through time for the whole batch, launched
 * for t = T-1 .. 0.  S [B N, lds] = S_t, dSnext [B N, ldd] = dL/dS_{t+1}; the step is recomputed on chip with
 * the forward's arithmetic (H_c, M_c, A_c, gi, gh, r, z, n), then
 *   dn = dS' (1 - z), dz = dS' (S - n), dS = dS' z, dn_pre = dn (1 - n^2), dz_pre = dz z (1 - z),
 *   dr_pre = dn_pre gh_n r (1 - r), dgi = [dr_pre, dz_pre, dn_pre], dgh = [dr_pre, dz_pre, dn_pre r]
 *   dS += dgh Whh ; per channel c: dA_c = dgi Wih[:, cD:(c+1)D], dM_c = Â_c^T dA_c per molecule,
 *   dHpre_c = (dM_c W2_c) [H_c > 0], dS += dHpre_c W1_c
 * W1, b1, .. bhh: the forward's operands; W1T [C][D][128], W2T [C][128][D], WihT [C][D][3 D] (block c =
 * Wih[:, cD:(c+1)D]^T), WhhT [D][3 D]: their transposes, packed by the caller.  Out: dS [B N, ldo] = dL/dS_t and
 * the row-space operands of this step's weight gradients, contiguous: dgi [B N][3 D], dghn [B N][D] (the n
 * part of dgh; its r and z parts are dgi's), A [B N][C D] = cat_c A_c, dM [B N][C D], H [B N][C 128],
 * dHpre [B N][C 128].  The caller contracts them over the rows (dWih = dgi^T A, dWhh = dgh^T S, dW2_c =
 * dM_c^T H_c, dW1_c = dHpre_c^T S, the biases their column sums) and may reuse the buffers for the next step.
 * The envelope of lnz_ggnn_forward (N <= 32, C <= 8, D a multiple of 32 and <= 128: LNZ_ENOTSUP, as are rows
 * that are not 16-byte aligned); null pointers, B or N <= 0, a row stride below D, negative strides of L,
 * an output overlapping an input or another output: LNZ_EINVAL.  L is read through its four strides and
 * never written.  32-row tiles, 138,368 B of dynamic LDS at D = 128; no atomics, every sum in a fixed order:
 * bit-reproducible. */
int lnz_ggnn_backward_step(const float* S, int lds, const float* dSnext, int ldd, const float* L, int64_t stride_b,
                           int64_t stride_r, int64_t stride_c, int64_t stride_ch, const float* W1, const float* b1,
                           const float* W2, const float* b2, const float* Wih, const float* bih, const float* Whh,
                           const float* bhh, const float* W1T, const float* W2T, const float* WihT,
                           const float* WhhT, int B, int N, int C, int D, int avg, float* dS, int ldo, float* dgi,
                           float* dghn, float* A, float* dM, float* H, float* dHpre, lnz_stream_t stream);

/* lnz_ggnn_readout_backward: the readout of lnz_ggnn_forward under loss.backward().  Slast [B N, ld] = S_T;
 * o = Wo s + bo and g = sigmoid(wg s + bg) recomputed as the forward computes them; per row i of the mask
 * (cnt of them; all N without a mask), with dscore [B, P]:
 *   dy = dscore / cnt, do = dy g, dzg = (sum_p dy[p] o[p]) g (1 - g), dSlast[i] = Wo^T do + wg dzg
 * dSlast [B N, ldg] is exactly 0 on rows outside the mask; dWo [P][D] = sum do s^T, dbo [P] = sum do,
 * dwg [D] = sum dzg s, dbg [1] = sum dzg over rows and molecules: per-molecule partials in workspace
 * [lnz_ggnn_readout_backward_workspace_floats(B, D, P)], added in a fixed order by a second launch.  A
 * molecule without a masked row (NaN in the forward) is unspecified.  N <= 32, D a multiple of 32 and <= 128,
 * P <= 16 (LNZ_ENOTSUP); dSlast must not alias Slast. */
int64_t lnz_ggnn_readout_backward_workspace_floats(int B, int D, int P);
int lnz_ggnn_readout_backward(const float* Slast, int ld, const uint8_t* mask, const float* Wo, const float* bo,
                              const float* wg, const float* bg, const float* dscore, int B, int N, int D, int P,
                              float* workspace, float* dSlast, int ldg, float* dWo, float* dbo, float* dwg,
                              float* dbg, lnz_stream_t stream);

/* ---- the MPNN baseline (model/mpnn.py:125-212, model/set2set.py:60-100, config/qm8_mpnn.yaml), csrc/mpnn.hip ----
 * lnz_mpnn_forward: all num_prop edge-network propagation steps (msg_func 'MLP') in ONE launch.  state0
 * [B N, ld0] is input_func(node_embedding(node_feat)); with C = num_bond_type + 1 channels, state width D,
 * message hidden width 64 and W1_c = [W1n_c | W1s_c] (columns 0 .. D-1 act on the neighbour h_b, columns
 * D .. 2D-1 on the row's own h_a), per step on the state S
 *   P_c = S W1n_c^T ; Q_c = S W1s_c^T + b1_c ; R_c[a] = sum over b with L[a, b, c] != 0 of relu(Q_c[a] + P_c[b])
 *   M_c[a] = R_c[a] W2_c^T + deg_c[a] b2_c, for avg != 0 divided by (deg_c[a] + FLT_EPSILON) AFTER the sum
 *   S' = GRUCell(cat_c M_c, S)     (the cell of lnz_ggnn_forward: Wih [3 D, C D], bih, Whh [3 D, D], bhh)
 * which is the reference's 2D -> 64 -> D MLP on all N^2 ordered pairs, factored.  W1 [C][64][2 D], b1 [C][64],
 * W2 [C][D][64], b2 [C][D].  Every one of the N rows of a molecule propagates (a padded row has degree 0, a
 * message of exactly 0 and evolves under GRU(0, h)).  L [B, N, N, C] is read through its four strides
 * (elements, >= 0), only compared with zero (a NaN or a negative entry is an edge) and never written.
 * state_out [B N, ldso] receives the final state (num_prop = 0: a copy of state0).
 * Envelope: N <= 32, C <= 8, D a multiple of 32 and <= 128, num_prop >= 0, 16-byte aligned rows (LNZ_ENOTSUP);
 * null pointers, B or N <= 0, a row stride below D, negative strides, state_out overlapping state0,
 * tile_rows other than 0, 32, 64: LNZ_EINVAL.  tile_rows as in lnz_ggnn_forward: a row's arithmetic and
 * bits do not depend on it.  Exact-fp32 MFMA, no atomics, every sum in a fixed order: bit-reproducible. */
int lnz_mpnn_forward(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                     int64_t stride_c, int64_t stride_ch, const float* W1, const float* b1, const float* W2,
                     const float* b2, const float* Wih, const float* bih, const float* Whh, const float* bhh, int B,
                     int N, int C, int D, int num_prop, int avg, float* state_out, int ldso, int tile_rows,
                     lnz_stream_t stream);

/* ---- the backward of the MPNN propagation, csrc/mpnn.hip and csrc/mpnn_grad.hip ----
 * lnz_mpnn_forward_states: lnz_mpnn_forward (the same kernel body, arguments, envelope and errors; the final
 * state has its bits at either tile height) that also leaves the state trajectory states
 * [num_prop + 1][B N][D] (row stride D, 16-byte aligned, no overlap with state0 or state_out): S_t at the start
 * of step t, S_T after the last.  state_out may be NULL here (the final state is states[num_prop]).  Nothing else
 * is saved: the backward recomputes a step from S_t.  lnz_last_kernel() names mpnn_forward_states_kernel. */
int lnz_mpnn_forward_states(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                            int64_t stride_c, int64_t stride_ch, const float* W1, const float* b1, const float* W2,
                            const float* b2, const float* Wih, const float* bih, const float* Whh, const float* bhh,
                            int B, int N, int C, int D, int num_prop, int avg, float* state_out, int ldso,
                            float* states, int tile_rows, lnz_stream_t stream);

/* lnz_mpnn_backward_step: one propagation step of backpropagation through time for the whole batch, launched
 * for t = T-1 .. 0.  S [B N, lds] = S_t, dSnext [B N, ldd] = dL/dS_{t+1}; the step is recomputed on chip with
 * the forward's arithmetic (P_c, Q_c, R_c, M_c, gi, gh, r, z, n), then
 *   dn = dS' (1 - z), dz = dS' (S - n), dS = dS' z, pn = dn (1 - n^2), pz = dz z (1 - z), pr = pn gh_n r (1 - r),
 *   dgi = [pr, pz, pn], dgh = [pr, pz, pn r], dS += dgh Whh ; per channel c:
 *   dM_c = dgi Wih[:, cD:(c+1)D] (avg != 0: divided by deg_c[a] + FLT_EPSILON), dR_c = dM_c W2_c,
 *   act_c[a, b, h] = (L[a, b, c] != 0 and Q_c[a, h] + P_c[b, h] > 0), dQ_c[a, h] = dR_c[a, h] #{b: act_c[a, b, h]},
 *   dP_c[b, h] = sum over a (ascending) with act_c[a, b, h] of dR_c[a, h], dS += dP_c W1n_c + dQ_c W1s_c
 * W1, b1, .. bhh: the forward's operands; W1T [C][2][D][64] (W1T[c][0] = W1n_c^T, W1T[c][1] = W1s_c^T),
 * W2T [C][64][D], WihT [C][D][3 D] (block c = Wih[:, cD:(c+1)D]^T), WhhT [D][3 D]: their transposes, packed by
 * the caller.  Out: dS [B N, ldo] = dL/dS_t and the row-space operands of this step's weight gradients,
 * contiguous: dgi [B N][3 D], dghn [B N][D] (the n part of dgh; its r and z parts are dgi's), M [B N][C D] =
 * cat_c M_c, R [B N][C 64] = cat_c R_c, dM [B N][C D] (scaled), dPQ [B N][C][dP_c 64 | dQ_c 64].  The caller
 * contracts them over the rows (dWih = dgi^T M, dWhh = dgh^T S, dW2_c = dM_c^T R_c, db2_c = sum_a deg_c[a]
 * dM_c[a], dW1_c = [dP_c^T S | dQ_c^T S], db1_c = sum dQ_c, dbih, dbhh the column sums of dgi, dgh) and may reuse
 * the buffers for the next step.  The envelope of lnz_mpnn_forward (N <= 32, C <= 8, D a multiple of 32 and
 * <= 128: LNZ_ENOTSUP, as are rows that are not 16-byte aligned); null pointers, B or N <= 0, a row stride below
 * D, negative strides of L, an output overlapping an input or another output: LNZ_EINVAL.  L is read through
 * its four strides and never written.  32-row tiles, 147,072 B of dynamic LDS at D = 128; no atomics, every sum
 * in a fixed order: bit-reproducible. */
int lnz_mpnn_backward_step(const float* S, int lds, const float* dSnext, int ldd, const float* L, int64_t stride_b,
                           int64_t stride_r, int64_t stride_c, int64_t stride_ch, const float* W1, const float* b1,
                           const float* W2, const float* b2, const float* Wih, const float* bih, const float* Whh,
                           const float* bhh, const float* W1T, const float* W2T, const float* WihT,
                           const float* WhhT, int B, int N, int C, int D, int avg, float* dS, int ldo, float* dgi,
                           float* dghn, float* M, float* R, float* dM, float* dPQ, lnz_stream_t stream);

/* lnz_set2vec_readout: Set2Vec (model/set2set.py:79-100) and output_func in ONE launch.  Per molecule, with
 * X = the rows of X [B N, ld] where mask [B, N] != 0 (NULL: all N rows), q* [2 D] = 0, mem [D] = 0, num_step times
 *   f, i, o = sigmoid(W_f q* + b_f), sigmoid(W_i q* + b_i), sigmoid(W_o q* + b_o) ; g = tanh(W_m q* + b_m)
 *   mem = f mem + i g ; q = o tanh(mem) ; e_j = sum_f tanh((q W_1)_f + X_jf) W_2[f]
 *   w = softmax_j(e) over the set (max-subtracted) ; q* = [q, sum_j w_j X_j]
 * then score [B, P] = Wout q* + bout.  Wg [4][D][2 D] and bg [4][D] stack the forget, input, output and memory
 * gates; W1T [D][D] is W_1 TRANSPOSED (W1T[f][k] = W_1[k][f]), w2 [D], Wout [P][2 D], bout [P].  Rows outside
 * the set are never loaded (they may hold NaN); a molecule with an empty set reads exactly 0 (finite score);
 * num_step = 0: score = bout.  N <= 32, D a multiple of 32 and <= 128, 1 <= P <= 16, num_step >= 0, 16-byte
 * aligned rows (LNZ_ENOTSUP); null pointers, B or N <= 0, ld < D, score overlapping X, mols_per_group outside
 * 0 .. 16: LNZ_EINVAL.  mols_per_group = 0: as few molecules per workgroup as spread the batch over the compute
 * units, at most the 16 rows of an MFMA tile; 1 .. 16 force it — a molecule's arithmetic and bits do not depend
 * on it.  No atomics, every sum in a fixed order: bit-reproducible. */
int lnz_set2vec_readout(const float* X, int ld, const uint8_t* mask, const float* Wg, const float* bg,
                        const float* W1T, const float* w2, const float* Wout, const float* bout, int B, int N, int D,
                        int P, int num_step, float* score, int mols_per_group, lnz_stream_t stream);

/* ---- the GPNN baseline (model/gpnn.py:141-251, config/qm8_gpnn.yaml), csrc/gpnn.hip ----
 * All num_prop outer steps and the readout in ONE launch.  state0 [B N, ld0] is
 * input_func(embedding(node_feat)); with C = num_bond_type + 1 channels, state width D, message hidden width
 * 128 and state_func's hidden width 512, per outer step on the state S
 *   Sc = S; num_prop_cluster times Sc = part(Sc, L_cluster) ;  Sx = S; num_prop_cut times Sx = part(Sx, L_cut)
 *   part(X, Lp): M = relu(X W1_0^T + b1_0) W2_0^T + b2_0                           (msg_func[0])
 *                A = Ŵ M per molecule; Ŵ = Lp, for avg != 0 Ŵ[i, j] = Lp[i, j] / (sum_j Lp[i, j] + FLT_EPSILON)
 *                X' = GRUCell(A, X)           (update_func_partition: Wpih [3 D][D], bpih, Wphh [3 D][D], bphh)
 *   S = relu([S | Sc | Sx] Ws1^T + bs1) Ws2^T + bs2                  (state_func: Ws1 [512][3 D], Ws2 [D][512])
 *   S = one step of lnz_ggnn_forward on S     (msg_func[0 .. C-1]: W1 [C][128][D], b1, W2 [C][D][128], b2; L != 0;
 *                                              update_func: Wih [3 D][C D], bih, Whh [3 D][D], bhh)
 * then the readout of lnz_ggnn_forward (Wo [P][D], bo, wg [D], bg [1]; mask [B, N] u8, NULL: all N rows; no
 * masked row: NaN).  All N rows of a molecule take part.  L through its four strides as in lnz_ggnn_forward:
 * only compared with zero, a NaN or a negative entry is an edge.  L_cluster and L_cut (element (b, i, j) at
 * b cl_stride_b + i cl_stride_r + j cl_stride_c floats, ct_* likewise, strides >= 0) enter BY VALUE; the 'avg'
 * row sum runs j ascending in float32; non-finite entries are outside the contract.  None of the three is
 * written.  A count of 0 hands S itself to state_func in place of Sc / Sx; num_prop = 0: the readout of state0.
 * state_out [B N, ldso] (may be NULL) receives the final state.
 * 1 <= N <= 32, 1 <= C <= 8, D a multiple of 32 and <= 128, 1 <= P <= 16, the three counts >= 0, ld0 / ldso
 * multiples of 4, state0 / state_out / the weights 16-byte aligned, tile_rows = 64 (not built) (LNZ_ENOTSUP
 * otherwise); null pointers, B or N <= 0, ld0 / ldso below D, negative strides, score or state_out overlapping
 * state0 or each other, tile_rows other than 0, 32, 64: LNZ_EINVAL.  A workgroup holds S, Sc and Sx of
 * floor(32 / N) molecules in LDS for all steps (111,744 B of dynamic LDS at D = 128).  Exact-fp32 MFMA, no
 * atomics, every sum in a fixed order: bit-reproducible, and a molecule's bits do not depend on its place in the
 * batch.  lnz_last_kernel() names gpnn_forward_kernel<D, 2>. */
int lnz_gpnn_forward(const float* state0, int ld0, const float* L, int64_t stride_b, int64_t stride_r,
                     int64_t stride_c, int64_t stride_ch, const float* L_cluster, int64_t cl_stride_b,
                     int64_t cl_stride_r, int64_t cl_stride_c, const float* L_cut, int64_t ct_stride_b,
                     int64_t ct_stride_r, int64_t ct_stride_c, const uint8_t* mask, const float* W1,
                     const float* b1, const float* W2, const float* b2, const float* Wih, const float* bih,
                     const float* Whh, const float* bhh, const float* Wpih, const float* bpih, const float* Wphh,
                     const float* bphh, const float* Ws1, const float* bs1, const float* Ws2, const float* bs2,
                     const float* Wo, const float* bo, const float* wg, const float* bg, int B, int N, int C, int D,
                     int P, int num_prop, int num_prop_cluster, int num_prop_cut, int avg, float* score,
                     float* state_out, int ldso, int tile_rows, lnz_stream_t stream);


/* ---- next row (SURVEY.md 8f rank 1 + 3): device-side collate from a packed molecule shard ----
 * Replaces the per-molecule pickles of dataset/get_qm8_data.py:56-96 (dense float64 Laplacians +
 * offline eigendecomposition), their loading (dataset/qm8.py:41-47) and the Python pad/concat of
 * QM8Data.collate_fn (dataset/qm8.py:57-100,220-262).  A shard is four flat device arrays:
 *   mol_off  [n_mol+1] int64   atom offsets          atoms  [total_atoms] u8  atom ids
 *   edge_off [n_mol+1] int64   bond offsets          edges  [total_bonds] u32 = u | v<<8 | type<<16
 *   labels   [n_mol, P] fp32                         (each undirected bond listed once)
 * One launch builds the batch of molecules ids[0..B) (NULL = 0..B-1), padded to N nodes
 * (N >= the largest molecule of the batch, qm8.py:66):
 *   L [B,N,N,E+1] fp32 channels-last, channel 0 = L4 of the simple graph sum_e A_e
 *     (get_qm8_data.py:62), channel 1+e = L4 of bond type e (utils/data_helper.py:92-116,
 *     155-156, 261-291), computed in fp64 and rounded once — bit-identical to lnz_laplacian_l4
 *     on the dense adjacency;
 *   node_feat [B,N] int64 (pad 0), mask [B,N] u8, label [B,P], n_nodes [B] int32.
 * (D, V) then come from lnz_lanczos_ritz on L[..., 0] instead of the pickled D_simple/V_simple.
 * An id outside [0, n_mol) yields an empty molecule (n_nodes = 0, a zero label); a molecule of more
 * than N atoms is cut to its first N (bonds into the cut atoms are dropped, n_nodes = N).
 * N*N*E*4 + (E+1)*N*8 <= 64 KiB (LNZ_ENOTSUP beyond).  lnz_last_kernel() names collate_qm8_kernel. */
int lnz_collate_qm8(const int64_t* mol_off, const int64_t* edge_off, const uint8_t* atoms,
                    const uint32_t* edges, const float* labels, const int64_t* ids, int64_t n_mol,
                    int B, int N, int E, int P, int64_t* node_feat, uint8_t* mask, float* label,
                    float* L, int32_t* n_nodes, lnz_stream_t stream);

/* ---- R12: unsorted_segment_sum -----------------------------------------------------------
 * out[b, ids[b,c], x] += data[b,c,x]  /  grad_data[b,c,x] = grad_out[b, ids[b,c], x].
 * Replaces operators/src/cuda/segment_reduction.cu:39-69 (+ launchers :72-95) behind
 * operators/functions/unsorted_segment_sum.py:8-44.  `out` must be pre-zeroed by the caller
 * (as :25-26 does).  The output batch stride is num_segments*dim2 (the reference kernel's
 * dim1*dim2 stride, :48, is only in-bounds when num_segments == dim1; identical there).
 * An id outside [0, num_segments) contributes nothing forward and receives zeros backward (the
 * reference would write and read out of bounds).  lnz_last_kernel() names the forward's
 * segsum_fwd_lds_kernel<VEC> x NW (VEC floats per lane, the rows split over NW waves) or
 * segsum_fwd_atomic_kernel, and the backward's segsum_bwd_kernel<VEC>. */
int lnz_unsorted_segment_sum_forward(const float* data, const int64_t* segment_ids, int B,
                                     int dim1, int dim2, int num_segments, float* out,
                                     lnz_stream_t stream);
int lnz_unsorted_segment_sum_backward(const float* grad_out, const int64_t* segment_ids, int B,
                                      int dim1, int dim2, int num_segments, float* grad_data,
                                      lnz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LANCZOSNET_HIP_H_ */
