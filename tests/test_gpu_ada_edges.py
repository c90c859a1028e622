"""The AdaLanczosNet stage kernels (csrc/ada_lanczos.hip, csrc/ada_lanczos_grad.hip) across the
envelope their launchers accept, each against a plain float64 reference (the numpy oracle, numpy,
or float64 torch autograd through the restatement of `lanczosnet_amd.model._ada`) — never against
another kernel.  tests/test_gpu_ada.py holds the same kernels at the one nominal point (K = 20,
S = 5, N <= 32); here: both instantiations of the Lanczos layer up to N = K = 64, the float64
layer and its reverse sweep at the sizes its arrays are dimensioned for, the T powers up to the
K = 64 / S = 16 / 160 KiB-LDS corner, the learned Laplacian in both precisions incl. its `pad`
branch, and the module at other `num_eig_vec` / `long_diffusion_dist`.

Every case prints its worst deviation; the figures measured on an MI355X stand next to the bars."""
import types

import numpy as np
import pytest
import torch

import oracle
from test_gpu_ada import _fixed_randn, _mol_err, _separation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS64 = 2.2e-16


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _gnp(rs, n, p):
  """Adjacency of G(n, p): symmetric 0/1, no self loops."""
  a = np.triu((rs.rand(n, n) < p).astype(np.float64), 1)
  return a + a.T


def _sizes(rs, B, lo, hi):
  """B sizes of lo .. hi; the two ends are always present."""
  n = rs.randint(lo, hi + 1, size=B)
  n[0], n[-1] = lo, hi
  return n


# =============================================================================================
# 1. Lanczos layer, fp32 in / fp32 out
# =============================================================================================
B1 = 24
#            N  n_lo n_hi  K    p   mask
LAYER_CASES = [(64, 33, 64, 64, 0.2, True),    # <64,64>, every array full
               (64, 33, 64, 20, 0.2, True),    # K < N on the wide instantiation
               (33, 20, 33, 33, 0.3, True),    # first size beyond <32,32> on both axes
               (32, 1, 32, 32, 0.3, True),     # <32,32> full; a one-node graph
               (32, 20, 32, 33, 0.3, True),    # K alone selects the wide instantiation
               (20, 5, 20, 64, 0.3, True),     # K > N: zero padding of T, Q to K
               (64, 40, 64, 53, 0.1, True),    # sparse graphs, odd K
               (48, 48, 48, 48, 0.2, False)]   # mask=None (null pointer path)


def _layer_inputs(N, n_lo, n_hi, K, p, use_mask):
  """L4 of G(n, p) zero padded to N, mask from n, q1 = randn; and the float64 oracle on them."""
  rs = np.random.RandomState(B1 + N + K)
  n = _sizes(rs, B1, n_lo, n_hi)
  A = np.zeros((B1, N, N), np.float32)
  mask = np.zeros((B1, N), np.uint8)
  for b in range(B1):
    A[b, :n[b], :n[b]] = oracle.laplacian_l4(_gnp(rs, int(n[b]), p))
    mask[b, :n[b]] = 1
  q1 = rs.randn(B1, N).astype(np.float32)
  mk = mask if use_mask else None
  T64, Q64, braw = oracle.ada_lanczos_layer(A, mk, q1, K, dtype=np.float64, return_raw_betas=True)
  return A, mk, q1, T64, Q64, _separation(braw)


@pytest.mark.parametrize('N,n_lo,n_hi,K,p,use_mask', LAYER_CASES)
def test_lanczos_layer_both_instantiations_match_the_float64_oracle(N, n_lo, n_hi, K, p, use_mask):
  """`ops.ada_lanczos_layer` (ada_lanczos_layer_kernel<32,32> for N, K <= 32, else <64,64>) against
  `oracle.ada_lanczos_layer(dtype=float64)`.  Held to the bar: the molecules whose breakdown
  decisions are stable (no raw beta within 10x of the 1e-4 threshold, `_separation`); at least 18
  of the 24 must be (asserted: a bad seed fails, it does not hide behind the filter).  On those the
  zero pattern of T and Q is the oracle's exactly and every value lies within 1e-5 of the
  molecule's largest entry (the kernel's recurrence is float64, its output one fp32 rounding:
  6e-8; the float64 oracle itself moves by <= 1.4e-8 on T under a node permutation).
  Measured on the MI355X: worst T 9.4e-8 (N = 64, K = 53), worst Q 6.6e-8 over the eight cases;
  20 .. 24 of the 24 molecules separated."""
  from lanczosnet_amd import ops
  A, mk, q1, T64, Q64, sep = _layer_inputs(N, n_lo, n_hi, K, p, use_mask)
  T, Q = ops.ada_lanczos_layer(_t(A), None if mk is None else _t(mk), _t(q1), K)
  assert tuple(T.shape) == (B1, K, K) and tuple(Q.shape) == (B1, N, K)
  T, Q = T.cpu().numpy(), Q.cpu().numpy()
  ok = sep >= 10
  eT, eQ = _mol_err(T, T64), _mol_err(Q, Q64)
  print('lanczos layer N=%d K=%d mask=%s: %d of %d molecules separated, worst T %.2e, worst Q %.2e '
        '(the others: T %.2e, Q %.2e)' % (N, K, use_mask, ok.sum(), B1, eT[ok].max(), eQ[ok].max(),
                                          eT[~ok].max() if (~ok).any() else 0.0,
                                          eQ[~ok].max() if (~ok).any() else 0.0))
  assert ok.sum() >= 18, ok.sum()
  assert np.isfinite(T).all() and np.isfinite(Q).all()
  np.testing.assert_array_equal((T != 0)[ok], (T64 != 0)[ok])
  np.testing.assert_array_equal((Q != 0)[ok], (Q64 != 0)[ok])
  assert eT[ok].max() < 1e-5, (np.where(ok & (eT >= 1e-5))[0], eT[ok].max())
  assert eQ[ok].max() < 1e-5, (np.where(ok & (eQ >= 1e-5))[0], eQ[ok].max())


@pytest.mark.parametrize('N,K', [(65, 20), (20, 65)])
def test_lanczos_layer_refuses_beyond_64(N, K):
  from lanczosnet_amd import ops
  A = torch.zeros((2, N, N), device=DEV)
  with pytest.raises(ops.NotSupported, match='exceed 64'):
    ops.ada_lanczos_layer(A, None, torch.ones((2, N), device=DEV), K)


# =============================================================================================
# 2. T powers and symmetrise, fp32 surface
# =============================================================================================
DIST16 = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32, 48, 64]
DISTS = [[1], [5, 7, 10, 20, 30], [30, 5, 20], DIST16]


def _sym_T(K, B, seed):
  """[B, K, K] float64, symmetric, spectral norm 0.9."""
  rs = np.random.RandomState(seed)
  T = rs.randn(B, K, K)
  T = T + T.transpose(0, 2, 1)
  return T * (0.9 / np.abs(np.linalg.eigvalsh(T)).max(axis=1))[:, None, None]


def _powers_ref(T, dist):
  """Sequential float64 products TT = TT @ T; [B, S, K, K]: one slot per GIVEN exponent, in the
  order given."""
  T = np.asarray(T, np.float64)
  out, TT = {}, T
  for ii in range(1, max(dist) + 1):
    if ii in dist:
      out[ii] = TT
    TT = TT @ T
  return np.stack([out[p] for p in dist], axis=1)


def _slot_err(tcat, ref):
  """tcat [B, K, S*K] (cat on dim 2) against ref [B, S, K, K]: per molecule and slot, relative to
  that slot's largest entry."""
  B, S, K, _ = ref.shape
  got = np.asarray(tcat, np.float64).reshape(B, K, S, K).transpose(0, 2, 1, 3)
  d = np.abs(got - ref).reshape(B, S, -1).max(axis=2)
  return d / np.abs(ref).reshape(B, S, -1).max(axis=2)


@pytest.mark.parametrize('dist', DISTS, ids=lambda d: 'S%d_p%d' % (len(d), d[0]))
@pytest.mark.parametrize('K', [1, 20, 52, 53, 64])
def test_t_powers_fp32_surface_matches_sequential_float64_products(K, dist):
  """`ops.ada_t_powers`: slot s holds T^dist[s] in the order given (also unsorted), float64
  products rounded once to fp32 (2^-24 = 6e-8): 1e-6 of the slot's largest entry, a margin of 16x.
  3 K K 8 bytes of dynamic LDS: 64 896 B at K = 52, 67 416 B at K = 53, 96 KiB at K = 64 — beyond
  64 KiB csrc/common.hpp requires the grant (LNZ_DYNAMIC_LDS), and the launcher asks for it like
  its float64 twins.  Outcome on the MI355X (ROCm 7): K = 53 and K = 64 give the right powers; a
  build of the launcher WITHOUT the grant launched there too and gave the same values (3.6e-9
  absolute from float64) — this runtime does not enforce the opt-in, the next one may.
  Measured on the MI355X: worst slot 5.9e-8 over the twenty cases."""
  from lanczosnet_amd import ops
  T32 = _sym_T(K, 3, 100 * K + len(dist)).astype(np.float32)
  ref = _powers_ref(T32, dist)
  got = ops.ada_t_powers(_t(T32), dist)
  assert tuple(got.shape) == (3, K, len(dist) * K)
  e = _slot_err(got.cpu().numpy(), ref)
  print('T powers fp32 K=%d dist=%r: worst slot %.2e' % (K, dist, e.max()))
  assert e.max() < 1e-6, e.max(axis=0)


BAD_DISTS = [[0], [5, 0, 7], [-1, 3], [1, 4097], [4097, 2]]


def test_t_powers_refusals():
  """S = 17 or K = 65: NotSupported.  An exponent < 1 or > 4096 ANYWHERE in the list: LnzError,
  on the fp32 entry and on the float64 pair (a slot whose exponent the kernel's loop never reaches
  would come back as uninitialised memory)."""
  from lanczosnet_amd import ops
  T = _t(_sym_T(4, 2, 0))
  with pytest.raises(ops.NotSupported):
    ops.ada_t_powers(T.float(), list(range(1, 18)))
  with pytest.raises(ops.NotSupported):
    ops.ada_t_powers(torch.zeros((1, 65, 65), device=DEV), [1, 2])
  with pytest.raises(ops.NotSupported):
    ops.ada_t_powers_f64(T, list(range(1, 18)))
  with pytest.raises(ops.NotSupported):
    ops.ada_t_powers_f64(torch.zeros((1, 65, 65), dtype=torch.float64, device=DEV), [1, 2])
  for dist in BAD_DISTS:
    S = len(dist)
    for call in (lambda: ops.ada_t_powers(T.float(), dist),
                 lambda: ops.ada_t_powers_f64(T, dist),
                 lambda: ops.ada_t_powers_f64_backward(
                     (T, torch.zeros((2, 8, 4, 4), dtype=torch.float64, device=DEV), tuple(dist)),
                     torch.zeros((2, 4, S * 4), device=DEV))):
      with pytest.raises(ops.LnzError, match='bad exponents') as ei:
        call()
      assert not isinstance(ei.value, ops.NotSupported), dist


@pytest.mark.parametrize('K,S', [(1, 1), (20, 5), (64, 16)])
def test_symmetrize_filters_bit_equal_to_numpy(K, S):
  """`ops.ada_symmetrize_filters`: bit-equal to numpy float32 (x + y) * 0.5 in the [B,S,K,K] layout."""
  from lanczosnet_amd import ops
  B = 3
  DD = np.random.RandomState(K + S).randn(B, K * K * S).astype(np.float32)
  got = ops.ada_symmetrize_filters(_t(DD), K, S).cpu().numpy()
  D4 = DD.reshape(B, K, K, S)
  ref = ((D4 + D4.transpose(0, 2, 1, 3)) * np.float32(0.5)).transpose(0, 3, 1, 2)
  assert ref.dtype == np.float32 and got.shape == (B, S, K, K)
  np.testing.assert_array_equal(got, ref)
  print('symmetrise K=%d S=%d: bit-equal' % (K, S))


# =============================================================================================
# 3. float64 Lanczos layer and its backward
# =============================================================================================
def _ref_lanczos(Le, mask, q1, K):
  """`AdaLanczosNet._torch_ada_lanczos`, the float64 torch restatement of the layer, on a stand-in
  that carries only what the method reads: no 50 M-parameter filter MLPs per case."""
  from lanczosnet_amd.model import AdaLanczosNet
  ns = types.SimpleNamespace(num_eig_vec=K, use_reorthogonalization=True)
  return AdaLanczosNet._torch_ada_lanczos(ns, Le, mask, q1)


def _ref_laplacian64(X64, adj):
  """model/ada_lanczos_net.py:101-137 on a float64 state (as `_torch_ada_laplacian`)."""
  B = X64.shape[0]
  diff = X64.unsqueeze(1) - X64.unsqueeze(2)
  dist2 = (diff * diff).sum(dim=3)
  sigma2 = dist2.reshape(B, -1).mean(dim=1).view(B, 1, 1)
  A = torch.exp(-dist2 / sigma2) * adj
  rs = A.sum(dim=2, keepdim=True)
  Dg = 1.0 / (rs + (rs == 0).double()).pow(0.5)
  return Dg * A * Dg.transpose(1, 2)


def _molecule_batch(B, n_lo, n_hi, N, seed):
  """Synthetic molecules (random trees + ring closures) of n_lo .. n_hi atoms padded to N: atom
  ids, node mask, the adjacency mask of the simple-graph L4 (edges + the diagonal of real nodes)."""
  from lanczosnet_amd.synthetic import draw_molecule
  rs = np.random.RandomState(seed)
  n = _sizes(rs, B, n_lo, n_hi)
  ids = np.zeros((B, N), np.int64)
  mask = np.zeros((B, N), np.uint8)
  adj = np.zeros((B, N, N), np.float32)
  for b in range(B):
    nb = int(n[b])
    adj[b, :nb, :nb] = (draw_molecule(rs, nb).sum(axis=2) + np.eye(nb)) != 0
    ids[b, :nb] = rs.randint(0, 70, size=nb)
    mask[b, :nb] = 1
  return ids, mask, adj


def _learned_laplacian64(ids, adj, seed):
  emb = torch.from_numpy(np.random.RandomState(seed).randn(70, 70)).to(DEV)
  return _ref_laplacian64(emb[_t(ids)], _t(adj).double()).contiguous()


def _with_self_deviation(tag, err, bar, d_ref_fn):
  """The bar of a float64 comparison.  Where a case exceeds the existing bar, the bar is not moved
  by eye: the reference's own deviation d_ref under a relative perturbation of its input by
  2.2e-16 randn is measured here, on the device, and the case is held to max(bar, 10 d_ref) (10:
  another summation order over up to 32 steps).  Both numbers are printed."""
  if err <= bar:
    return bar
  d_ref = float(d_ref_fn())
  print('%s: %.2e exceeds the bar %.1e; the reference itself moves by d_ref = %.2e under a 2.2e-16 '
        'perturbation of its input: held to max(bar, 10 d_ref) = %.2e'
        % (tag, err, bar, d_ref, max(bar, 10.0 * d_ref)))
  return max(bar, 10.0 * d_ref)


#             B  n_lo n_hi  N   K   mask
F64_CASES = [(8, 32, 32, 32, 32, True),     # N = K = 32: every [33] / [34] array full
             (16, 1, 32, 32, 32, True),     # padded to N = 32, a one-node graph
             (16, 8, 26, 26, 31, True),
             (16, 20, 32, 32, 16, True),    # K < N
             (16, 3, 12, 12, 32, True),     # K > N
             (16, 8, 26, 26, 1, True),      # K = 1: Q does not depend on Le
             (16, 26, 26, 26, 20, False)]   # mask=None (null pointer path), every node real
# (mask=None over PADDED nodes is no test case: the start vector then has a component in the null
#  space of the zero rows, several late betas of one molecule land just above the 1e-4 threshold,
#  and the float64 restatement itself moves by 0.5 in Q under a 2.2e-16 perturbation of Le)


@pytest.mark.parametrize('B,n_lo,n_hi,N,K,use_mask', F64_CASES)
def test_lanczos_layer_f64_and_backward_at_the_array_bounds(B, n_lo, n_hi, N, K, use_mask):
  """lnz_ada_lanczos_layer_f64 / _backward against `_torch_ada_lanczos` and float64 autograd
  through it (random gT, gQ), on learned Laplacians of synthetic molecules: forward 1e-11 (T
  relative to max(1, max|T|), Q absolute), gradient 1e-9 of its largest entry — the bars of
  tests/test_gpu_ada.py, there measured at K = 20 only.  (The restatement's own conditioning at
  these shapes, Le against Le (1 + 2.2e-16 randn): Q moves by up to 4e-12, the gradient by up to
  4e-11 of its largest entry.)  K = 1: Q = q1 masked and normalised does not depend on Le, the
  autograd reference takes T alone and dLe must come from dT alone, whatever gQ holds.
  Measured on the MI355X: forward T 7.3e-14, Q 6.3e-13, gradient 7.6e-12 (worst of the seven cases,
  all at N = K = 32; K = 16 < N: 3.1e-14): no case needed the rule of `_with_self_deviation`."""
  from lanczosnet_amd import ops
  ids, mask, adj = _molecule_batch(B, n_lo, n_hi, N, seed=1000 * B + 10 * N + K)
  Le = _learned_laplacian64(ids, adj, seed=K)
  torch.manual_seed(N + K)
  q1 = torch.randn(B, N, 1).to(DEV)
  mask_ref = _t(mask) if use_mask else torch.ones((B, N), dtype=torch.uint8, device=DEV)

  def reference(Lx, grads=None):
    Lx = Lx.clone().requires_grad_(True)
    T_t, Q_t = _ref_lanczos(Lx, mask_ref, q1, K)
    if grads is None:
      return T_t.detach(), Q_t.detach()
    outs, gs = ([T_t], grads[:1]) if K == 1 else ([T_t, Q_t], list(grads))
    return T_t.detach(), Q_t.detach(), torch.autograd.grad(outs, [Lx], gs)[0]

  T_h, Q_h, ws = ops.ada_lanczos_layer_f64(Le, _t(mask) if use_mask else None, q1, K)
  assert tuple(T_h.shape) == (B, K, K) and tuple(Q_h.shape) == (B, N, K)
  gT, gQ = torch.randn_like(T_h), torch.randn_like(Q_h)
  T_t, Q_t, want = reference(Le, (gT, gQ))
  got = ops.ada_lanczos_layer_f64_backward(Le, ws, gT, gQ)
  assert torch.isfinite(want).all() and torch.isfinite(got).all() and torch.isfinite(Q_h).all()
  Lp = Le * (1.0 + EPS64 * torch.randn_like(Le))
  eT = float((T_h - T_t).abs().max()) / max(1.0, float(T_t.abs().max()))
  eQ = float((Q_h - Q_t).abs().max())
  scale = float(want.abs().max())
  assert scale > 0
  eG = float((got - want).abs().max()) / scale
  print('f64 Lanczos layer B=%d N=%d K=%d mask=%s: forward T %.2e Q %.2e, gradient %.2e of the '
        'largest entry' % (B, N, K, use_mask, eT, eQ, eG))
  tag = 'f64 Lanczos layer N=%d K=%d' % (N, K)
  bT = _with_self_deviation(tag + ' T', eT, 1e-11, lambda: (reference(Lp)[0] - T_t).abs().max()
                            / max(1.0, float(T_t.abs().max())))
  bQ = _with_self_deviation(tag + ' Q', eQ, 1e-11, lambda: (reference(Lp)[1] - Q_t).abs().max())
  bG = _with_self_deviation(tag + ' gradient', eG, 1e-9,
                            lambda: (reference(Lp, (gT, gQ))[2] - want).abs().max() / scale)
  assert eT <= bT, (eT, bT)
  assert eQ <= bQ, (eQ, bQ)
  assert eG <= bG, (eG, bG)


@pytest.mark.parametrize('N,K', [(33, 20), (20, 33)])
def test_lanczos_layer_f64_refuses_beyond_32(N, K):
  from lanczosnet_amd import ops
  Le = torch.zeros((2, N, N), dtype=torch.float64, device=DEV)
  q1 = torch.ones((2, N, 1), device=DEV)
  with pytest.raises(ops.NotSupported, match='exceed 32'):
    ops.ada_lanczos_layer_f64(Le, None, q1, K)
  ws = torch.zeros((2 * 8192,), dtype=torch.float64, device=DEV)
  with pytest.raises(ops.NotSupported, match='exceed 32'):
    ops.ada_lanczos_layer_f64_backward(Le, ws, torch.zeros((2, K, K), dtype=torch.float64, device=DEV),
                                       torch.zeros((2, N, K), dtype=torch.float64, device=DEV))


# =============================================================================================
# 4. learned Laplacian, both precisions
# =============================================================================================
def _laplacian_inputs(N, D, B=6):
  """Atom ids + an embedding table [70, D]; adjacency masks of G(n, 0.3) with the diagonal of the
  real nodes set, padded nodes in every graph but the last (they count in sigma2, as in the
  reference), and in graph 0 a REAL node with an empty row and column: row sum 0, the `pad`
  branch, next to the padded rows that take it too."""
  rs = np.random.RandomState(7 * N + D)
  n = _sizes(rs, B, max(2, N // 2), N)
  n[0] = max(2, N - 1)
  ids = np.zeros((B, N), np.int64)
  adj = np.zeros((B, N, N), np.float32)
  for b in range(B):
    nb = int(n[b])
    adj[b, :nb, :nb] = _gnp(rs, nb, 0.3) + np.eye(nb)
    ids[b, :nb] = rs.randint(0, 70, size=nb)
  adj[0, 1, :] = 0
  adj[0, :, 1] = 0
  emb = rs.randn(70, D).astype(np.float32)
  return ids, emb, adj


@pytest.mark.parametrize('N,D', [(33, 70), (64, 128), (5, 1)])
def test_learned_laplacian_fp32_matches_the_float64_oracle(N, D):
  """`ops.ada_graph_laplacian`, id + embedding form and float-feature form, against
  `oracle.ada_graph_laplacian(dtype=float64)`.  The kernel's arithmetic is fp32 (the mean of
  dist2 and the row sums accumulate in float64), so the bar comes from the fp32 run of the same
  oracle: with e32 its distance from the float64 run, max(1e-5, 3 e32), per molecule relative to
  its largest entry.
  Measured on the MI355X: worst 2.0e-7 (e32 1.9e-7 .. 2.3e-7), both forms bit-identical."""
  from lanczosnet_amd import ops
  ids, emb, adj = _laplacian_inputs(N, D)
  X = emb[ids]
  ref = oracle.ada_graph_laplacian(X, adj, dtype=np.float64)
  assert (ref[0, 1] == 0).all() and (ref[0, :, 1] == 0).all() and np.isfinite(ref).all()
  e32 = _mol_err(oracle.ada_graph_laplacian(X, adj, dtype=np.float32), ref).max()
  bar = max(1e-5, 3.0 * e32)
  L0 = _t(adj)
  a = ops.ada_graph_laplacian(_t(ids), _t(emb), L0).cpu().numpy()
  b = ops.ada_graph_laplacian(_t(X), None, L0).cpu().numpy()
  ea, eb = _mol_err(a, ref).max(), _mol_err(b, ref).max()
  print('learned Laplacian fp32 N=%d D=%d: ids + embedding %.2e, float features %.2e (fp32 oracle '
        'vs float64 oracle e32 = %.2e, bar %.2e)' % (N, D, ea, eb, e32, bar))
  np.testing.assert_array_equal(a, b)
  np.testing.assert_array_equal(a != 0, ref != 0)
  assert ea <= bar and eb <= bar, (ea, eb, bar)
  # a strided view of the operand (the module passes L[:, :, :, 0])
  L4 = torch.zeros((adj.shape[0], N, N, 3), device=DEV)
  L4[:, :, :, 0] = L0
  c = ops.ada_graph_laplacian(_t(ids), _t(emb), L4[:, :, :, 0]).cpu().numpy()
  np.testing.assert_array_equal(c, a)


@pytest.mark.parametrize('N,D', [(32, 128), (40, 70), (5, 1)])
def test_learned_laplacian_f64_and_backward_match_float64_autograd(N, D):
  """lnz_ada_graph_laplacian_f64 / _backward against the float64 restatement and autograd through
  it (random upstream gradient): forward 1e-12, gradient 1e-10 of its largest entry — the bars of
  tests/test_gpu_ada.py.
  Measured on the MI355X: forward 2.2e-16, gradient 2.2e-15."""
  from lanczosnet_amd import ops
  ids, emb, adj = _laplacian_inputs(N, D)
  X = _t(emb[ids])
  L0 = _t(adj)
  Le_h, saved = ops.ada_graph_laplacian_f64(X, L0)
  st64 = X.double().requires_grad_(True)
  Le_t = _ref_laplacian64(st64, L0.double())
  torch.manual_seed(N + D)
  gL = torch.randn_like(Le_t)
  want, = torch.autograd.grad([Le_t], [st64], [gL])
  got = ops.ada_graph_laplacian_f64_backward(saved, gL)
  eF = float((Le_h - Le_t.detach()).abs().max())
  eG = float((got - want).abs().max() / want.abs().max())
  print('learned Laplacian f64 N=%d D=%d: forward %.2e, gradient %.2e of the largest entry' % (N, D, eF, eG))
  assert torch.isfinite(got).all() and (Le_h[0, 1] == 0).all()
  assert eF < 1e-12, eF
  assert eG < 1e-10, eG


def test_learned_laplacian_f64_refuses_beyond_its_lds_limit():
  """N = 64, D = 128: the forward needs 98 816 B, the backward 132 096 B of LDS — beyond the
  launchers' 96 KiB: NotSupported, nothing launched."""
  from lanczosnet_amd import ops
  B, N, D = 2, 64, 128
  X = torch.zeros((B, N, D), device=DEV)
  L0 = torch.zeros((B, N, N), device=DEV)
  with pytest.raises(ops.NotSupported, match='too large'):
    ops.ada_graph_laplacian_f64(X, L0)
  # (the forward refuses, so the backward's saved state [B][2 N N + N + 1] is made by hand)
  for Nb in (64, 56):   # N = 56: the forward's 82 880 B fit, the backward's 108 416 B do not
    sv = torch.zeros((B * (2 * Nb * Nb + Nb + 1),), dtype=torch.float64, device=DEV)
    with pytest.raises(ops.NotSupported, match='too large'):
      ops.ada_graph_laplacian_f64_backward((torch.zeros((B, Nb, D), device=DEV), sv),
                                           torch.zeros((B, Nb, Nb), dtype=torch.float64, device=DEV))


# =============================================================================================
# 5. float64 T powers
# =============================================================================================
@pytest.mark.parametrize('dist', [[1], [5, 7, 10, 20, 30], DIST16], ids=lambda d: 'S%d' % len(d))
@pytest.mark.parametrize('K', [1, 20, 32, 64])
def test_t_powers_f64_and_backward_match_float64_autograd(K, dist):
  """lnz_ada_t_powers_f64 / _backward against sequential float64 products and autograd through
  them (random upstream gradient, fp32 like the kernel's operand): forward 1e-6 of the slot's
  largest entry (one fp32 rounding of the output), gradient 1e-10 of its largest entry.
  K = 64: the backward asks for 5 x 64 x 64 x 8 B = exactly 160 KiB of dynamic LDS, all a
  workgroup can have.  Accepted: the right gradient, or NotSupported with the launcher's message
  about the grant — never a bare launch error, never a wrong result.  Outcome on the MI355X: the
  grant is given and the gradient is right (5.6e-16 at K = 64, S = 16).
  Measured on the MI355X: forward 5.5e-8 (worst slot), gradient 5.6e-16; no case needed the rule
  of `_with_self_deviation`."""
  from lanczosnet_amd import ops
  B = 3
  T = _t(_sym_T(K, B, 200 * K + len(dist)))

  def reference(Tx, g):
    Tx = Tx.clone().requires_grad_(True)
    out, TT = {}, Tx
    for ii in range(1, max(dist) + 1):
      if ii in dist:
        out[ii] = TT
      TT = torch.bmm(TT, Tx)
    tc = torch.cat([out[p] for p in dist], dim=2)
    return tc.detach(), torch.autograd.grad([tc], [Tx], [g])[0]

  tc_h, saved = ops.ada_t_powers_f64(T, dist)
  assert tc_h.dtype == torch.float32 and tuple(tc_h.shape) == (B, K, len(dist) * K)
  torch.manual_seed(K + len(dist))
  g32 = torch.randn((B, K, len(dist) * K), device=DEV)
  tc_t, want = reference(T, g32.double())
  eF = _slot_err(tc_h.cpu().numpy(), tc_t.cpu().numpy().reshape(B, K, len(dist), K).transpose(0, 2, 1, 3)).max()
  assert torch.equal(saved[1][:, 0], T)   # the saved powers (what the backward reads) start at T
  try:
    got = ops.ada_t_powers_f64_backward(saved, g32)
  except ops.NotSupported as e:
    assert K == 64 and 'bytes of dynamic LDS per workgroup are not available' in str(e), e
    print('T powers f64 K=%d S=%d: forward %.2e; backward refused: %s' % (K, len(dist), eF, e))
    assert eF < 1e-6, eF
    return
  scale = float(want.abs().max())
  eG = float((got - want).abs().max()) / scale
  print('T powers f64 K=%d S=%d: forward worst slot %.2e, gradient %.2e of the largest entry'
        % (K, len(dist), eF, eG))
  assert torch.isfinite(got).all()
  assert eF < 1e-6, eF
  Tp = T * (1.0 + EPS64 * torch.randn_like(T))
  bG = _with_self_deviation('T powers f64 K=%d S=%d gradient' % (K, len(dist)), eG, 1e-10,
                            lambda: (reference(Tp, g32.double())[1] - want).abs().max() / scale)
  assert eG <= bG, (eG, bG)


# =============================================================================================
# 6. through the module
# =============================================================================================
@pytest.mark.parametrize('dist', [[5, 7, 10, 20, 30], [1, 2, 3]], ids=lambda d: 'S%d' % len(d))
@pytest.mark.parametrize('K', [32, 12, 18])
def test_module_scores_at_other_num_eig_vec_and_scales(K, dist):
  """`AdaLanczosNet` in eval mode (2 layers x 128) at `num_eig_vec` 32, 12, 18 (18 % 4 != 0) and two
  lists of long scales, against `oracle.ada_lanczos_net_forward(dtype=float64)` with the same
  parameters and start vectors.  Per molecule with stable breakdown decisions (sep >= 10, at
  least 12 of the 16: asserted): no further from the float64 oracle than 3 e32 + 1e-5, e32 being
  that molecule's distance between the fp32 run and the float64 run of the oracle — the "add no
  noise" rule of tests/test_gpu_ada.py with the oracle in the reference's place.  Whichever route
  the module takes has to give these scores; it is printed.
  Measured on the MI355X: all six on the HIP kernels; worst 3.4e-6 (K = 32, e32 there 2.7e-6), never
  beyond 3 e32 (worst e - 3 e32: -7.7e-8); 13 .. 15 of the 16 molecules separated."""
  import warnings
  from lanczosnet_amd.model import AdaLanczosNet
  from lanczosnet_amd.synthetic import draw_batch
  from lanczosnet_amd.utils.arg_helper import make_model_config
  cfg = dict(oracle.DEFAULT_QM8_CFG, short_diffusion_dist=[1, 2, 3], long_diffusion_dist=list(dist),
             hidden_dim=[128, 128], num_layer=2, num_eig_vec=K)
  P = oracle.make_ada_params(cfg, 11)
  net = AdaLanczosNet(make_model_config(cfg, name='AdaLanczosNet')).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV)
  Bm = 16
  # The batch / start-vector seed is picked per list of scales on the float64 oracle's raw betas
  # alone (nothing of the code under test), so that the condition holds: at num_eig_vec = 32 > n
  # every molecule runs until its Krylov space is exhausted, and of a random batch only about half
  # the molecules keep every late beta 10x away from the threshold.
  seed = {5: 8, 3: 11}[len(dist)]
  b = draw_batch(Bm, seed=seed, n_min=8, n_max=26)
  N = b['node_mask'].shape[1]
  L = np.zeros((Bm, N, N, 7), np.float32)
  for i in range(Bm):
    n = int(b['n_nodes'][i])
    L[i, :n, :n] = oracle.laplacian_multi_l4(b['adjs'][i, :n, :n])
  q1 = np.random.RandomState(seed).randn(Bm, N).astype(np.float32)
  s64, _, braw = oracle.ada_lanczos_net_forward(P, cfg, b['node_feat'], L, b['node_mask'], q1,
                                                dtype=np.float64, return_raw_betas=True)
  s32, _ = oracle.ada_lanczos_net_forward(P, cfg, b['node_feat'], L, b['node_mask'], q1,
                                          dtype=np.float32)
  why = net._off_nominal(N, False)
  with warnings.catch_warnings(), _fixed_randn(q1), torch.no_grad():
    warnings.simplefilter('ignore')
    score = net(_t(b['node_feat']), _t(L), mask=_t(b['node_mask'])).cpu().numpy()
  scale = np.abs(s64).max(axis=1)
  e32 = np.abs(s32 - s64).max(axis=1) / scale
  e_our = np.abs(score - s64).max(axis=1) / scale
  ok = _separation(braw) >= 10
  print('module K=%d long scales %r: route %s; %d of %d molecules separated, worst %.2e (e32 there up to '
        '%.2e, worst beyond 3 e32: %.2e); the others: %.2e'
        % (K, dist, 'HIP kernels' if not why else 'torch restatement (%s)' % why, ok.sum(), Bm,
           e_our[ok].max(), e32[ok].max(), (e_our - 3 * e32)[ok].max(),
           e_our[~ok].max() if (~ok).any() else 0.0))
  assert ok.sum() >= 12, ok.sum()
  assert np.isfinite(score).all()
  bad = np.where(ok & (e_our > 3.0 * e32 + 1e-5))[0]
  assert len(bad) == 0, (bad, e_our[bad], e32[bad])
