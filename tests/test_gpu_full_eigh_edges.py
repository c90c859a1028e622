"""The hand-written full eigendecomposition (lnz_sym_eigh_topk: csrc/sym_eigh.hip, and the bisection
and inverse-iteration bodies of csrc/tridiag_eig.hpp) held to float64 eigh at every kernel seam and
beyond L4 Laplacians.  Inputs: eigh_cases.py (pinned without a GPU by test_eigh_cases_cpu.py).

Reference: np.linalg.eigh of the float32 block in float64 + the stable |lambda| mergesort
(ritz_cases.eigh_ref).  Bars, the project's own, each relative to max |lambda| of the graph
(ritz_cases.check_bars, nothing skipped): |D - D_ref| < 1e-6, |V^T V - I| < 2e-6, |A V - V D| <
2e-6, spectral projectors of powers 1, 5, 30 within 1e-5; info == 0 everywhere.  The reference
rounded to float32 meets them with |V^T V - I| <= 8.3e-8 and |A V - V D| <= 4.8e-8 (24 times inside
the tightest bar; test_eigh_cases_cpu.py).

* seams      N in SEAM_N: the panel seams (NB = 32: n = 1, 2, 3 with no or one reflector, 31/32/33,
             63/64/65, 96/97, a last panel of one column at 129 and 193), the tile seams of the
             trailing product and update (TS = 64: 64/65, 128/129), passengers of n = 3, 2, 1, 0
             riding column launches whose j >= n, a diagonal and a tridiagonal input (Householder
             meets zero columns), K = 1, 15, 16, 17 around the KC = 16 back-transformation columns,
             min(N, 64) (n = 2K - 1, 2K, 2K + 1 of the candidate seam), K = MAX_K = 256 > n.
* spectra    spread + graded + paired at n = 65, 129; Wilkinson W+ at m = 16, 32, 48 in five forms;
             raw adjacency, L1 and L2 of small graphs.
* scale      the n = 65 spectra and Wilkinson m = 32 times 2^-60, 2^-20, 2^20, 2^60: the bars, and
             V bitwise equal / D an exact multiple of the unscaled run (every threshold is
             relative to ||T||).
* clusters   the zero matrix, 0.75 I, a diagonal of 20 values five times each, three copies of a
             43-node matrix: eigh_cases.check_clusters.
* split      one graph alone (inv_x = 64 workgroups share its clusters) and at three places of a
             batch of 300 (inv_x = 1): the same bits.
* entry      n_nodes None / beyond N / negative, a transposed view, a misaligned workspace.

Measured on an MI355X (worst figure of each family; D, orthogonality, residual, projector):
  seams                      0        7.4e-8   4.7e-8   1.8e-11
  spread, graded, paired     0        3.3e-8   2.5e-8   1.6e-13
  Wilkinson                  0        8.3e-8   3.0e-8   1.0e-7
  adjacency, L1, L2          4.4e-16  8.5e-8   1.8e-8   8.2e-8
  clustered                  0        7.1e-8   2.0e-8   6.5e-8   (containment 1.7e-8)
The scaled runs repeat the unscaled bits (no threshold with an absolute floor that matters was
found; with the cluster gap made absolute, test_gpu_full_eigh.py still passes and all four scale
cases fail).  The split changes no bit.

Found by `zero40`: the zero matrix came back with info = 2 — the failure test of the inverse
iteration, res <= 1e-9 max(||T||, 1e-300), lay below the residual of the -1.5 pivmin at which
bisection places a zero eigenvalue (csrc/tridiag_eig.hpp, invit_body); its floor is 4 pivmin now."""
import functools

import numpy as np
import pytest
import torch

import eigh_cases as ec
import ritz_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _eigh(A, ns, K):
  from lanczosnet_amd import ops
  D, V, info = ops.sym_eigh_topk(_t(A), None if ns is None else _t(ns), K, return_info=True)
  return D.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy()


def _sign_rule(ns, K, V, names):
  """The first entry of largest magnitude is positive (decided in fp64 on the device), up to the
  fp32 rounding of the output."""
  for b, n in enumerate(ns):
    kk = min(int(n), K)
    if kk:
      Vb = V[b, :n, :kk].astype(np.float64)
      assert (Vb.max(axis=0) >= np.abs(Vb).max(axis=0) * (1 - 1e-6)).all(), names[b]


def _held_to_the_bars(batch, run=None):
  """Every K of the batch through check_bars, info == 0 and the sign rule.  -> worst figures"""
  worst = np.zeros(4)
  for K in batch.Ks:
    D, V, info = (run or _eigh)(batch.A, batch.ns, K)
    assert D.shape == (len(batch.ns), K) and V.shape == (len(batch.ns), batch.A.shape[1], K)
    assert (info == 0).all(), (batch.label, K, info)
    fig = rc.check_bars(batch.A, batch.ns, K, D, V, ec.reference(batch.label, K), batch.names)
    _sign_rule(batch.ns, K, V, batch.names)
    print('%s K=%d: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  projector %.2e' % ((batch.label, K) + tuple(fig)))
    worst = np.maximum(worst, fig)
  print('%s worst: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  projector %.2e' % ((batch.label,) + tuple(worst)))
  return worst


# ------------------------------------------------------------------------------------------- seams
@pytest.mark.parametrize('N', ec.SEAM_N)
def test_panel_tile_candidate_and_k_seams(N):
  batch = [b for b in ec.seam_batches() if b.label == 'seam%d' % N][0]
  assert batch.A.shape[1] == N and batch.Ks == ec.seam_K(N)
  _held_to_the_bars(batch)


# ----------------------------------------------------------------------------------------- spectra
@pytest.mark.parametrize('label', [b.label for b in ec.spectra_batches()])
def test_spectra_beyond_l4_laplacians(label):
  """spread + graded + paired (n = 65, 129; K = 16, 64), Wilkinson W+ (m = 16, 32, 48; K = 16, 2m;
  five forms) and the operators that are no L4 Laplacian (K = 32)."""
  _held_to_the_bars([b for b in ec.spectra_batches() if b.label == label][0])


# ------------------------------------------------------------------------------------------- scale
@functools.lru_cache(maxsize=None)
def _unscaled(which, K):
  base = ec.scale_free_bases()[which]
  return _eigh(base.A, base.ns, K)


@pytest.mark.parametrize('s', ec.SCALES, ids=['2^%d' % int(np.log2(s)) for s in ec.SCALES])
def test_every_threshold_is_relative_to_the_norm(s):
  """A power-of-two multiple of the matrix is exact in every step where the thresholds (the split,
  pivmin, the bisection tolerance, the cluster gap, the pivot perturbation, the failure test) are
  relative to ||T||: the bars, V bit for bit that of the unscaled run, D its exact multiple."""
  for which in (0, 1):
    batch = ec.scaled_batch(which, s)
    kept = {}

    def run(A, ns, K):
      kept[K] = _eigh(A, ns, K)
      return kept[K]

    _held_to_the_bars(batch, run)
    for K in batch.Ks:
      D0, V0, _ = _unscaled(which, K)
      D, V, _ = kept[K]
      np.testing.assert_array_equal(V, V0, err_msg='%s K=%d' % (batch.label, K))
      np.testing.assert_array_equal(D, D0 * np.float32(s), err_msg='%s K=%d' % (batch.label, K))


# ---------------------------------------------------------------------------------------- clusters
@pytest.mark.parametrize('K', ec.CLUSTER_K)
def test_exact_multiplicities(K):
  """tnorm = 0, one cluster of K vectors, clusters of five on a diagonal input (T splits into 1 x 1
  blocks), and exact triples across blocks that straddle the panel seams (T does not split)."""
  cases = ec.clustered()
  A, ns = rc.pad_batch(cases)
  names = [c[0] for c in cases]
  D, V, info = _eigh(A, ns, K)
  fig = ec.check_clusters(A, ns, K, D, V, info, names, say=print)
  _sign_rule(ns, K, V, names)
  print('clustered K=%d worst: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  containment %.2e  projector %.2e'
        % ((K,) + tuple(fig)))


# ------------------------------------------------------------------------------------------- split
def test_the_inverse_iteration_split_does_not_change_a_bit():
  """inv_x = min(K, ceil(256 / B)) workgroups share a graph's clusters: 64 for a graph alone, one
  in a batch of 300.  paired(65) and W+_65 at K = 64 (real clusters: CGS2 against vectors that
  other workgroups would have computed if the split followed anything but the cluster) give the
  same D and V alone and as entry 0, 150 and 299 of the batch."""
  from lanczosnet_amd import ops
  n, K, B = 65, 64, 300
  assert min(K, (256 + 1 - 1) // 1) == 64 and min(K, (256 + B - 1) // B) == 1
  per = ops._abi().sym_eigh_topk_workspace_bytes(1, n, K)
  assert B * per <= ops.SYM_EIGH_WORKSPACE_CAP and B <= ops.SYM_EIGH_MAX_B      # one chunk
  sizes = np.random.RandomState(61).randint(1, n + 1, size=B)
  fill = [('fill%d' % i, rc.random_symmetric(int(m), 6100 + i)) for i, m in enumerate(sizes)]
  for name, M in (rc.paired(n)[0], rc.wilkinson(32, forms=('plain',))[0]):
    cases = list(fill)
    for at in (0, 150, B - 1):
      cases[at] = (name, M)
    A, ns = rc.pad_batch(cases, n)
    Ad, nd = _t(A), _t(ns)
    D1, V1, i1 = ops.sym_eigh_topk(Ad[:1], nd[:1], K, return_info=True)
    Db, Vb, ib = ops.sym_eigh_topk(Ad, nd, K, return_info=True)
    assert int(i1.abs().sum()) == 0 and int(ib.abs().sum()) == 0
    for at in (0, 150, B - 1):
      assert torch.equal(Db[at], D1[0]) and torch.equal(Vb[at], V1[0]), (name, at)
    one = [(name, M)]
    A1, n1 = rc.pad_batch(one, n)
    fig = rc.check_bars(A1, n1, K, D1.cpu().numpy(), V1.cpu().numpy(), rc.eigh_ref(A1, n1, K), [name], say=print)
    print('%s alone and in a batch of %d: the same bits; worst figures %s' % (name, B, fig))


# ------------------------------------------------------------------------------------------- entry
def test_entry_contract():
  """N = 33, K = 16: n_nodes = None is n_nodes = N; N + 5 and -2 are clamped to N and 0; of a
  transposed view (row stride 1) only the VIEW's lower triangle counts; a workspace that is not
  256-byte aligned is refused."""
  from lanczosnet_amd import ops
  N, K, B = 33, 16, 4
  A = np.stack([rc.random_symmetric(N, 7000 + i) for i in range(B)])
  Ad = _t(A)
  full = _t(np.full((B,), N, np.int32))
  D0, V0, i0 = ops.sym_eigh_topk(Ad, full, K, return_info=True)
  Dn, Vn, inn = ops.sym_eigh_topk(Ad, None, K, return_info=True)
  assert torch.equal(D0, Dn) and torch.equal(V0, Vn) and torch.equal(i0, inn)
  ns = np.full((B,), N, np.int32)
  fig = rc.check_bars(A, ns, K, D0.cpu().numpy(), V0.cpu().numpy(), rc.eigh_ref(A, ns, K))
  print('entry N=%d K=%d: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  projector %.2e' % ((N, K) + tuple(fig)))

  wild = _t(np.array([N + 5, -2, N, 0], np.int32))
  tame = _t(np.array([N, 0, N, 0], np.int32))
  Dw, Vw, iw = ops.sym_eigh_topk(Ad, wild, K, return_info=True)
  Dt, Vt, it = ops.sym_eigh_topk(Ad, tame, K, return_info=True)
  assert torch.equal(Dw, Dt) and torch.equal(Vw, Vt) and torch.equal(iw, it)
  assert torch.equal(Dw[0], D0[0]) and torch.equal(Vw[0], V0[0]) and int(iw.abs().sum()) == 0
  assert (Dw[1] == 0).all() and (Vw[1] == 0).all() and (Dw[3] == 0).all() and (Vw[3] == 0).all()

  M = np.random.RandomState(71).randn(B, N, N).astype(np.float32) / np.float32(np.sqrt(8.0 * N))
  assert not np.array_equal(M, M.transpose(0, 2, 1))            # deliberately unsymmetric storage
  view = _t(M).transpose(1, 2)
  assert view.stride(1) == 1 and view.stride(2) == N
  low = np.tril(M.transpose(0, 2, 1))                            # the view's lower triangle
  S = low + np.tril(M.transpose(0, 2, 1), -1).transpose(0, 2, 1)
  assert np.array_equal(S, S.transpose(0, 2, 1))
  Dv, Vv, iv = ops.sym_eigh_topk(view, full, K, return_info=True)
  Ds, Vs, is_ = ops.sym_eigh_topk(_t(S), full, K, return_info=True)
  assert torch.equal(Dv, Ds) and torch.equal(Vv, Vs) and torch.equal(iv, is_) and int(iv.abs().sum()) == 0
  fig = rc.check_bars(S, ns, K, Dv.cpu().numpy(), Vv.cpu().numpy(), rc.eigh_ref(S, ns, K))
  print('transposed view: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  projector %.2e' % tuple(fig))

  need = ops._abi().sym_eigh_topk_workspace_bytes(B, N, K)
  ws = torch.empty((need + 256,), dtype=torch.uint8, device=DEV)
  assert ws.data_ptr() % 256 == 0
  Da, Va = ops.sym_eigh_topk(Ad, full, K, workspace=ws[:need])
  assert torch.equal(Da, D0) and torch.equal(Va, V0)
  with pytest.raises(ops.LnzError):
    ops.sym_eigh_topk(Ad, full, K, workspace=ws[128:128 + need])
