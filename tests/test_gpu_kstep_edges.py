"""GPU checks of the K-step Lanczos kernels beyond L4 spectra of norm 1 (csrc/lanczos_large.hip: dense
stream, symmetric stream, sliced-ELL image; csrc/lanczos_wide.hip), on the inputs of
tests/kstep_cases.py — every case through every entry:

  large      ops.lanczos_ritz_large (a full tile; a ragged one: the same kernel behind
             ops.lanczos_ritz_kstep(symmetric=False, compact=False), which passes n_nodes)
  large_sym  the same with symmetric=True
  compact    ops.lanczos_ritz_kstep(compact=True): the steps on the image
  pair       ... on channel 0 of a channels-last [B, N, N, 2] block, read in place
  wide       lnz_lanczos_ritz_kstep_wide, the raw entry (ops routes N <= 2048, M <= 64 elsewhere)

(a) a full Krylov space against float64 eigh, (b) multiplicities, (c) M < n against the float64
restatement with the kernels' rules, (d) powers of two.  The rules (lnz::CgsBound for the second
Gram-Schmidt pass, the stop relative to the matrix' scale: DESIGN.md 4.5h) are what these inputs
changed: with the 1 - 1e-6 fraction alone and the absolute 1e-8 the kernels lost the basis on L1, L2
and spread spectra and stopped after one step on a matrix times 2^-30 (test_kstep_cases_cpu.py shows
both on the restatement)."""
import numpy as np
import pytest
import torch

import kstep_cases as kc
import ritz_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ENTRIES = ('large', 'large_sym', 'compact', 'pair', 'wide')


def _run(entry, A, ns, M, K, row_cap=None):
  """A [B, N, N] float32 numpy (N % 4 == 0), ns [B] or None (a full tile).
  -> D [B, K], V [B, N, K], info [B], fallback flags [B] or None, all numpy."""
  from lanczosnet_amd import ops
  Ad = torch.from_numpy(np.ascontiguousarray(A)).to(DEV)
  nd = torch.from_numpy(np.asarray(ns, np.int32)).to(DEV) if ns is not None else None
  B, N, _ = A.shape
  fb = None
  if entry in ('large', 'large_sym'):
    sym = entry == 'large_sym'
    if nd is None:
      D, V, info = ops.lanczos_ritz_large(Ad, M, K, return_info=True, symmetric=sym)
    else:
      D, V, info = ops.lanczos_ritz_kstep(Ad, nd, M, K, symmetric=sym, compact=False, return_info=True)
    assert ops.last_kernel() == 'lanczos_ritz_large_kernel<%d>' % (1 if sym else 0)
  elif entry in ('compact', 'pair'):
    if entry == 'pair':
      Ad = torch.stack([Ad, Ad * 0.5], dim=3)[..., 0]
      assert Ad.stride(2) == 2
    D, V, info, fb = ops.lanczos_ritz_kstep(Ad, nd, M, K, compact=True, row_cap=row_cap, return_info=True,
                                            return_fallback=True)
    assert 'lanczos_ritz_large_kernel<2>' in ops.last_kernel()
  else:
    cap = int(row_cap if row_cap is not None else ops.kstep_row_cap(N))
    need = ops._abi().lanczos_ritz_kstep_wide_workspace_bytes(B, N, M, cap)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    D = torch.empty((B, K), dtype=torch.float32, device=DEV)
    V = torch.empty((B, N, K), dtype=torch.float32, device=DEV)
    info = torch.empty((B,), dtype=torch.int32, device=DEV)
    fb = torch.empty((B,), dtype=torch.int32, device=DEV)
    ops._abi().lanczos_ritz_kstep_wide(Ad, Ad.stride(0), Ad.stride(1), Ad.stride(2), nd, B, N, M, K, cap, ws, need,
                                       D, V, info, fb)
    assert 'wide' in ops.last_kernel()
  return D.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy(), (fb.cpu().numpy() if fb is not None else None)


# ---- (a) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('entry', ENTRIES)
def test_full_krylov_space_against_float64_eigh(entry, which):
  """A tile of 64 run for 64 steps: a graph of n nodes stops after n steps and the Ritz pairs are the
  eigenpairs — check_bars against eigh, every graph, nothing skipped."""
  tag, A, ns, names, ks = kc.full_batches()[which]
  worst = np.zeros(4)
  for K in ks:
    D, V, info, _ = _run(entry, A, ns, kc.N_FULL, K)
    assert info.tolist() == ns.tolist(), (tag, K, info.tolist())
    worst = np.maximum(worst, rc.check_bars(A, ns, K, D, V, rc.eigh_ref(A, ns, K), names))
  print('%s %s: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  projector %.2e' % ((entry, tag) + tuple(worst)))


# ---- (b) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
def test_multiplicities_each_distinct_eigenvalue_once(entry):
  A, ns, names = kc.multiplicity_batch()
  D, V, info, _ = _run(entry, A, ns, 24, 24)
  for b, name in enumerate(names):
    fig = kc.check_distinct(name, A[b, :ns[b], :ns[b]], D[b], V[b], info[b], 24)
    print('%s %s: steps %d  |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e' % ((entry, name, info[b]) + fig))


# ---- (c) ---------------------------------------------------------------------------------------
def _check_batch(entry, A, ns, names, M, K, out, worst):
  D, V, info, _ = out
  for b in range(A.shape[0]):
    n = int(ns[b]) if ns is not None else A.shape[1]
    fig = kc.check_restatement('%s %s' % (entry, names[b]), A[b, :n, :n], M, K, D[b], V[b], info[b])
    worst[:] = np.maximum(worst, fig)


@pytest.mark.parametrize('N', kc.SEAM_N)
@pytest.mark.parametrize('entry', ENTRIES)
def test_kstep_seams_against_the_restatement(entry, N):
  """The L4 and the L1 of one connected graph per tile width, a full tile, every (M, K)."""
  A = kc.seam_graphs(N)
  worst = np.zeros(3)
  for M, K in kc.seam_shapes(N):
    _check_batch(entry, A, None, ('N%d_L4' % N, 'N%d_L1' % N), M, K, _run(entry, A, None, M, K), worst)
  print('%s N=%d: |D-Dref| %.2e  projector %.2e  |VtV-I| %.2e' % ((entry, N) + tuple(worst)))


@pytest.mark.parametrize('M', kc.OPERATOR_M)
@pytest.mark.parametrize('entry', ENTRIES)
def test_l1_and_l2_operators_against_the_restatement(entry, M):
  """L2 and L1 of G(128, 0.1) and G(256, 0.05): a single Gram-Schmidt pass compounds here."""
  cases = kc.operator_cases()
  worst = np.zeros(3)
  for n in (128, 256):
    cs = [c for c in cases if c[1].shape[0] == n]
    A, _ = rc.pad_batch(cs, n)
    _check_batch(entry, A, None, [c[0] for c in cs], M, M, _run(entry, A, None, M, M), worst)
  print('%s M=%d: |D-Dref| %.2e  projector %.2e  |VtV-I| %.2e' % ((entry, M) + tuple(worst)))


@pytest.mark.parametrize('entry', ENTRIES)
def test_ragged_tile(entry):
  A, ns, names = kc.ragged_batch()
  worst = np.zeros(3)
  out = _run(entry, A, ns, 64, 64)
  assert out[2].tolist() == [64, 64, 64, 3, 0]
  _check_batch(entry, A, ns, names, 64, 64, out, worst)
  print('%s ragged: |D-Dref| %.2e  projector %.2e  |VtV-I| %.2e' % ((entry,) + tuple(worst)))


@pytest.mark.parametrize('M', (65, 100))
def test_wide_kernel_through_ops_beyond_64_steps(M):
  """M > 64 on a 260-node tile: no other kernel serves it, ops routes it to the wide one."""
  from lanczosnet_amd import ops
  A, ns, names = kc.ragged_batch()
  D, V, info = ops.lanczos_ritz_kstep(torch.from_numpy(A).to(DEV), torch.from_numpy(ns).to(DEV), M, M, return_info=True)
  assert 'wide' in ops.last_kernel()
  assert info.cpu().tolist() == [M, M, M, 3, 0]
  worst = np.zeros(3)
  _check_batch('ops', A, ns, names, M, M, (D.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy(), None), worst)
  print('wide through ops M=%d: |D-Dref| %.2e  projector %.2e  |VtV-I| %.2e' % ((M,) + tuple(worst)))


@pytest.mark.parametrize('entry', ENTRIES)
def test_row_capacity_and_the_dense_fallback(entry):
  """A row of exactly row_cap entries stays on the image; row_cap + 1 raises the graph's flag and the
  graph is multiplied from its dense rows in the same call."""
  A, ns, _ = kc.row_cap_batch()
  out = _run(entry, A, ns, 16, 16, row_cap=kc.ROW_CAP)
  if out[3] is not None:
    assert out[3].tolist() == [0, 1]
  worst = np.zeros(3)
  _check_batch(entry, A, ns, ('hub_at_cap', 'hub_beyond_cap'), 16, 16, out, worst)
  print('%s row_cap: |D-Dref| %.2e  projector %.2e  |VtV-I| %.2e' % ((entry,) + tuple(worst)))


# ---- invariants -----------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
def test_same_bits_alone_in_a_batch_and_again(entry):
  A, ns, _ = kc.ragged_batch()
  big, bns = np.tile(A, (60, 1, 1)), np.tile(ns, 60)        # 300 graphs; graph 150 is the 260-node one
  assert big.shape[0] == 300 and bns[150] == kc.RAGGED_N
  D, V, info, _ = _run(entry, big, bns, 64, 17)
  D1, V1, info1, _ = _run(entry, big[150:151], bns[150:151], 64, 17)
  assert np.array_equal(D[150], D1[0]) and np.array_equal(V[150], V1[0]) and info[150] == info1[0]
  for b in range(5, 300, 5):                                  # every copy of the tile: the same bits
    assert np.array_equal(D[b:b + 5], D[:5]) and np.array_equal(V[b:b + 5], V[:5])
    assert np.array_equal(info[b:b + 5], info[:5])
  D2, V2, info2, _ = _run(entry, big, bns, 64, 17)
  assert np.array_equal(D, D2) and np.array_equal(V, V2) and np.array_equal(info, info2)


# ---- (d) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', kc.BIG_SCALES)
@pytest.mark.parametrize('entry', ENTRIES)
def test_power_of_two_scaling_changes_nothing_but_the_scale(entry, s):
  for tag, A, ns in kc.scale_base():
    M = 64 if tag == 'full64' else 24
    D0, V0, info0, _ = _run(entry, A, ns, M, M)
    assert info0.tolist() == (ns.tolist() if tag == 'full64' else [8])
    D1, V1, info1, _ = _run(entry, (A * np.float32(s)).astype(np.float32), ns, M, M)
    assert np.array_equal(info1, info0), (entry, tag, s, info1.tolist())
    assert np.array_equal(V1, V0) and np.array_equal(D1, D0 * np.float32(s)), (entry, tag, s)


# ---- refusals --------------------------------------------------------------------------------------
def _raw_call(entry, N, M, K, row_cap=64, alloc_n=None):
  """One raw C entry on a zero batch of one graph (nothing is read: the launcher refuses first)."""
  from lanczosnet_amd import ops
  abi = ops._abi()
  A = torch.zeros((1, N, N), dtype=torch.float32, device=DEV)
  D = torch.empty((1, max(K, 1)), dtype=torch.float32, device=DEV)
  V = torch.empty((1, N, max(K, 1)), dtype=torch.float32, device=DEV)
  ws = torch.empty((1 << 24,), dtype=torch.uint8, device=DEV)
  s = (A.stride(0), A.stride(1))
  if entry == 'large':
    return abi.lanczos_ritz_large(A, s[0], s[1], 1, N, M, K, ws, D, V, None)
  if entry == 'large_sym':
    return abi.lanczos_ritz_large_sym(A, s[0], s[1], 1, N, M, K, ws, D, V, None)
  if entry in ('kstep', 'kstep_compact'):
    flags = 3 if entry == 'kstep_compact' else 1
    return abi.lanczos_ritz_kstep(A, s[0], s[1], 1, None, 1, N, M, K, flags, row_cap if flags & 2 else 0, ws,
                                  ws.numel(), D, V, None, None)
  return abi.lanczos_ritz_kstep_wide(A, s[0], s[1], 1, None, 1, N, M, K, row_cap, ws, ws.numel(), D, V, None, None)


RAW = ('large', 'large_sym', 'kstep', 'kstep_compact', 'wide')


@pytest.mark.parametrize('entry', RAW)
def test_entries_refuse_what_they_cannot_serve(entry):
  from lanczosnet_amd import _lib
  for N, M, K in ((16, 17, 4), (16, 8, 9), (62, 8, 8)):          # M > N, K > M, N % 4 != 0
    with pytest.raises(_lib.LnzError):
      _raw_call(entry, N, M, K)
  _raw_call(entry, 16, 8, 8)                                      # (the same call within the envelope runs)
  torch.cuda.synchronize()
  if entry != 'wide':                                             # one workgroup holds 2048 nodes
    with pytest.raises(_lib.NotSupported):
      _raw_call(entry, 2052, 64, 64)
  if entry in ('kstep_compact', 'wide'):
    with pytest.raises(_lib.LnzError):
      _raw_call(entry, 64, 16, 16, row_cap=12)


def test_ops_refuses_more_steps_than_nodes_and_more_pairs_than_steps():
  from lanczosnet_amd import _lib, ops
  A = torch.zeros((1, 16, 16), dtype=torch.float32, device=DEV)
  for M, K in ((17, 4), (8, 9)):
    with pytest.raises(_lib.LnzError):
      ops.lanczos_ritz_kstep(A, None, M, K)
    with pytest.raises(_lib.LnzError):
      ops.lanczos_ritz_large(A, M, K)
