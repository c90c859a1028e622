"""GPU checks of the wide K-step path (lnz_lanczos_ritz_kstep_wide, csrc/lanczos_wide.hip): graphs of
2049 .. 16384 nodes and 65 .. 256 Lanczos steps, M > K included, against the fp64 restatement
(oracle/lanczos_kstep.py) at the bars of test_large_lanczos_matches_fp64_restatement; the seam to the
one-workgroup entry; the product surface on top."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

from large_fixture import adjacency, general_inputs, graphs as _graphs, kstep_ritz  # noqa: E402


def _check_against_restatement(tag, D, V, A, M, K, info=None, want_steps=None):
  """The five bars for one graph: D [K], V [n, K] (device, as numpy) against the restatement of A [n, n]."""
  Dr, Vr, (_, _, steps, _) = oracle.lanczos_kstep_fp64(A, M, K)
  V = V.astype(np.float64)
  kk = min(K, steps)
  A64 = A.astype(np.float64)
  eD = np.abs(D - Dr).max()
  eP = np.abs(V @ V.T - Vr @ Vr.T).max()
  eO = np.abs(V[:, :kk].T @ V[:, :kk] - np.eye(kk)).max() if kk else 0.0
  res = np.linalg.norm(A64 @ V - V * D.astype(np.float64), axis=0)
  res_ref = np.linalg.norm(A64 @ Vr - Vr * Dr, axis=0)
  eR = np.abs(res - res_ref).max()
  print('%s: |D - D_ref| %.2e  projector %.2e  |V^T V - I| %.2e  residual gap %.2e  steps %s (restatement %d)'
        % (tag, eD, eP, eO, eR, info, steps))
  assert eD < 1e-6
  assert eP < 1e-5
  assert eO < 1e-5
  assert eR < 1e-4
  if info is not None:
    assert int(info) == (steps if want_steps is None else want_steps)
  return Dr, Vr, steps


def _projector_gap(Va, Vb):
  Pa = Va.double() @ Va.double().transpose(1, 2)
  Pb = Vb.double() @ Vb.double().transpose(1, 2)
  return float((Pa - Pb).abs().max())


# (the first four shapes: |theta| gap at the K cut 6e-3 for (2560, 96, 48) and 5e-4 for (4096, 128, 64),
#  checked on the CPU with 1-ulp noise on every A q — well conditioned; none had to change its seed)
@pytest.mark.parametrize('N,M,K,B', [(2560, 96, 96, 2), (2560, 96, 48, 2), (4096, 128, 64, 2), (4096, 160, 160, 1),
                                     (2048, 128, 64, 2), (1000, 100, 100, 2), (8192, 64, 64, 1)])
def test_wide_kstep_matches_fp64_restatement(N, M, K, B):
  from lanczosnet_amd import ops
  A = _graphs(B, N, 8.0 / N, seed=N)
  D, V, info = ops.lanczos_ritz_kstep(torch.from_numpy(A).to(DEV), None, M, K, return_info=True)
  assert D.shape == (B, K) and V.shape == (B, N, K)
  assert 'wide' in ops.last_kernel()
  D, V, info = D.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy()
  for b in range(B):
    _check_against_restatement('N %d M %d K %d graph %d' % (N, M, K, b), D[b], V[b], A[b], M, K, info[b], M)


def _direct(entry, A, M, K, n_nodes=None):
  """A call of a C entry through the ctypes binding on the current stream (contiguous A)."""
  from lanczosnet_amd import _lib, ops
  lib = _lib.load()
  B, N, _ = A.shape
  cap = ops.kstep_row_cap(N)
  D = torch.empty((B, K), dtype=torch.float32, device=A.device)
  V = torch.empty((B, N, K), dtype=torch.float32, device=A.device)
  info = torch.empty((B,), dtype=torch.int32, device=A.device)
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  nn = C.c_void_p(n_nodes.data_ptr()) if n_nodes is not None else C.c_void_p(None)
  p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
  if entry == 'kstep':
    need = lib.lnz_lanczos_ritz_kstep_workspace_bytes(B, N, 3, cap)
    ws = torch.empty((need,), dtype=torch.uint8, device=A.device)
    rc = lib.lnz_lanczos_ritz_kstep(p(A), A.stride(0), A.stride(1), 1, nn, B, N, M, K, 3, cap, p(ws), need, p(D), p(V),
                                    p(info), C.c_void_p(None), st)
  else:
    need = lib.lnz_lanczos_ritz_kstep_wide_workspace_bytes(B, N, M, cap)
    ws = torch.empty((need,), dtype=torch.uint8, device=A.device)
    rc = lib.lnz_lanczos_ritz_kstep_wide(p(A), A.stride(0), A.stride(1), 1, nn, B, N, M, K, cap, p(ws), need, p(D),
                                         p(V), p(info), C.c_void_p(None), st)
  _lib.check(rc)
  torch.cuda.synchronize()
  return D, V, info


@pytest.mark.parametrize('N,M', [(2048, 64), (1412, 40)])
def test_route_up_to_2048_nodes_and_64_steps_is_untouched(N, M):
  """ops.lanczos_ritz_kstep inside the one-workgroup envelope: bitwise the existing C entry."""
  from lanczosnet_amd import ops
  A = torch.from_numpy(_graphs(2, N, 8.0 / N, seed=N)).to(DEV)
  ops.forget_autograd_kernel()
  D, V = ops.lanczos_ritz_kstep(A, None, M, M)
  assert 'lanczos_ritz_large_kernel' in ops.last_kernel() and 'wide' not in ops.last_kernel()
  D0, V0, _ = _direct('kstep', A, M, M)
  assert torch.equal(D, D0) and torch.equal(V, V0)


def test_new_entry_agrees_with_the_existing_one_at_the_seam():
  N, M = 2048, 64
  A = torch.from_numpy(_graphs(2, N, 8.0 / N, seed=N)).to(DEV)
  D0, V0, i0 = _direct('kstep', A, M, M)
  D1, V1, i1 = _direct('wide', A, M, M)
  print('seam: |D| %.2e projector %.2e' % (float((D0 - D1).abs().max()), _projector_gap(V0, V1)))
  assert torch.equal(i0, i1)
  assert (D0 - D1).abs().max() < 1e-6
  assert _projector_gap(V0, V1) < 1e-5


def test_ragged_batch_and_unaligned_width():
  from lanczosnet_amd import ops
  N, K = 3001, 32
  sizes = [3001, 2100, 0, 2100]
  A = np.zeros((4, N, N), np.float32)
  A[0] = _graphs(1, 3001, 8.0 / 3001, seed=61)[0]
  A[1, :2100, :2100] = _graphs(1, 2100, 8.0 / 2100, seed=62)[0]
  A[3] = A[1]
  nn = torch.tensor(sizes, dtype=torch.int32, device=DEV)
  Ad = torch.from_numpy(A).to(DEV)
  D, V, info = ops.lanczos_ritz_kstep(Ad, nn, K, K, return_info=True)
  assert V.shape == (4, N, K)
  Dn, Vn = D.cpu().numpy(), V.cpu().numpy()
  for b, n in enumerate(sizes):
    if n == 0:
      assert int(info[b]) == 0 and (Dn[b] == 0).all() and (Vn[b] == 0).all()
      continue
    _, _, kk = _check_against_restatement('ragged graph %d (n = %d)' % (b, n), Dn[b], Vn[b, :n], A[b, :n, :n], K, K,
                                          info[b])
    assert (Vn[b, n:] == 0).all() and (Vn[b, :, kk:] == 0).all() and (Dn[b, kk:] == 0).all()
  # a result depends neither on the position in the batch nor on the neighbours
  assert torch.equal(D[1], D[3]) and torch.equal(V[1], V[3])
  D1, V1 = ops.lanczos_ritz_kstep(Ad[1:2], nn[1:2], K, K)
  assert torch.equal(D1[0], D[1]) and torch.equal(V1[0], V[1])


def test_early_stop_on_invariant_subspace():
  from lanczosnet_amd import ops
  N, M = 2304, 16
  A = torch.eye(N, dtype=torch.float32, device=DEV)[None]
  D, V, info = ops.lanczos_ritz_kstep(A, None, M, M, return_info=True)
  assert int(info[0]) == 1
  D = D.cpu().numpy()[0]
  assert abs(D[0] - 1.0) < 1e-6 and (D[1:] == 0).all()
  assert (V.cpu().numpy()[0][:, 1:] == 0).all()


def test_dense_rows_are_multiplied_in_the_same_call():
  """A graph with a row beyond the image's capacity (row_cap = 8) is flagged — that graph only — and
  multiplied from its dense rows; both graphs meet the bars."""
  from lanczosnet_amd import ops
  N, M = 2304, 32
  A = np.zeros((2, N, N), np.float32)
  # graph 0: thinned until no row of its Laplacian (degree + the diagonal) has more than 8 entries
  adj = adjacency(1, N, 2.0 / N, 72)[0]
  while ((adj != 0).sum(axis=1) + 1).max() > 8:
    r = int(((adj != 0).sum(axis=1)).argmax())
    c = int(np.nonzero(adj[r])[0][0])
    adj[r, c] = adj[c, r] = 0
  A[0] = oracle.laplacian_l4(adj)
  hub = adjacency(1, N, 2.0 / N, 73)[0]
  hub[5, 10:200] = hub[10:200, 5] = 1.0
  A[1] = oracle.laplacian_l4(hub)
  Ad = torch.from_numpy(A).to(DEV)
  sync = []
  orig = torch.Tensor.any

  def spy(self, *a, **kw):
    sync.append(1)
    return orig(self, *a, **kw)
  torch.Tensor.any = spy
  try:
    D, V, info, fb = ops.lanczos_ritz_kstep(Ad, None, M, M, row_cap=8, return_info=True, return_fallback=True)
  finally:
    torch.Tensor.any = orig
  assert not sync                                   # contiguous input: nobody looked at the flags
  assert fb.cpu().tolist() == [0, 1]
  for b in range(2):
    _check_against_restatement('dense rows, graph %d' % b, D[b].cpu().numpy(), V[b].cpu().numpy(), A[b], M, M,
                               info[b], M)


def test_channel_0_of_the_collated_laplacian_in_place():
  import warnings
  from lanczosnet_amd import ops
  N, M, B = 2304, 32, 2
  A = _graphs(B, N, 8.0 / N, seed=5)
  Ad = torch.from_numpy(A).to(DEV)
  L = torch.stack([Ad, Ad * 0.5], dim=3)
  copies = []
  orig = torch.zeros

  def spy(*a, **kw):
    if len(a) and isinstance(a[0], tuple) and len(a[0]) == 3:
      copies.append(a[0])
    return orig(*a, **kw)
  torch.zeros = spy
  try:
    Dv, Vv, info, fb = ops.lanczos_ritz_kstep(L[..., 0], None, M, M, return_info=True, return_fallback=True)
    assert not copies and (fb == 0).all() and (info == M).all()
    Dc, Vc = ops.lanczos_ritz_kstep(Ad, None, M, M)
    assert not copies
  finally:
    torch.zeros = orig
  print('in place vs contiguous: |D| %.2e projector %.2e' % (float((Dv - Dc).abs().max()), _projector_gap(Vv, Vc)))
  assert (Dv - Dc).abs().max() < 1e-6 and _projector_gap(Vv, Vc) < 1e-5
  L2 = L.clone()
  L2[1, 7, :400, 0] = 0.01                                   # a row beyond the capacity (256 at this width)
  L2[1, :400, 7, 0] = 0.01
  Df, Vf, fbf = ops.lanczos_ritz_kstep(L2[..., 0], None, M, M, return_fallback=True)
  assert fbf.cpu().tolist() == [0, 1]
  Dd, Vd, fbd = ops.lanczos_ritz_kstep(L2[..., 0].contiguous(), None, M, M, return_fallback=True)
  assert fbd.cpu().tolist() == [0, 1]
  assert torch.equal(Df, Dd) and torch.equal(Vf, Vd)         # the copy took the dense form's path
  Le = torch.stack([Ad, Ad], dim=3)
  n = torch.full((B,), N, dtype=torch.int32, device=DEV)
  with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter('always')
    ops._WARNED.clear()
    De, Ve = ops.lanczos_ritz_collated(Le, n, M)
  assert any('use_eigen_decomp=False' in str(x.message) for x in w)
  assert torch.equal(De, Dv) and torch.equal(Ve, Vv)
  # the wide entry leaves no conv image behind: the module builds its own, as whenever none is attached
  assert ops.attached_sparse_image(Le) is None


def test_two_calls_give_the_same_bits():
  from lanczosnet_amd import ops
  N, M, K = 2560, 96, 48
  A = torch.from_numpy(_graphs(2, N, 8.0 / N, seed=N)).to(DEV)
  D0, V0 = ops.lanczos_ritz_kstep(A, None, M, K)
  D1, V1 = ops.lanczos_ritz_kstep(A, None, M, K)
  assert torch.equal(D0, D1) and torch.equal(V0, V1)


def test_product_surface_end_to_end_beyond_2048_nodes():
  """Raw adjacency -> collate_graph_adjacency -> LanczosNetGeneral at N = 2304, and the reference's
  use_eigen_decomp=False surface at k = 96 > 64."""
  import warnings
  from lanczosnet_amd.dataset.graph_data import collate_graph_adjacency
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  from lanczosnet_amd.utils.data_helper import get_graph_laplacian_eigs_batched
  B, N, K, seed = 2, 2304, 32, 9
  p_edge = 8.0 / N
  cfg, P, X, L, mask = general_inputs(B, N, K, 2, seed, p_edge)
  net = LanczosNetGeneral(make_model_config(cfg, general=True)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV)
  net.gemm_mode = 'fp32'
  adj = adjacency(B, N, p_edge, seed)
  items = [dict(adjs=adj[b][:, :, None].astype(np.float32), node_feat=X[b], label=np.zeros((1, 2)))
           for b in range(B)]
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    batch = collate_graph_adjacency(items, K, device=DEV)
  assert np.abs(batch['L'].cpu().numpy() - L).max() < 1e-7
  D, V = batch['D'].cpu().numpy(), batch['V'].cpu().numpy()
  Dr, Vr = kstep_ritz(L, K)
  for b in range(B):
    _check_against_restatement('collate graph %d' % b, D[b], V[b], L[b, :, :, 0], K, K)
    assert np.abs(D[b] - Dr[b]).max() < 1e-6
    Vg = V[b].astype(np.float64)
    assert np.abs(Vg @ Vg.T - Vr[b].astype(np.float64) @ Vr[b].astype(np.float64).T).max() < 1e-5
  with torch.no_grad():
    score = net(batch['node_feat'], batch['L'], batch['D'], batch['V'], mask=torch.from_numpy(mask).to(DEV))
  ref = oracle.lanczos_net_forward(P, cfg, X, L, D, V, mask, dtype=np.float64, general=True)
  err = np.abs(score.cpu().numpy() - ref).max() / np.abs(ref).max()
  print('N = 2304 forward on the device pairs vs oracle: rel err %.2e' % err)
  assert err < 1e-5
  k = 96
  n = torch.full((B,), N, dtype=torch.int32, device=DEV)
  D9, V9 = get_graph_laplacian_eigs_batched(batch['L'][..., 0], n, k, use_eigen_decomp=False)
  assert D9.shape == (B, k) and V9.shape == (B, N, k)
  for b in range(B):
    _check_against_restatement('eigs_batched k = 96 graph %d' % b, D9[b].cpu().numpy(), V9[b].cpu().numpy(),
                               L[b, :, :, 0], k, k)


def test_wider_krylov_space_converges_more_pairs():
  """M > K, the knob of the reference's eigsh call: on one G(2048, 0.01) graph at K = 64 the count of
  converged pairs (residual < 1e-6) is the restatement's at M = 64 and at M = 256, and grows."""
  from scipy.sparse.linalg import eigsh
  from lanczosnet_amd import ops
  N, K = 2048, 64
  A = _graphs(1, N, 0.01, seed=3)
  A64 = A[0].astype(np.float64)
  lam = np.linalg.eigvalsh(A64)
  Ad = torch.from_numpy(A).to(DEV)
  counts = {}
  for M in (64, 256):
    D, V = ops.lanczos_ritz_kstep(Ad, None, M, K)
    D, V = D.cpu().numpy()[0].astype(np.float64), V.cpu().numpy()[0].astype(np.float64)
    Dr, Vr, _ = oracle.lanczos_kstep_fp64(A[0], M, K)
    res = np.linalg.norm(A64 @ V - V * D, axis=0)
    res_ref = np.linalg.norm(A64 @ Vr - Vr * Dr, axis=0)
    band = (res_ref > 3e-7) & (res_ref < 3e-6)
    assert band.sum() <= 4            # (otherwise: another seed)
    conv = (res < 1e-6) & ~band
    conv_ref = (res_ref < 1e-6) & ~band
    near = np.abs(D[conv][:, None] - lam[None, :]).min(axis=1) if conv.any() else np.zeros(0)
    print('M = %d: converged device %d, restatement %d, in the band %d; largest converged residual %.2e, '
          'eigenvalue error %.2e' % (M, conv.sum(), conv_ref.sum(), band.sum(),
                                     res[conv].max() if conv.any() else 0.0, near.max() if near.size else 0.0))
    assert conv.sum() == conv_ref.sum()
    assert (near < 1e-6).all()
    e, _ = eigsh(A64, k=2, which='LM')
    lead = np.sort(np.abs(e))[::-1]
    assert conv[0] and abs(abs(D[0]) - lead[0]) < 1e-6
    counts[M] = int(conv.sum())
  assert counts[256] > counts[64]
