"""The full-length Ritz kernels at their edges and beyond molecule spectra: the one-wavefront
kernel (csrc/lanczos_ritz.hip, N <= 32) at every store path, tile size and n_nodes clamp, through
its QL fallback and on matrices that are no L4 Laplacian; the workgroup kernel
(csrc/lanczos_ritz_wg.hip, 33..192 nodes) on evenly spread and graded spectra; the fused
preparation launches at K = N = 32 and K = 3.

Reference: np.linalg.eigh of the float32 matrix in float64 + the |lambda| mergesort
(ritz_cases.eigh_ref).  Bars, relative to max |lambda| of the case (ritz_cases.check_bars):
|D - D_ref| < 1e-6, |V^T V - I| < 2e-6, |A V - V D| < 2e-6, spectral projectors of powers 1, 5, 30
within 1e-5.  K = n wherever a family has ties, so no case is skipped for a degenerate cut.

The `spread` cases and the L1 operators are what the rule of the second Gram-Schmidt pass was
changed for (lnz::CgsBound, csrc/wave.hpp): with the 99 % rule alone the kernels
returned |V^T V - I| = 0.11 for L1 of G(32, 0.3), 1.2e-3 for spread(40) and Ritz values off by
14 |A| and more from n = 64 on, all with info = 0."""
import functools

import numpy as np
import pytest
import torch

import oracle
import ritz_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ritz(A, ns, K, kernel='auto'):
  from lanczosnet_amd import ops
  D, V, info = ops.lanczos_ritz(_t(A), _t(ns), K, return_info=True, kernel=kernel)
  return D.cpu().numpy(), V.cpu().numpy(), info.cpu().numpy()


# ------------------------------------------------------------------------- the wavefront kernel
SHAPES, _shape_batch = rc.SHAPES, rc.shape_batch


@pytest.mark.parametrize('N,K', SHAPES)
def test_wavefront_kernel_at_every_tile_size_and_store_path(N, K):
  A, ns, names = _shape_batch(N)
  D, V, info = _ritz(A, ns, K)
  assert D.shape == (len(ns), K) and V.shape == (len(ns), N, K)
  rc.check_bars(A, ns, K, D, V, rc.eigh_ref(A, ns, K), names, say=print)
  assert (info >= 0).all()


@pytest.mark.parametrize('N,K', [(31, 20), (17, 65)])
def test_raw_abi_entry_writes_every_element(N, K):
  """lnz_lanczos_ritz on D, V, info full of NaN / -1: every element is written (zeros beyond the
  live block included), and the bits are those of the torch entry."""
  from lanczosnet_amd import ops
  A, ns, names = _shape_batch(N)
  B = len(ns)
  At, nt = _t(A), _t(ns)
  D = torch.full((B, K), float('nan'), dtype=torch.float32, device=DEV)
  V = torch.full((B, N, K), float('nan'), dtype=torch.float32, device=DEV)
  info = torch.full((B,), -1, dtype=torch.int32, device=DEV)
  sb, sr, sc = At.stride()
  with torch.cuda.device(At.device):
    ops._abi().lanczos_ritz(At, sb, sr, sc, nt, B, N, K, D, V, info)
  torch.cuda.synchronize()
  assert torch.isfinite(D).all() and torch.isfinite(V).all() and (info >= 0).all()
  D2, V2, info2 = ops.lanczos_ritz(At, nt, K, return_info=True)
  assert torch.equal(D, D2) and torch.equal(V, V2) and torch.equal(info, info2)
  rc.check_bars(A, ns, K, D.cpu().numpy(), V.cpu().numpy(), rc.eigh_ref(A, ns, K), names)


@pytest.mark.parametrize('N,K', [(17, 20), (32, 32)])
def test_n_nodes_is_clamped_to_the_tile(N, K):
  """n_nodes = -3 behaves as 0 and N + 5 as N, bit for bit."""
  A = np.stack([rc.random_symmetric(N, 77 + i) for i in range(4)])
  wild = np.array([-3, N + 5, N, 0], np.int32)
  tame = np.array([0, N, N, 0], np.int32)
  Dw, Vw, iw = _ritz(A, wild, K)
  Dt, Vt, it = _ritz(A, tame, K)
  np.testing.assert_array_equal(Dw, Dt)
  np.testing.assert_array_equal(Vw, Vt)
  np.testing.assert_array_equal(iw, it)
  assert (Dw[0] == 0).all() and (Vw[0] == 0).all()
  rc.check_bars(A, tame, K, Dw, Vw, rc.eigh_ref(A, tame, K))


@functools.lru_cache(maxsize=None)
def _spectra_batch():
  cases = [c for n in (24, 31, 32) for c in rc.spread(n) + rc.graded(n) + rc.paired(n)]
  A, ns = rc.pad_batch(cases, 32)
  return A, ns, [c[0] for c in cases], rc.eigh_ref(A, ns, 32)


def test_wavefront_kernel_on_spread_graded_and_paired_spectra():
  """Evenly spread, graded over six decades, and +-lambda pairs, n = 24, 31, 32 in the 32 tile,
  K = 32 (nothing cut).  Two calls give the same bits."""
  A, ns, names, ref = _spectra_batch()
  D, V, info = _ritz(A, ns, 32)
  rc.check_bars(A, ns, 32, D, V, ref, names, say=print)
  D2, V2, info2 = _ritz(A, ns, 32)
  np.testing.assert_array_equal(D, D2)
  np.testing.assert_array_equal(V, V2)
  np.testing.assert_array_equal(info, info2)


def test_wavefront_kernel_on_operators_that_are_no_l4_laplacian():
  """Raw adjacency, L1 = D - A (norm up to twice the largest degree) and L2 of a path, a ring, a
  star and a G(32, 0.3); K = 32 (the ring's and the star's spectra are full of ties).  A
  channels-last view gives the bits of the contiguous copy."""
  from lanczosnet_amd import ops
  cases = rc.non_l4_operators()
  A, ns = rc.pad_batch(cases, 32)
  names = [c[0] for c in cases]
  D, V, info = _ritz(A, ns, 32)
  rc.check_bars(A, ns, 32, D, V, rc.eigh_ref(A, ns, 32), names, say=print)
  L = torch.zeros((len(ns), 32, 32, 2), dtype=torch.float32, device=DEV)
  L[..., 0] = _t(A)
  L[..., 1] = 7.0   # (never read)
  view = L[..., 0]
  assert not view.is_contiguous()
  Dv, Vv = ops.lanczos_ritz(view, _t(ns), 32)
  np.testing.assert_array_equal(Dv.cpu().numpy(), D)
  np.testing.assert_array_equal(Vv.cpu().numpy(), V)


@functools.lru_cache(maxsize=None)
def _molecule_cases():
  from lanczosnet_amd.synthetic import draw_batch
  b = draw_batch(8, seed=3, n_min=4, n_max=26)
  out = []
  for i in range(8):
    n = int(b['n_nodes'][i])
    out.append(('mol%d' % i, oracle.laplacian_l4(b['adjs'][i, :n, :n].sum(axis=2)).astype(np.float32)))
  return out


@pytest.mark.parametrize('s', rc.SCALES)
def test_wavefront_kernel_is_scale_free(s):
  """A molecule batch and spread(32) times 2^-20 .. 2^20: D / s and V meet the same relative bars
  (the breakdown tolerance is relative to the matrix)."""
  for cases in (_molecule_cases(), rc.spread(32)):
    cases = rc.scaled(cases, s)
    A, ns = rc.pad_batch(cases)
    K = A.shape[1]
    D, V, info = _ritz(A, ns, K)
    rc.check_bars(A, ns, K, D, V, rc.eigh_ref(A, ns, K), [c[0] for c in cases], say=print)


def test_wavefront_kernel_ql_fallback_on_wilkinson_matrices():
  """W+_{2m+1}, m = 8, 9, 10, 12, 13, 14, plain, / 16, - 3 I, negated and permuted, in one batch:
  the largest eigenvalues agree pairwise to ~1e-14 with no weak coupling between the copies, the
  twist windows cannot separate them and the kernel takes its implicit-QL sweep (info >= 256).
  Every member meets the bars whichever solver ran; the members whose Lanczos matrix the mirror
  sends to the sweep (test_ritz_cases_cpu.py pins them: the first four forms) take it here too."""
  cases = rc.wilkinson_family()
  A, ns = rc.pad_batch(cases, 32)
  names = [c[0] for c in cases]
  D, V, info = _ritz(A, ns, 32)
  took = [nm for nm, i in zip(names, info) if i >= 256]
  print('QL fallback on %d of %d: %s' % (len(took), len(names), took))
  rc.check_bars(A, ns, 32, D, V, rc.eigh_ref(A, ns, 32), names, say=print)
  pinned = [nm for nm in names if not nm.endswith('_permuted')]
  assert len(pinned) == 24
  missing = [nm for nm in pinned if nm not in took]
  assert not missing, missing


# ------------------------------------------------------------------------- the workgroup kernel
WG_KERNELS = ('auto', 'workgroup_ws', 'workgroup_mw', 'workgroup_p1', 'workgroup_p2', 'workgroup_p4', 'workgroup_ql')


@pytest.mark.parametrize('n', [40, 64, 100, 128, 160])
def test_workgroup_kernel_on_spread_and_graded_spectra(n):
  """spread(n) (rotated and diagonal) and graded(n): the wave-level Lanczos phase up to 128 nodes,
  the eight-wave form at 160, every placement and split, and the QL sweep, K = n.  The eight-wave
  form with the basis in LDS and in the workspace stays bit-identical — compared at K = 24, where
  both placements have room for the parallel eigensolver's vectors (at K = n = 100 the LDS
  placement has not and takes the QL sweep: the same T, other last bits in V)."""
  cases = rc.spread(n) + rc.graded(n)
  A, ns = rc.pad_batch(cases, n)
  names = [c[0] for c in cases]
  ref = rc.eigh_ref(A, ns, n)
  for kern in WG_KERNELS:
    D, V, info = _ritz(A, ns, n, kernel=kern)
    rc.check_bars(A, ns, n, D, V, ref, ['%s %s' % (kern, nm) for nm in names], say=print)
    assert kern != 'workgroup_ql' or (info >= 256).all()
  ref24 = rc.eigh_ref(A, ns, 24)
  Dw, Vw, iw = _ritz(A, ns, 24, kernel='workgroup_ws')
  Dm, Vm, im = _ritz(A, ns, 24, kernel='workgroup_mw')
  rc.check_bars(A, ns, 24, Dw, Vw, ref24, ['workgroup_ws K=24 ' + nm for nm in names], say=print)
  np.testing.assert_array_equal(iw, im)   # (the same eigensolver ran)
  np.testing.assert_array_equal(Dw, Dm)
  np.testing.assert_array_equal(Vw, Vm)


# ---------------------------------------------------------------------------- the fused launches
@pytest.mark.parametrize('N,K,B,seed', [(32, 32, 40, 34), (5, 3, 9, 5)])
def test_fused_preparation_launches_return_the_standalone_bits(N, K, B, seed):
  """lnz_prepare_batch and lnz_prepare_batch_prev_gains run the wavefront kernel's body: D and V
  equal lnz_lanczos_ritz bit for bit at K = N = 32 (n up to 32) and at N = 5, K = 3."""
  from lanczosnet_amd import ops
  from lanczosnet_amd.model import LanczosNet
  from lanczosnet_amd.synthetic import draw_batch
  from lanczosnet_amd.utils.arg_helper import make_model_config
  cfg = dict(oracle.DEFAULT_QM8_CFG)
  net = LanczosNet(make_model_config(cfg)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_lanczosnet_params(cfg, 5).items()})
  plan = net.to(DEV)._plan()
  batch = draw_batch(B, seed=seed, n_min=1, n_max=N, N=N, num_bond_type=4)   # (5 channels: both launches' staging tile)
  assert int(batch['n_nodes'].max()) == N and int(batch['n_nodes'].min()) == 1
  n = _t(batch['n_nodes'])
  L = ops.laplacian_l4(_t(batch['adjs']), n)
  mask = _t(batch['node_mask']).contiguous()
  D1, V1 = ops.lanczos_ritz(L[:, :, :, 0], n, K)
  Lp2, tiles2, rows2, D2, V2 = ops.prepare_batch(plan, L, mask, n, K)
  assert torch.equal(D1, D2) and torch.equal(V1, V2)
  gains = (cfg['long_diffusion_dist'], cfg['num_layer'], plan['mlp_pack'])
  Lp3, tiles3, rows3, D3, V3, G3 = ops.prepare_batch_prev_gains(plan, L, mask, n, K, prev=(D2, rows2), gains=gains)
  torch.cuda.synchronize()
  assert torch.equal(D1, D3) and torch.equal(V1, V3) and torch.equal(Lp2, Lp3)
  A = L[:, :, :, 0].cpu().numpy()
  ns = batch['n_nodes']
  kk = np.minimum(ns, K)
  Dn, Vn = D1.cpu().numpy(), V1.cpu().numpy()
  for b in range(B):
    assert (Dn[b, kk[b]:] == 0).all() and (Vn[b, ns[b]:] == 0).all() and (Vn[b, :, kk[b]:] == 0).all()
    Vb = Vn[b, :ns[b], :kk[b]].astype(np.float64)
    assert np.abs(Vb.T @ Vb - np.eye(kk[b])).max() < rc.TOL_ORTH
    assert np.abs(A[b, :ns[b], :ns[b]].astype(np.float64) @ Vb - Vb * Dn[b, :kk[b]]).max() < rc.TOL_RES
