"""The spectral-gains kernels on their own (csrc/spectral_gains.hip, csrc/gains_body.hpp) against
the float64 oracle: one to sixteen long scales (the upper k-half of the first layer, lanes 32..63,
only carries data above eight), both MLP kernels by the launcher's own rule, every ragged tail, both
packers, live-row lists, the power branch and the fused preparation launch.

Bars: `rel_err` (max deviation over a layer's G / that layer's max |G|) < 1e-5, the project's
parity bar; the fp32 oracle against the fp64 oracle sits at 4e-7..7e-7 by that measure for every S
here.  (Per row it reaches 4.6e-5 at S = 1, a scalar output crossing zero: not used.)  The power
branch is held to one fp32 ulp of the float64 power; bit-identity everywhere two launches compute
the same rows."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err
from gains_tiles_worker import CASES, DIST16, compute, gains_cfg, mlp_layers, planted_eigenvalues
from lanczosnet_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, K, L, two-tile kernel by the launcher's rule ceil(R/32) * L >= 2048, what the shape is for)
SHAPES = [
    (3, 5, 1, False),      # R = 15 < 32: one part-filled tile
    (37, 27, 2, False),    # R = 999: one-tile kernel, ragged (R % 32 = 7)
    (1024, 20, 7, True),   # the bench shape, R % 64 = 0
    (293, 27, 16, True),   # R = 7911: R % 64 = 39 (second tile part-filled), sixteen layers
    (205, 20, 16, True),   # R = 4100: R % 64 = 4 (the last wave's second tile is wholly invalid)
]


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _two_tile(B, K, L):
  return (B * K + 31) // 32 * L >= 2048


def test_the_shapes_reach_both_kernels_and_every_tail():
  """the launch rule of lnz_spectral_gains_rows_split_to, restated: the table above is what it says"""
  for B, K, L, two in SHAPES:
    assert _two_tile(B, K, L) == two, (B, K, L)
  R = [B * K for B, K, L, two in SHAPES]
  assert R[0] < 32 and R[1] % 32 and R[2] % 64 == 0 and 32 < R[3] % 64 < 64 and 1 <= R[4] % 64 <= 32
  assert os.environ.get('LNZ_GAINS_TILES') is None   # (a forced kernel would void the table)


@pytest.mark.parametrize('B,K,L,two', SHAPES)
@pytest.mark.parametrize('S', [1, 2, 7, 8, 9, 12, 15, 16])
def test_mlp_gains_match_the_float64_oracle(S, B, K, L, two):
  """G of every layer against oracle.spectral_gains in float64.  The two small shapes go through the
  per-layer packer (pack_w0_kernel and friends), the others through the one-launch packer, so each
  packer's image of S > 8 faces the oracle, not only the other packer."""
  cfg = gains_cfg(S, L)
  P = oracle.make_lanczosnet_params(cfg, 1000 + 17 * S + L)
  layers = mlp_layers(P, L, DEV)
  if L <= 2:
    pack = torch.stack([ops.pack_spectral_mlp(lins, S) for lins in layers])
  else:
    pack = ops.pack_spectral_mlp_layers(layers, S)
  D = planted_eigenvalues(B, K, 7 * S + B)
  G = ops.spectral_gains(_t(D), DIST16[:S], L, pack).cpu().numpy()
  assert G.shape == (L, B, S, K) and np.isfinite(G).all()
  worst = 0.0
  for l in range(L):
    ref = oracle.spectral_gains(P, cfg, D, l, dtype=np.float64)   # B x K x S
    worst = max(worst, rel_err(G[l].transpose(0, 2, 1), ref))
  print('gains vs fp64: S=%d B=%d K=%d L=%d %s-tile kernel: rel_err %.3e'
        % (S, B, K, L, 'two' if two else 'one', worst))
  assert worst < 1e-5


def test_one_tile_and_two_tile_kernels_give_the_same_bits(tmp_path):
  """gains_body.hpp: "a row's arithmetic does not depend on RT".  One fresh child per forced kernel
  (LNZ_GAINS_TILES is read once per process); the files they write are bit-identical, and equal to
  what this process computes with the launcher's own choice (one-tile for the small cases, two-tile
  for the last)."""
  assert [_two_tile(B, K, L) for S, B, K, L in CASES] == [False, False, False, False, True]
  files = {}
  for tiles in ('1', '2'):
    files[tiles] = str(tmp_path / ('gains_tiles%s.f32' % tiles))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gains_tiles_worker.py'), files[tiles]],
                         cwd=ROOT, env=dict(os.environ, LNZ_GAINS_TILES=tiles), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert 'GAINS_TILES_OK tiles=%s' % tiles in out.stdout
  one, two = open(files['1'], 'rb').read(), open(files['2'], 'rb').read()
  want = sum(L * B * S * K for S, B, K, L in CASES) * 4
  assert len(one) == len(two) == want
  assert one == two
  assert compute(torch.device(DEV)).tobytes() == one


@pytest.mark.parametrize('B,K,L', [(37, 27, 2), (293, 27, 16)])
@pytest.mark.parametrize('S', [9, 16])
def test_live_row_lists_above_eight_scales(S, B, K, L):
  """lnz_plan_batch rows on a ragged batch (n from 1 to beyond K): bit-identical to the full
  computation on the slots k < min(n, K), exactly zero elsewhere (zero_fill), on the one-tile and
  on the two-tile kernel."""
  cfg = gains_cfg(S, L)
  P = oracle.make_lanczosnet_params(cfg, 77 + S)
  pack = ops.pack_spectral_mlp_layers(mlp_layers(P, L, DEV), S)
  rs = np.random.RandomState(B + S)
  n = rs.randint(1, 33, size=B).astype(np.int32)
  n[:4] = [1, K - 1, K, 32]
  mask = _t((np.arange(32)[None, :] < n[:, None]).astype(np.uint8))
  _, rows = ops.plan_batch(mask, True, K)
  live = np.minimum(n, K)
  assert int(rows[1].item()) == int(live.sum())
  D = _t(planted_eigenvalues(B, K, 5 + S))
  G_full = ops.spectral_gains(D, DIST16[:S], L, pack)
  G_rows = ops.spectral_gains(D, DIST16[:S], L, pack, rows=rows, zero_fill=True)
  sel = (torch.arange(K, device=DEV)[None, :] < _t(live)[:, None])[None, :, None, :].expand_as(G_full)
  assert torch.equal(G_rows[sel], G_full[sel])
  assert (G_rows[~sel] == 0).all()


def _no_subnormal_powers(D, dist, rs):
  """Redraw the entries of D of which some power is subnormal in fp32 (0 < |x| < 2^-126): whether
  the hardware flushes such a result is not what the power branch's test is about.  Powers that
  underflow to exact zero stay (1e-30 squared)."""
  tiny = np.float32(2.0 ** -126)
  for _ in range(64):
    ref = np.stack([np.power(D.astype(np.float64), p) for p in dist]).astype(np.float32)
    bad = ((ref != 0) & (np.abs(ref) < tiny)).any(axis=0)
    if not bad.any():
      return D
    D[bad] = rs.uniform(-1.0, 1.0, size=int(bad.sum())).astype(np.float32)
  raise AssertionError('redraw did not converge')


def test_power_branch_within_one_ulp_at_sixteen_scales():
  """mlp_pack=None: G[l][b][s][k] = D[b,k]^p_s for every layer, within one fp32 ulp of
  float32(np.power(float64(D), p)); exact zeros (0^p, 1e-30^p) are exact, signs of odd powers kept."""
  B, K, L = 37, 27, 2
  D = _no_subnormal_powers(planted_eigenvalues(B, K, 3), DIST16, np.random.RandomState(4))
  assert 0.0 in D and np.float32(1e-30) in D and np.float32(-1.0) in D
  ref = np.stack([np.power(D.astype(np.float64), p) for p in DIST16], axis=1).astype(np.float32)  # B,S,K
  assert not ((ref != 0) & (np.abs(ref) < np.float32(2.0 ** -126))).any()   # the condition on the inputs
  assert (ref == 0).sum() > 16            # 0^p and the underflowing powers of 1e-30 are in
  G = ops.spectral_gains(_t(D), DIST16, L, None).cpu().numpy()
  assert G.shape == (L, B, 16, K)
  ulp = np.where(ref == 0, np.float32(0), np.spacing(np.abs(ref)))
  worst = 0.0
  for l in range(L):
    dev = np.abs(G[l].astype(np.float64) - ref.astype(np.float64))
    assert (dev <= ulp).all(), (l, float((dev / np.maximum(ulp, 1e-45)).max()))
    nz = ref != 0
    worst = max(worst, float((dev[nz] / ulp[nz]).max()))
    assert np.array_equal(np.signbit(G[l][nz]), np.signbit(ref[nz]))
  print('power branch, S=16: worst deviation %.2f ulp (%d exact zeros)' % (worst, int((ref == 0).sum())))


@pytest.mark.parametrize('S', [1, 8, 9, 16])
def test_the_two_packers_give_the_same_gains(S):
  """lnz_pack_spectral_mlp per layer (stacked) and lnz_pack_spectral_mlp_layers: the same pack up to
  the prefetch slack, the same G bit for bit."""
  B, K, L = 37, 27, 3
  P = oracle.make_lanczosnet_params(gains_cfg(S, L), 500 + S)
  layers = mlp_layers(P, L, DEV)
  one = torch.stack([ops.pack_spectral_mlp(lins, S) for lins in layers])
  all_ = ops.pack_spectral_mlp_layers(layers, S)
  assert one.shape == all_.shape
  D = _t(planted_eigenvalues(B, K, 9 + S))
  assert torch.equal(ops.spectral_gains(D, DIST16[:S], L, one), ops.spectral_gains(D, DIST16[:S], L, all_))


@pytest.mark.parametrize('S', [0, 17])
def test_scale_counts_outside_one_to_sixteen_are_refused(S):
  """both packers and the gains entry point (either branch) raise; nothing is launched, and the
  stream is healthy afterwards."""
  dist = list(range(1, S + 1))
  rs = np.random.RandomState(S)
  lin = lambda o, i: (_t(rs.randn(o, i).astype(np.float32)), _t(rs.randn(o).astype(np.float32)))  # noqa: E731
  layers = [[lin(128, S), lin(128, 128), lin(128, 128), lin(S, 128)] for _ in range(2)]
  with pytest.raises(ops.LnzError):
    ops.pack_spectral_mlp(layers[0], S)
  with pytest.raises(ops.LnzError):
    ops.pack_spectral_mlp_layers(layers, S)
  D = _t(planted_eigenvalues(8, 20, 1))
  with pytest.raises(ops.NotSupported):
    ops.spectral_gains(D, dist, 2, None)
  P = oracle.make_lanczosnet_params(gains_cfg(16, 2), 1)
  pack16 = ops.pack_spectral_mlp_layers(mlp_layers(P, 2, DEV), 16)
  with pytest.raises(ops.NotSupported):
    ops.spectral_gains(D, dist, 2, pack16)
  torch.cuda.synchronize()
  assert ops.spectral_gains(D, DIST16, 2, pack16).isfinite().all()


@pytest.mark.parametrize('S', [9, 16])
def test_fused_preparation_launch_computes_the_gains_above_eight_scales(S):
  """lnz_prepare_batch_prev_gains at S > 8: the previous batch's gains out of the fused launch equal
  the standalone launch bit for bit on the live slots (the gains body is shared; its launch, row
  list and tail handling are not)."""
  from lanczosnet_amd.model import LanczosNet
  from lanczosnet_amd.synthetic import draw_batch
  from lanczosnet_amd.utils.arg_helper import make_model_config
  cfg = dict(oracle.DEFAULT_QM8_CFG, long_diffusion_dist=DIST16[:S], num_layer=3, hidden_dim=[128] * 3)
  net = LanczosNet(make_model_config(cfg)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_lanczosnet_params(cfg, 5).items()})
  net = net.to(DEV)
  plan = net._plan()
  gains = (DIST16[:S], 3, plan['mlp_pack'])
  ba, bb = draw_batch(200, seed=1, n_min=1, n_max=26), draw_batch(333, seed=2)
  prep = {}
  for key, b in (('a', ba), ('b', bb)):
    n = _t(b['n_nodes'])
    L = ops.laplacian_l4(_t(b['adjs']), n)
    mask = _t(b['node_mask']).contiguous()
    prep[key] = (L, mask, n) + tuple(ops.prepare_batch(plan, L, mask, n, 20))
  La, ma, na, Lpa, tla, rowsa, Da, Va = prep['a']
  Lb, mb, nb, Lpb, tlb, rowsb, Db, Vb = prep['b']
  Ga = ops.spectral_gains(Da, *gains, rows=rowsa)
  Lp2, tl2, rows2, D2, V2, G2 = ops.prepare_batch_prev_gains(plan, Lb, mb, nb, 20, prev=(Da, rowsa), gains=gains)
  assert torch.equal(Lp2, Lpb) and torch.equal(D2, Db) and torch.equal(V2, Vb)
  live = torch.clamp(na, max=20).long()
  sel = (torch.arange(20, device=DEV)[None, :] < live[:, None])[None, :, None, :].expand_as(Ga)
  assert tuple(G2.shape) == (3, 200, S, 20)
  assert torch.equal(Ga[sel], G2[sel])
  # and the standalone launch it is compared with is itself right
  Gref = oracle.spectral_gains({k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}, cfg,
                               Da.cpu().numpy(), 1, dtype=np.float64)
  G_full = ops.spectral_gains(Da, *gains).cpu().numpy()
  assert rel_err(G_full[1].transpose(0, 2, 1), Gref) < 1e-5
