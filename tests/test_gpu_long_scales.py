"""Nine to sixteen (and seventeen) long diffusion scales through the module on molecules of up to
32 nodes, against the float64 oracle fed the same Laplacians and Ritz pairs.

The fused kernels end at 12 long scales / 32 message channels (csrc/conv_strip.hip
strip_forward_eligible, csrc/conv_forward.hip launch_conv), the gains kernel at 16: up to there the
strip kernel must serve the call, beyond it the module must say so once and still give the
reference's result on the library path — the reference takes any `long_diffusion_dist`.

Bar: per-molecule `rel_err_rows` < 1e-5.  The fp32 oracle alone sits at 2e-7..1.1e-6 against the
fp64 oracle for S in {9, 12, 13, 16}, MLP and power filters, with and without short scales: a factor
of ten over the reference's own rounding.  Gradients: 2e-4 of max |g| per tensor, the tolerance of
test_hip_backward_short_channels_general_and_power_filters; the gain-gradient kernel at that
test's own 2e-6."""
import warnings

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err, rel_err_rows
from gains_tiles_worker import DIST16
from lanczosnet_amd.synthetic import draw_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _model(cfg, params):
  from lanczosnet_amd.model import LanczosNet
  from lanczosnet_amd.utils.arg_helper import make_model_config
  net = LanczosNet(make_model_config(cfg)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
  return net.to(DEV)


def _batch(B, seed, num_bond_type, **kw):
  """draw_batch's molecules; for more bond types than its six, every edge of the same graphs gets
  one of `num_bond_type` types (the channels still partition the edges)."""
  if num_bond_type <= 6:
    return draw_batch(B, seed=seed, num_bond_type=num_bond_type, **kw)
  b = draw_batch(B, seed=seed, **kw)
  simple = np.triu(b['adjs'].sum(axis=3), 1)                       # [B,N,N] 0/1
  rs = np.random.RandomState(1000 + seed)
  kind = rs.randint(num_bond_type, size=simple.shape)
  adjs = np.zeros(simple.shape + (num_bond_type,), np.float32)
  for e in range(num_bond_type):
    ae = simple * (kind == e)
    adjs[..., e] = ae + ae.transpose(0, 2, 1)
  assert np.array_equal(adjs.sum(axis=3), b['adjs'].sum(axis=3))
  return dict(b, adjs=adjs)


def _device_inputs(batch, K):
  from lanczosnet_amd import ops
  n = _t(batch['n_nodes'])
  L = ops.laplacian_l4(_t(batch['adjs']), n)
  D, V = ops.lanczos_ritz(L[:, :, :, 0], n, K)
  return L, D, V


# name, long scales, short scales, bond types, filter kind, gemm mode, route
FORWARD_CASES = [
    ('S9', 9, [], 6, 'MLP', 'fp32', 'strip'),
    ('S12', 12, [], 6, 'MLP', 'fp32', 'strip'),
    ('S12_f16x3', 12, [], 6, 'MLP', 'f16x3', 'strip'),
    ('S12_short3_bonds16_32ch', 12, [1, 2, 3], 16, 'MLP', 'fp32', 'strip'),
    ('S12_short3_bonds17_33ch', 12, [1, 2, 3], 17, 'MLP', 'fp32', 'library'),
    ('S13', 13, [], 6, 'MLP', 'fp32', 'library'),
    ('S16', 16, [], 6, 'MLP', 'fp32', 'library'),
    ('S16_pow', 16, [], 6, 'None', 'fp32', 'library'),
    ('S17', 17, [], 6, 'MLP', 'fp32', 'library'),
    ('S17_pow', 17, [], 6, 'None', 'fp32', 'library'),
]


@pytest.mark.parametrize('name,S,short,bonds,kind,gemm,route', FORWARD_CASES, ids=[c[0] for c in FORWARD_CASES])
def test_forward_nine_to_seventeen_long_scales(name, S, short, bonds, kind, gemm, route):
  from lanczosnet_amd import ops
  dist = DIST16[:S] if S <= 16 else DIST16 + [60]
  cfg = dict(oracle.DEFAULT_QM8_CFG, num_bond_type=bonds, short_diffusion_dist=short,
             long_diffusion_dist=dist, spectral_filter_kind=kind)
  assert len(short) + S + bonds + 1 == {'S12_short3_bonds16_32ch': 32, 'S12_short3_bonds17_33ch': 33}.get(
      name, S + 7)
  P = oracle.make_lanczosnet_params(cfg, 31 + S)
  net = _model(cfg, P)
  net.gemm_mode = gemm
  batch = _batch(96, 12, bonds, n_min=3, n_max=30)
  L, D, V = _device_inputs(batch, cfg['num_eig_vec'])
  nf, mask = _t(batch['node_feat']), _t(batch['node_mask'])
  with torch.no_grad():
    if route == 'strip':
      with warnings.catch_warnings():
        warnings.filterwarnings('error', message='.*library-GEMM path')   # the fused path does not say it
        score = net(nf, L, D, V, mask=mask)
      assert ops.last_kernel().startswith('lanczosnet_strip_kernel<0,0,'), ops.last_kernel()
      assert ops.last_kernel().endswith(',true>' if gemm == 'f16x3' else ',false>'), ops.last_kernel()
    else:
      with pytest.warns(UserWarning, match='library-GEMM path'):
        score = net(nf, L, D, V, mask=mask)
      with warnings.catch_warnings():
        warnings.filterwarnings('error', message='.*library-GEMM path')   # said once
        again = net(nf, L, D, V, mask=mask)
      assert torch.equal(score, again)
  score = score.cpu().numpy()
  ref = oracle.lanczos_net_forward(P, cfg, batch['node_feat'], L.cpu().numpy(), D.cpu().numpy(),
                                   V.cpu().numpy(), batch['node_mask'], dtype=np.float64)
  e_rows, e_all = rel_err_rows(score, ref), rel_err(score, ref)
  print('forward %s (%s path): per-molecule rel err vs fp64 oracle %.3e (batch-normalised %.3e)'
        % (name, route, e_rows, e_all))
  assert np.isfinite(score).all()
  if gemm == 'f16x3':
    assert e_all < 1e-5     # the bar of test_split_precision_f16x3_mode_meets_parity_bar
  else:
    assert e_rows < 1e-5


def _train_cfg(S):
  return dict(num_atom=13, num_bond_type=2, short_diffusion_dist=[], long_diffusion_dist=DIST16[:S],
              num_eig_vec=12, spectral_filter_kind='MLP', input_dim=32, hidden_dim=[128, 128, 128],
              output_dim=4, num_layer=3)


@pytest.mark.parametrize('S', [9, 12])
def test_hip_backward_matches_the_torch_route_above_eight_scales(S):
  """The HIP backward on the strip kernels with more long scales than the hand-written filter-MLP
  gradient takes (its S <= 8: autograd through the small MLP there) against the torch route."""
  cfg = _train_cfg(S)
  net = _model(cfg, oracle.make_lanczosnet_params(cfg, 21)).train()
  assert net._fused_backward_supported()
  batch = draw_batch(29, seed=8, n_min=4, n_max=24, num_atom=13, num_bond_type=2, num_label=4)
  L, D, V = _device_inputs(batch, 12)
  mask, label, nf = _t(batch['node_mask']), _t(batch['label']), _t(batch['node_feat'])
  got = {}
  for impl in ('hip', 'torch'):
    net.backward_impl = impl
    net.zero_grad(set_to_none=True)
    score, loss = net(nf, L, D, V, label=label, mask=mask)
    loss.backward()
    got[impl] = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
  assert set(got['hip']) == set(got['torch']) == set(k for k, _ in net.named_parameters())
  worst = 0.0
  for k in got['hip']:
    a, b = got['hip'][k], got['torch'][k]
    worst = max(worst, (a - b).abs().max().item() / b.abs().max().item())
    assert (a - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-9, k
  print('training S=%d: HIP route vs torch route, worst %.2e of max |g|' % (S, worst))


def test_training_at_thirteen_scales_runs_and_matches_float64_autograd():
  """Thirteen long scales are beyond the fused kernels: training takes the differentiable library
  route, and its parameter gradients are those of the reference's operator sequence in float64
  (oracle.lanczos_net_forward_torch under autograd)."""
  cfg = _train_cfg(13)
  P = oracle.make_lanczosnet_params(cfg, 22)
  net = _model(cfg, P).train()
  assert not net._fused_backward_supported()
  batch = draw_batch(29, seed=8, n_min=4, n_max=24, num_atom=13, num_bond_type=2, num_label=4)
  L, D, V = _device_inputs(batch, 12)
  cot = np.random.RandomState(3).randn(29, 4)
  with pytest.warns(UserWarning, match='library-GEMM path'):
    score = net(_t(batch['node_feat']), L, D, V, mask=_t(batch['node_mask']))
  (score * _t(cot.astype(np.float32))).sum().backward()
  P64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
  ref = oracle.lanczos_net_forward_torch(P64, cfg, batch['node_feat'], L.cpu().numpy(), D.cpu().numpy(),
                                         V.cpu().numpy(), batch['node_mask'], dtype=torch.float64,
                                         differentiable=True)
  assert rel_err_rows(score.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
  (ref * torch.from_numpy(cot)).sum().backward()
  worst = 0.0
  for k, p in net.named_parameters():
    assert p.grad is not None and P64[k].grad is not None, k
    a, b = p.grad.detach().cpu().double(), P64[k].grad
    worst = max(worst, (a - b).abs().max().item() / b.abs().max().item())
    assert (a - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-9, k
  print('training S=13 (library route) vs float64 autograd: worst %.2e of max |g|' % worst)


@pytest.mark.parametrize('S,B,pairs', [(12, 8, True), (12, 1024, True), (16, 37, False), (16, 1024, True)])
def test_gain_grad_kernel_at_twelve_and_sixteen_scales(S, B, pairs):
  """test_gain_grad_kernel_matches_the_eigen_space_formula's check where the strip form ends
  (12 scales: the eight waves' partial sums just fit its dY buffer) and on the 32-row-tile form
  beyond it (16), against plain torch (fp32) at that test's 2e-6; dead slots exactly zero, repeated
  launches bit-identical."""
  from lanczosnet_amd import ops
  cfg = dict(oracle.DEFAULT_QM8_CFG, long_diffusion_dist=DIST16[:S])
  net = _model(cfg, oracle.make_lanczosnet_params(cfg, 1))
  batch = draw_batch(B, seed=2)
  n = _t(batch['n_nodes'])
  mask = _t(batch['node_mask']).to(torch.uint8).contiguous()
  L = ops.laplacian_l4(_t(batch['adjs']), n)
  K, Lnum, dh = cfg['num_eig_vec'], cfg['num_layer'], 128
  D, V = ops.lanczos_ritz(L[..., 0], n, K)
  plan = net._plan_backward()
  Lp = ops.pack_laplacian_for(plan, L)
  N, din0p = V.shape[1], plan['din0']
  g = torch.Generator(device=DEV).manual_seed(1)
  rows = (torch.arange(32, device=DEV)[None, :] < n[:, None]).float()
  act = torch.rand((Lnum, B, 32, dh), device=DEV, generator=g) * rows[None, :, :, None]
  dy = torch.randn((Lnum, B, 32, dh), device=DEV, generator=g) * rows[None, :, :, None]
  x0 = torch.randn((B, 32, din0p), device=DEV, generator=g) * rows[:, :, None]
  tiles = ops.plan_tiles(mask, allow_pairs=pairs)
  dG = ops.lanczosnet_gain_grad(plan, Lp, V, None, mask, act, x0, dy, tiles)
  assert torch.equal(dG, ops.lanczosnet_gain_grad(plan, Lp, V, None, mask, act, x0, dy, tiles))
  n_chan = S + cfg['num_bond_type'] + 1
  Vt = V.transpose(1, 2)
  ref = []
  for la in range(Lnum):
    X = x0[:, :N] if la == 0 else act[la - 1][:, :N]
    W = net._mix_weight(la).detach().view(dh, n_chan, -1)[:, :S, :]
    W = torch.nn.functional.pad(W, (0, X.shape[2] - W.shape[2]))
    Qs = torch.einsum('bki,osi->bkso', torch.bmm(Vt, X), W)
    ref.append((Qs * torch.bmm(Vt, dy[la][:, :N]).unsqueeze(2)).sum(3))
  ref = torch.stack(ref)
  err = (dG - ref).abs().max().item() / ref.abs().max().item()
  print('gain grad S=%d B=%d pairs=%s: %.2e of max |dG|' % (S, B, pairs, err))
  assert (dG - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()
  dead = (torch.arange(K, device=DEV)[None, :] >= n[:, None])
  assert (dG[:, dead] == 0).all()
