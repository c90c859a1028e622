"""GPU: the GAT backward kernels (csrc/gat_grad.hip) against float64 autograd through tests/gat_mirror.py,
and the module's opt-in route 'gat_hip_train' against the reference's own numbers in tests/golden/gat.npz
and against float64 autograd through the restatement of tests/gat_grad_mirror.py.

Bar of the kernel-level cases, derived as tests/test_gpu_gat.py derives its own: truth = float64 autograd;
e32 = the error of the same autograd in CPU float32 in units of max|truth| of that gradient tensor, the
LARGEST of eight evaluations (the inputs as given and seven with the molecules and the nodes consistently
permuted, the gradients un-permuted); the kernel has to be within max(4 e32, 4 * 2^-23) of max|truth|.
(The kernel's summation order is one more draw of the same rounding; the eight draws of one tensor differ by
up to 14x for the scalar-sized db1 / db2, whose terms nearly cancel because each softmax column's dE sums
to zero: one draw is no yardstick there.)  Where the float64 gradient is identically zero (N = 1: da1, db1,
da2, db2) the kernel's has to be exactly 0.
Module level: per parameter group, max(1e-5, 4 e32) of the group's max|truth| (1e-5: the project's gradient
bar; e32 as above — the float32 gradients of the att_net_* groups are 1e-5 .. 4e-4 off by
cancellation, every other group is below 4e-6)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import gat_grad_mirror as M
import gat_mirror as G
import test_gpu_gat as FWD

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


def _check(names, got, truth, e32, what):
  """every gradient within max(4 e32, 4 ulp) of max|truth|; exactly 0 where the truth is identically 0"""
  for name, g, t, e in zip(names, got, truth, e32):
    g = g.double().cpu()
    assert tuple(g.shape) == tuple(t.shape), name
    assert torch.isfinite(g).all(), name
    scale = float(t.abs().max())
    if scale == 0.0:
      print('%s %s: truth identically 0, kernel max %.2e' % (what, name, float(g.abs().max())))
      assert float(g.abs().max()) == 0.0, name
      continue
    err = float((g - t).abs().max()) / scale
    bar = max(4.0 * e, 4.0 * ULP)
    print('%s %s: %.2e of the scale, float32 reference (worst of 8) %.2e, bar %.2e' % (what, name, err, e, bar))
    assert err <= bar, (name, err, bar)


def _device_L(L, lkind, B, N, C):
  """(host L as the mirror sees it, device L as the kernel reads it)"""
  if lkind == 'expanded':   # one channel, seen C times through a zero stride
    Ld = L[..., :1].cuda().expand(B, N, N, C)
    assert Ld.stride(3) == 0
    return L[..., :1].expand(B, N, N, C), Ld
  if lkind == 'sliced':     # channels 1, 3, .. of a wider tensor: stride_ch = 2, stride_c = 2 C + 1
    wide = torch.zeros(B, N, N, 2 * C + 1, device='cuda')
    wide[..., 1:2 * C:2] = L.cuda()
    Ld = wide[..., 1:2 * C:2]
    assert Ld.stride(3) == 2 and Ld.stride(2) == 2 * C + 1
    return L, Ld
  return L, L.cuda()


def _attention_case(seed, B, N, C, H, Dh, elu, pad=0, lkind='plain', s_scale=1.0):
  """-> (device results of ops.gat_attention_backward, dWh's padded buffer, truth, e32)"""
  from lanczosnet_amd import ops
  Wh, L, a1, b1, a2, b2, bias = FWD._attention_operands(seed, B, N, C, H, Dh, s_scale=s_scale)
  dOut = torch.randn(B, N, C * H * Dh, generator=torch.Generator().manual_seed(seed + 1))
  L, Ld = _device_L(L, lkind, B, N, C)
  w = C * H * Dh
  Whd, dOutd = FWD._padded(Wh, pad), FWD._padded(dOut, pad)
  outbuf = torch.full((B, N, w + pad), float('nan'), device='cuda')
  dev = [x.cuda() for x in (a1, b1, a2, b2)]
  out = ops.gat_attention(Whd, Ld, dev[0], dev[1], dev[2], dev[3], bias.cuda(), H, elu=elu, out=outbuf[:, :, :w])
  gbuf = torch.full((B, N, w + pad), float('nan'), device='cuda')
  got = ops.gat_attention_backward(Whd, Ld, *dev, out if elu else None, dOutd, H, elu=elu, dWh=gbuf[:, :, :w])
  ops32 = (Wh, L, a1, b1, a2, b2, bias, dOut)
  truth = M.attention_autograd(*(x.double() for x in ops32), H, elu)
  return got, gbuf, truth, M.attention_e32(ops32, truth, H, elu)


@pytest.mark.parametrize('N,C,H,Dh,B,elu,pad,lkind', FWD.ATTENTION_CASES)
def test_gat_attention_backward_matches_float64_autograd(N, C, H, Dh, B, elu, pad, lkind):
  got, gbuf, truth, e32 = _attention_case(1000 + N + 7 * C + 13 * Dh, B, N, C, H, Dh, elu, pad, lkind)
  _check(M.ATT_NAMES, got, truth, e32, 'gat_attention_backward N %d C %d H %d Dh %d B %d' % (N, C, H, Dh, B))
  if pad:   # the NaN beyond the width of Wh / out / dOut reached no result; nothing written beyond dWh's
    assert torch.isnan(gbuf[:, :, C * H * Dh:]).all()
  if N == 1:
    for k in (1, 2, 3, 4):
      assert float(truth[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0


def test_gat_attention_backward_at_logits_of_100():
  """s1, s2 scaled until the logits reach +-100 (the forward test's construction)"""
  N, C, H, Dh, B = 17, 2, 3, 16, 3
  got, _, truth, e32 = _attention_case(77, B, N, C, H, Dh, True, s_scale=50.0)
  _check(M.ATT_NAMES, got, truth, e32, 'gat_attention_backward at +-100 logits')


def test_gat_attention_backward_is_bitwise_reproducible_and_the_raw_op_gives_the_same_bits():
  from lanczosnet_amd import ops
  N, C, H, Dh, B = 31, 7, 8, 16, 5
  Wh, L, a1, b1, a2, b2, bias = (x.cuda() for x in FWD._attention_operands(79, B, N, C, H, Dh))
  dOut = torch.randn(B, N, C * H * Dh, device='cuda')
  out = ops.gat_attention(Wh, L, a1, b1, a2, b2, bias, H)
  r1 = ops.gat_attention_backward(Wh, L, a1, b1, a2, b2, out, dOut, H)
  r2 = ops.gat_attention_backward(Wh, L, a1, b1, a2, b2, out, dOut, H)
  for x, y in zip(r1, r2):
    assert torch.equal(x, y)
  w, CH = C * H * Dh, C * H
  ws = torch.empty(torch.ops.lanczosnet.raw_gat_attention_backward_workspace_floats(B, C, H, Dh), device='cuda')
  new = lambda *s: torch.full(s, float('nan'), device='cuda')  # noqa: E731
  dWh, da1, db1, da2, db2, dbias = new(B, N, w), new(CH, Dh), new(CH), new(CH, Dh), new(CH), new(CH, Dh)
  torch.ops.lanczosnet.raw_gat_attention_backward(Wh, w, L, L.stride(0), L.stride(1), L.stride(2), L.stride(3),
                                                  a1, b1, a2, b2, out, w, dOut, w, B, N, C, H, Dh, 1, ws, dWh, w,
                                                  da1, db1, da2, db2, dbias)
  for x, y in zip(r1, (dWh, da1, db1, da2, db2, dbias)):
    assert torch.equal(x, y)


def _readout_operands(N, B, Dh, CH, P, mkind):
  g = torch.Generator().manual_seed(2000 + N + 3 * CH + P)
  Hl = torch.randn(B, N, CH * Dh, generator=g)
  Wo, wg = 0.4 * torch.randn(P, Dh, generator=g), 0.4 * torch.randn(1, Dh, generator=g)
  bo, bg = 0.1 * torch.randn(P, generator=g), 0.1 * torch.randn(1, generator=g)
  mask = None
  if mkind is not None:
    n = torch.randint(1, N + 1, (B,), generator=g) if mkind == 'ragged' else torch.ones(B, dtype=torch.long)
    mask = (torch.arange(N).unsqueeze(0) < n.unsqueeze(1)).to(torch.uint8)
  return Hl, mask, Wo, bo, wg, bg, torch.randn(B, P, generator=g)


@pytest.mark.parametrize('N,B,Dh,CH,P,mkind,pad', FWD.READOUT_CASES)
def test_gat_readout_backward_matches_float64_autograd(N, B, Dh, CH, P, mkind, pad):
  from lanczosnet_amd import ops
  Hl, mask, Wo, bo, wg, bg, dscore = _readout_operands(N, B, Dh, CH, P, mkind)
  gbuf = torch.full((B, N, CH * Dh + pad), float('nan'), device='cuda')
  got = ops.gat_readout_backward(FWD._padded(Hl, pad), None if mask is None else mask.cuda(), Wo.cuda(), bo.cuda(),
                                 wg.cuda(), bg.cuda(), CH, dscore.cuda(), dHlast=gbuf[:, :, :CH * Dh])
  d = lambda x: x.double()  # noqa: E731
  truth = M.readout_autograd(d(Hl), mask, d(Wo), d(bo), d(wg), d(bg), CH, d(dscore))
  e32 = M.readout_e32((Hl, mask, Wo, bo, wg, bg, dscore), truth, CH)
  _check(M.RO_NAMES, got, truth, e32, 'gat_readout_backward N %d B %d Dh %d CH %d P %d' % (N, B, Dh, CH, P))
  if mask is not None and bool((mask == 0).any()):
    outside = got[0].cpu()[mask == 0]
    assert float(outside.abs().max()) == 0.0                            # exactly 0 outside the mask
  if pad:
    assert torch.isnan(gbuf[:, :, CH * Dh:]).all()


def test_gat_readout_backward_is_bitwise_reproducible_and_the_raw_op_gives_the_same_bits():
  from lanczosnet_amd import ops
  N, B, Dh, CH, P = 17, 67, 16, 56, 16
  Hl, mask, Wo, bo, wg, bg, dscore = (None if x is None else x.cuda()
                                      for x in _readout_operands(N, B, Dh, CH, P, 'ragged'))
  r1 = ops.gat_readout_backward(Hl, mask, Wo, bo, wg, bg, CH, dscore)
  r2 = ops.gat_readout_backward(Hl, mask, Wo, bo, wg, bg, CH, dscore)
  for x, y in zip(r1, r2):
    assert torch.equal(x, y)
  ws = torch.empty(torch.ops.lanczosnet.raw_gat_readout_backward_workspace_floats(B, Dh, P), device='cuda')
  new = lambda *s: torch.full(s, float('nan'), device='cuda')  # noqa: E731
  dH, dWo, dbo, dwg, dbg = new(B, N, CH * Dh), new(P, Dh), new(P), new(Dh), new(1)
  torch.ops.lanczosnet.raw_gat_readout_backward(Hl, CH * Dh, mask, Wo, bo, wg.reshape(-1), bg, dscore, B, N, CH, Dh,
                                                P, ws, dH, CH * Dh, dWo, dbo, dwg, dbg)
  for x, y in zip(r1, (dH, dWo, dbo, dwg, dbg)):
    assert torch.equal(x, y)


def test_out_of_envelope_backward_arguments_raise_not_supported():
  from lanczosnet_amd import ops
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def att(N, C, H, Dh, host=False):
    w = C * H * Dh
    return ops.gat_attention_backward(torch.zeros(1, N, w) if host else z(1, N, w), z(1, N, N, C), z(C * H, Dh),
                                      z(C * H), z(C * H, Dh), z(C * H), z(1, N, w), z(1, N, w), H)
  for shape in ((33, 1, 2, 16), (8, 1, 2, 6), (8, 9, 2, 16), (8, 1, 17, 16)):
    with pytest.raises(ops.NotSupported):
      att(*shape)
  with pytest.raises(ops.NotSupported):
    ops.gat_readout_backward(z(1, 8, 64), None, z(17, 16), z(17), z(1, 16), z(1), 4, z(1, 17))
  with pytest.raises(ops.NotSupported):
    ops.gat_readout_backward(z(1, 33, 64), None, z(16, 16), z(16), z(1, 16), z(1), 4, z(1, 16))
  with pytest.raises(ops.LnzError):
    ops.gat_attention_backward(z(1, 8, 64), z(1, 8, 8, 2), z(4, 16), z(4), z(4, 16), z(4), None, z(1, 8, 64), 2)
  with pytest.raises(RuntimeError):
    att(8, 1, 2, 16, host=True)
  with pytest.raises(RuntimeError):
    ops.gat_readout_backward(torch.zeros(1, 8, 64), None, z(16, 16), z(16), z(1, 16), z(1), 4, z(1, 16))


# ------------------------------------------------------------------------------------------ module
def _net(name, g, dropout=None):
  net, cfg, batch, P, d = FWD._net(name, g)
  if dropout is not None:
    from lanczosnet_amd.model import GAT
    keys, _ = G.CASES[name]
    cfg = G.make_config(dropout=dropout, **keys)
    fresh = GAT(cfg)
    fresh.load_state_dict(net.state_dict())
    net = fresh.cuda()
  net.gat_backward_impl = 'hip'
  return net, cfg, batch, P, d


def _step(net, d):
  net.zero_grad(set_to_none=True)
  score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  loss.backward()
  return score.detach(), loss.detach()


def test_gat_hip_training_route_matches_the_reference_gradients():
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net('b', g)
  net.train()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score, loss = _step(net, d)
    assert net.last_route == 'gat_hip_train'
    with torch.no_grad():
      ref = net(d['node_feat'], d['L'], mask=d['node_mask'])
    assert net.last_route == 'gat_hip'
  assert not [w for w in rec if 'gat_torch' in str(w.message)]
  assert torch.equal(score, ref)                                         # the inference route's bits
  assert abs(float(loss) - float(g['b_loss'])) < 1e-5 * abs(float(g['b_loss']))
  gd = dict(net.named_parameters())
  for k, gs, ga, none in zip(g['b_names'], g['b_gsum'], g['b_gabs'], g['b_grad_none']):
    gr = gd[str(k)].grad
    assert (gr is None) == bool(none), k
    if gr is None:
      continue
    tol = 2e-4 * float(ga) + 1e-9
    assert abs(float(gr.double().sum()) - float(gs)) < tol, (k, float(gr.double().sum()), float(gs))
    assert abs(float(gr.double().abs().sum()) - float(ga)) < tol, k


@functools.lru_cache(maxsize=None)
def _truth(name):
  """(float64 gradients by name, per group: names, max|truth|, e32 = worst of eight float32 evaluations)"""
  g = load_golden('gat.npz')
  cfg, batch = G.case_inputs(name)
  shapes = [tuple(int(x) for x in str(s).split('x')) for s in g[name + '_shapes']]
  P = G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])
  g64, _ = M.net_gradients(P, cfg, batch, torch.float64)
  groups = M.param_groups(P.keys(), cfg)
  B, N = batch['node_feat'].shape
  e32 = {gn: 0.0 for gn, _ in groups}
  for perm in [None] + M.permutations(B, N)[1:]:
    g32, _ = M.net_gradients(P, cfg, batch, torch.float32, perm)
    for gn, names in groups:
      t = torch.cat([g64[k].reshape(-1) for k in names])
      a = torch.cat([g32[k].reshape(-1) for k in names]).double()
      e32[gn] = max(e32[gn], float((a - t).abs().max()) / float(t.abs().max()))
  return g64, groups, e32


@pytest.mark.parametrize('name', ['c', 'd', 'b'])
def test_gat_hip_training_gradients_match_float64_autograd(name):
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.train()
  _step(net, d)
  assert net.last_route == 'gat_hip_train'
  g64, groups, e32 = _truth(name)
  gd = dict(net.named_parameters())
  assert {k for k, v in g64.items() if v is None} == {k for k, p in gd.items() if p.grad is None}
  failed = []
  for gn, names in groups:
    t = torch.cat([g64[k].reshape(-1) for k in names])
    a = torch.cat([gd[k].grad.reshape(-1) for k in names]).double().cpu()
    err = float((a - t).abs().max()) / float(t.abs().max())
    bar = max(1e-5, 4.0 * e32[gn])
    print('GAT case %s group %s: %.2e of the scale, float32 autograd (worst of 8) %.2e, bar %.2e'
          % (name, gn, err, e32[gn], bar))
    if not err <= bar:
      failed.append((gn, err, bar))
  assert not failed, failed


def test_two_backward_passes_give_bitwise_equal_gradients():
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net('d', g)
  net.train()
  _step(net, d)
  first = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
  _step(net, d)
  second = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
  assert set(first) == set(second) and all(torch.equal(first[k], second[k]) for k in first)


def test_an_adam_step_moves_the_next_forward_like_the_torch_route():
  from lanczosnet_amd.train import make_adam
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net('c', g)
  net.train()
  opt = make_adam(net.parameters(), lr=1e-2)
  before, _ = _step(net, d)
  opt.step()
  after, _ = _step(net, d)
  assert net.last_route == 'gat_hip_train' and not torch.equal(before, after)
  net.gat_backward_impl = 'torch'
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    tor, _ = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  assert net.last_route == 'gat_torch'
  err = float((after.double() - tor.detach().double()).abs().max() / tor.detach().double().abs().max())
  print('after one Adam step: gat_hip_train vs gat_torch on the updated weights %.2e' % err)
  assert err <= 1e-5


def test_dropout_in_training_still_takes_the_torch_route_and_inference_the_kernels():
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net('c', g, dropout=0.5)
  net.train()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    _step(net, d)
  assert net.last_route == 'gat_torch'
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'gat_torch' in str(w.message)]
  assert len(mine) == 1 and 'dropout' in str(mine[0].message)
  with torch.no_grad():
    net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'gat_torch'                                   # training mode: dropout draws even so
  net.eval()
  net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'gat_hip_train'                               # eval, gradients on: the kernels, saved for backward
  with torch.no_grad():
    net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'gat_hip'
  net.gat_backward_impl = 'torch'
  with torch.no_grad():
    net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'gat_hip'
