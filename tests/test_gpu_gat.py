"""GPU: the GAT kernels (csrc/gat.hip) against the float64 restatement of tests/gat_mirror.py, and
the module's two routes against the reference's own numbers in tests/golden/gat.npz.

Bar of the kernel-level cases: the reference arithmetic is the CPU float32 torch evaluation of the
same single-layer formula on the same inputs; its error e32 against float64 is measured at run time
and the kernel has to be within max(4 e32, 4 fp32 ulps) max|out| of float64.  (4: another summation
order draws another sample of the same rounding — eight reordered or one-ulp-perturbed float32 runs
of the reference spread 2.5x between best and worst; the ulp floor: the device expf / expm1f are
accurate to 1-2 ulp, and at N = 1 the reference's own error is near zero.)
Module level: max(1e-5, 4 e_ref) max|s64| with e_ref read from the fixture."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import gat_mirror as G

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23


def _bar(got, ref32, ref64):
  scale = float(ref64.abs().max())
  e32 = float((ref32.double() - ref64).abs().max()) / scale
  err = float((got.double().cpu() - ref64).abs().max()) / scale
  return err, e32, max(4.0 * e32, 4.0 * ULP)


def _attention_operands(seed, B, N, C, H, Dh, s_scale=1.0):
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
  u = lambda *s: torch.rand(*s, generator=g) * 0.2 - 0.1  # noqa: E731
  Wh = 0.5 * r(B, N, C * H * Dh)
  L = 0.5 * torch.rand(B, N, N, C, generator=g)
  a1, a2 = 0.3 * s_scale * r(C * H, Dh), 0.3 * s_scale * r(C * H, Dh)
  return Wh, L, a1, u(C * H), a2, u(C * H), u(C * H, Dh)


def _padded(x, pad):
  """x [B, N, W] as a view of a [B, N, W + pad] device buffer filled with NaN beyond the width"""
  buf = torch.full(x.shape[:2] + (x.shape[2] + pad,), float('nan'), device='cuda')
  buf[:, :, :x.shape[2]] = x.cuda()
  return buf[:, :, :x.shape[2]]


# (N, C, H, Dh, B, elu, row padding, how L reaches the kernel): every value of every axis, and the
# corners where two upper limits meet (N x C x H x Dh all at their limits; each pair with the others low)
ATTENTION_CASES = [
    (1, 1, 1, 4, 1, True, 0, 'plain'),
    (5, 2, 3, 16, 3, False, 0, 'plain'),
    (16, 7, 8, 16, 3, True, 8, 'plain'),
    (17, 2, 3, 32, 1, True, 0, 'sliced'),
    (31, 2, 3, 4, 65, False, 4, 'expanded'),
    (32, 8, 16, 32, 3, True, 0, 'plain'),
    (32, 7, 8, 16, 65, True, 0, 'plain'),
    (32, 8, 16, 4, 1, False, 0, 'plain'),
    (32, 1, 1, 32, 1, True, 0, 'plain'),
    (1, 8, 16, 32, 3, True, 0, 'plain'),
    # a round of four heads after the first with live and idle waves: H = 5 (1 of 4), 13 (1 of 4), 6 (2 of 4)
    (9, 2, 5, 8, 2, True, 0, 'plain'),
    (32, 1, 13, 32, 1, False, 0, 'plain'),
    (17, 3, 6, 16, 2, True, 4, 'plain'),
]


@pytest.mark.parametrize('N,C,H,Dh,B,elu,pad,lkind', ATTENTION_CASES)
def test_gat_attention_matches_float64(N, C, H, Dh, B, elu, pad, lkind):
  from lanczosnet_amd import ops
  Wh, L, a1, b1, a2, b2, bias = _attention_operands(1000 + N + 7 * C + 13 * Dh, B, N, C, H, Dh)
  if lkind == 'expanded':   # one channel, seen C times through a zero stride
    L = L[..., :1].expand(B, N, N, C)
    Ld = L[..., :1].cuda().expand(B, N, N, C)
    assert Ld.stride(3) == 0
  elif lkind == 'sliced':   # channels 1, 3, .. of a wider tensor: stride_ch = 2, stride_c = 2 C + 1
    wide = torch.zeros(B, N, N, 2 * C + 1, device='cuda')
    wide[..., 1:2 * C:2] = L.cuda()
    Ld = wide[..., 1:2 * C:2]
    assert Ld.stride(3) == 2 and Ld.stride(2) == 2 * C + 1
  else:
    Ld = L.cuda()
  Whd = _padded(Wh, pad)
  outbuf = torch.full((B, N, C * H * Dh + pad), float('nan'), device='cuda')
  out = ops.gat_attention(Whd, Ld, a1.cuda(), b1.cuda(), a2.cuda(), b2.cuda(), bias.cuda(), H, elu=elu,
                          out=outbuf[:, :, :C * H * Dh])
  ref32 = G.attention(Wh, L, a1, b1, a2, b2, bias, H, elu)
  ref64 = G.attention(*(x.double() for x in (Wh, L, a1, b1, a2, b2, bias)), H, elu)
  err, e32, bar = _bar(out, ref32, ref64)
  print('gat_attention N %d C %d H %d Dh %d B %d: %.2e of the scale, float32 reference %.2e, bar %.2e'
        % (N, C, H, Dh, B, err, e32, bar))
  assert torch.isfinite(out).all()
  assert err <= bar
  if pad:
    assert torch.isnan(outbuf[:, :, C * H * Dh:]).all()     # nothing written beyond the width


def test_gat_attention_subtracts_the_column_maximum():
  """s1, s2 scaled until the logits reach +-100: exp of the raw logit overflows float32"""
  from lanczosnet_amd import ops
  N, C, H, Dh, B = 17, 2, 3, 16, 3
  Wh, L, a1, b1, a2, b2, bias = _attention_operands(77, B, N, C, H, Dh, s_scale=50.0)
  s1 = torch.einsum('bnkd,kd->bnk', Wh.view(B, N, C * H, Dh), a1)
  s2 = torch.einsum('bnkd,kd->bnk', Wh.view(B, N, C * H, Dh), a2)
  assert float((s1.max(dim=1)[0] + s2.max(dim=1)[0]).max()) > 100.0 and float(s1.min() + s2.min()) < -100.0
  out = ops.gat_attention(*(x.cuda() for x in (Wh, L, a1, b1, a2, b2, bias)), H, elu=True)
  ref32 = G.attention(Wh, L, a1, b1, a2, b2, bias, H, True)
  ref64 = G.attention(*(x.double() for x in (Wh, L, a1, b1, a2, b2, bias)), H, True)
  err, e32, bar = _bar(out, ref32, ref64)
  print('gat_attention at +-100 logits: %.2e of the scale, float32 reference %.2e, bar %.2e' % (err, e32, bar))
  assert torch.isfinite(out).all()
  assert err <= bar


def test_gat_attention_runs_over_the_padded_rows():
  """property 1: L is zero beyond n < N, and the padded rows and columns still take part in the
  softmax and the aggregate — compared at the same padded N"""
  from lanczosnet_amd import ops
  N, C, H, Dh, B = 16, 2, 3, 16, 3
  Wh, L, a1, b1, a2, b2, bias = _attention_operands(78, B, N, C, H, Dh)
  for b, n in enumerate((16, 9, 1)):
    L[b, n:] = 0.0
    L[b, :, n:] = 0.0
  out = ops.gat_attention(*(x.cuda() for x in (Wh, L, a1, b1, a2, b2, bias)), H, elu=True)
  ref32 = G.attention(Wh, L, a1, b1, a2, b2, bias, H, True)
  ref64 = G.attention(*(x.double() for x in (Wh, L, a1, b1, a2, b2, bias)), H, True)
  err, e32, bar = _bar(out, ref32, ref64)
  print('gat_attention on padded molecules: %.2e of the scale, float32 reference %.2e' % (err, e32))
  assert err <= bar
  # a masked softmax over the real block gives something else: the padding is not ignored
  real = G.attention(*(x.double() for x in (Wh[1:2, :9], L[1:2, :9, :9], a1, b1, a2, b2, bias)), H, True)
  assert float((real - ref64[1:2, :9]).abs().max()) > 1e-3


def test_gat_attention_is_bitwise_reproducible_and_the_raw_op_gives_the_same_bits():
  from lanczosnet_amd import ops
  N, C, H, Dh, B = 31, 7, 8, 16, 5
  Wh, L, a1, b1, a2, b2, bias = (x.cuda() for x in _attention_operands(79, B, N, C, H, Dh))
  out1 = ops.gat_attention(Wh, L, a1, b1, a2, b2, bias, H)
  out2 = ops.gat_attention(Wh, L, a1, b1, a2, b2, bias, H)
  assert torch.equal(out1, out2)
  raw = torch.empty_like(out1)
  w = C * H * Dh
  torch.ops.lanczosnet.raw_gat_attention(Wh, w, L, L.stride(0), L.stride(1), L.stride(2), L.stride(3), a1, b1,
                                         a2, b2, bias, B, N, C, H, Dh, 1, raw, w)
  assert torch.equal(raw, out1)


# (N, B, Dh, CH, P, mask, row padding)
READOUT_CASES = [
    (1, 1, 4, 1, 1, None, 0),
    (5, 3, 16, 56, 16, 'ragged', 0),
    (32, 65, 32, 128, 16, 'one', 0),
    (17, 3, 16, 56, 1, 'ragged', 8),
    (31, 1, 32, 1, 16, None, 0),
    (16, 3, 4, 128, 1, 'one', 0),
]


@pytest.mark.parametrize('N,B,Dh,CH,P,mkind,pad', READOUT_CASES)
def test_gat_readout_matches_float64(N, B, Dh, CH, P, mkind, pad):
  from lanczosnet_amd import ops
  g = torch.Generator().manual_seed(2000 + N + 3 * CH + P)
  Hl = torch.randn(B, N, CH * Dh, generator=g)
  Wo, wg = 0.4 * torch.randn(P, Dh, generator=g), 0.4 * torch.randn(1, Dh, generator=g)
  bo, bg = 0.1 * torch.randn(P, generator=g), 0.1 * torch.randn(1, generator=g)
  mask = None
  if mkind is not None:
    n = torch.randint(1, N + 1, (B,), generator=g) if mkind == 'ragged' else torch.ones(B, dtype=torch.long)
    mask = (torch.arange(N).unsqueeze(0) < n.unsqueeze(1)).to(torch.uint8)
  got = ops.gat_readout(_padded(Hl, pad), None if mask is None else mask.cuda(), Wo.cuda(), bo.cuda(), wg.cuda(),
                        bg.cuda(), CH)
  ref32 = G.readout(Hl, mask, Wo, bo, wg, bg, CH)
  ref64 = G.readout(Hl.double(), mask, Wo.double(), bo.double(), wg.double(), bg.double(), CH)
  err, e32, bar = _bar(got, ref32, ref64)
  print('gat_readout N %d B %d Dh %d CH %d P %d: %.2e of the scale, float32 reference %.2e, bar %.2e'
        % (N, B, Dh, CH, P, err, e32, bar))
  assert tuple(got.shape) == (B, P) and err <= bar


def test_gat_readout_of_a_molecule_without_nodes_is_nan():
  from lanczosnet_amd import ops
  Hl = torch.randn(2, 5, 32, device='cuda')
  mask = torch.tensor([[1, 1, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=torch.uint8, device='cuda')
  s = ops.gat_readout(Hl, mask, torch.randn(3, 16, device='cuda'), torch.zeros(3, device='cuda'),
                      torch.randn(1, 16, device='cuda'), torch.zeros(1, device='cuda'), 2)
  assert torch.isfinite(s[0]).all() and torch.isnan(s[1]).all()


def test_out_of_envelope_arguments_raise_not_supported():
  from lanczosnet_amd import ops
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def att(N, C, H, Dh):
    return ops.gat_attention(z(1, N, C * H * Dh), z(1, N, N, C), z(C * H, Dh), z(C * H), z(C * H, Dh), z(C * H),
                             z(C * H, Dh), H)
  for shape in ((33, 1, 2, 16), (8, 1, 2, 6), (8, 9, 2, 16)):
    with pytest.raises(ops.NotSupported):
      att(*shape)
  with pytest.raises(ops.NotSupported):
    ops.gat_readout(z(1, 8, 64), None, z(17, 16), z(17), z(1, 16), z(1), 4)
  with pytest.raises(ops.NotSupported):
    ops.gat_readout(z(1, 33, 64), None, z(16, 16), z(16), z(1, 16), z(1), 4)
  with pytest.raises(ops.LnzError):
    ops.gat_attention(z(1, 8, 64), z(1, 8, 8, 2), z(4, 16), z(4), z(4, 16), z(4), z(3, 16), 2)   # a short bias
  with pytest.raises(RuntimeError):
    ops.gat_attention(torch.zeros(1, 8, 64), z(1, 8, 8, 2), z(4, 16), z(4), z(4, 16), z(4), z(4, 16), 2)


# ------------------------------------------------------------------------------------------ module
def _net(name, g):
  from lanczosnet_amd.model import GAT
  cfg, batch = G.case_inputs(name)
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])
  net = GAT(cfg)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  return net.cuda(), cfg, batch, P, {k: t(v) for k, v in batch.items()}


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_gat_module_matches_the_reference_float64_scores(name):
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.eval()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      s1 = net(d['node_feat'], d['L'], mask=d['node_mask'])
      s2 = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'gat_hip' and not [w for w in rec if 'lanczosnet_amd' in str(w.message)]
  assert torch.equal(s1, s2)                                            # bitwise from call to call
  ref = g[name + '_score64']
  err = float(np.abs(s1.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
  bar = max(1e-5, 4.0 * float(g[name + '_e_ref']))
  print('GAT case %s: gat_hip vs reference float64 %.2e (reference float32 %.2e, bar %.2e)'
        % (name, err, float(g[name + '_e_ref']), bar))
  assert err <= bar
  # with a label the call returns (score, loss); no gradient is needed under no_grad -> still the kernels
  with torch.no_grad():
    s3, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  assert net.last_route == 'gat_hip' and torch.equal(s3, s1)
  assert abs(float(loss) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))


def test_gat_training_takes_the_torch_route_and_matches_the_reference_gradients():
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net('b', g)
  net.train()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
    net.zero_grad(set_to_none=True)
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
  assert net.last_route == 'gat_torch'
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'gat_torch' in str(w.message)]
  assert len(mine) == 1 and 'gradients' in str(mine[0].message)         # once per module
  assert abs(float(loss.detach()) - float(g['b_loss'])) < 1e-5 * abs(float(g['b_loss']))
  gd = dict(net.named_parameters())
  for k, gs, ga, none in zip(g['b_names'], g['b_gsum'], g['b_gabs'], g['b_grad_none']):
    gr = gd[str(k)].grad
    assert (gr is None) == bool(none), k
    if gr is None:
      continue
    tol = 2e-4 * float(ga) + 1e-9
    assert abs(float(gr.double().sum()) - float(gs)) < tol, (k, float(gr.double().sum()), float(gs))
    assert abs(float(gr.double().abs().sum()) - float(ga)) < tol, k


def test_an_in_place_update_invalidates_the_stacked_operands():
  g = load_golden('gat.npz')
  net, cfg, batch, P, d = _net('c', g)
  net.eval()
  with torch.no_grad():
    before = net(d['node_feat'], d['L'], mask=d['node_mask'])
    net.filter[1][0][1].weight.mul_(1.5)
    after = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'gat_hip' and not torch.equal(before, after)
  Q = dict(P)
  Q['filter.1.0.1.weight'] = P['filter.1.0.1.weight'] * np.float32(1.5)
  ref = G.forward(Q, cfg, batch['node_feat'], batch['L'], batch['node_mask']).numpy()
  err = float(np.abs(after.cpu().numpy() - ref).max() / np.abs(ref).max())
  assert err <= 1e-5
  # host inputs are moved with one warning
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      host = net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']),
                 mask=torch.from_numpy(batch['node_mask']))
      net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']), mask=d['node_mask'])
  assert torch.equal(host, after) and len([w for w in rec if 'moved there' in str(w.message)]) == 1
