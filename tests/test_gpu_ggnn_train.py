"""GPU: the GGNN backward (csrc/ggnn_grad.hip, the trajectory entry of csrc/ggnn.hip) against float64
autograd through tests/ggnn_mirror.py, and route 'ggnn_hip_train' of the module against the reference's own
numbers in tests/golden/ggnn.npz.

Bar of the kernel-level cases: truth is float64 autograd (ggnn_grad_mirror.propagate_autograd /
readout_autograd); e32 is the error of the CPU float32 autograd of the same formula, the largest of eight
evaluations (the inputs as given and seven with molecules, nodes and channel order consistently permuted),
per gradient tensor in units of max|truth|.  The kernel has to be within max(K e32, 4 * 2^-23) max|truth| per
gradient tensor; where the truth is identically zero the kernel's gradient is exactly 0.  K starts at the
project's 4: another summation order draws another sample of the same rounding.  Measured before relying on
it (CPU, STEP_CASES below with their seeds, the spread worst / best e32 of the eight evaluations per gradient
tensor, the largest over the nine tensors of a case): see SPREAD below — the measurement and what K follows
from it.  The kernel's own output never enters the bar.
Module level: the fixture's loss to 1e-5, its _gsum / _gabs to 2e-4 gabs + 1e-9, and per parameter
max(1e-5, 4 e32) max|truth| against float64 autograd of the whole net."""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import ggnn_grad_mirror as GM
import ggnn_mirror as G

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
# SPREAD: measured on the CPU over STEP_CASES (worst / best e32 of the eight evaluations, largest over the nine
# gradient tensors of a case; e32 itself 5e-8 .. 1.1e-6): 'avg' 1.8 .. 2.3 (2.19 at N 5, 1.83 at N 16, 2.29 at
# N 31: dbih, 1.78 at N 32 with 15 steps), 'sum' 1.0 .. 2.5 (1.00 at N 1, where five of the nine truths are
# identically zero, 2.10 at N 17, 2.51 at N 32: dbhh; no 'sum' case runs 15 steps here) — below 4 for both
# aggregates, so K stays at the project's 4.  The two cases with several molecules per tile: 1.72 at N 5, D 96, 'avg'
# (dbih), 2.14 at N 11, D 64, 'sum' (dbhh).
K = {'avg': 4.0, 'sum': 4.0}

# (N, C, D, B, steps, agg, row padding, how L reaches the kernel); B = 65 crosses a tile boundary with a
# remainder (a tile holds floor(32 / N) molecules)
STEP_CASES = [
    (1, 1, 32, 1, 1, 'sum', 0, 'plain'),
    (5, 2, 32, 3, 2, 'avg', 0, 'plain'),
    (16, 7, 128, 3, 1, 'avg', 8, 'plain'),
    (17, 2, 64, 1, 3, 'sum', 0, 'sliced'),
    (31, 2, 32, 65, 2, 'avg', 4, 'expanded'),
    (32, 8, 128, 3, 15, 'avg', 0, 'plain'),
    (32, 1, 96, 2, 3, 'sum', 0, 'plain'),
    (5, 3, 96, 14, 3, 'avg', 4, 'plain'),                 # tiles of 6, 6, 2 molecules: dead rows, then a tile
    (11, 2, 64, 7, 3, 'sum', 0, 'plain'),                 # tiles of 2, 2, 2, 1
]


def step_case_inputs(N, C, D, B, lkind='plain'):
  """(S_0, L as the formulas see it, the twelve operands, dS_T): fixed seeds, CPU"""
  S, L, W = GM.draw_operands(4000 + N + 7 * C + D, B, N, C, D)
  if lkind == 'expanded':   # one channel, seen C times through a zero stride
    L = L[..., :1].expand(B, N, N, C).contiguous()
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(11 + N))
  return S, L, W, dST


@functools.lru_cache(maxsize=None)
def _step_truth(N, C, D, B, steps, agg, lkind):
  """(truth: the nine float64 gradients, e32: nine numbers) — computed once, shared, never changed"""
  S, L, W, dST = step_case_inputs(N, C, D, B, lkind)
  d = lambda x: x.double()  # noqa: E731
  truth = GM.propagate_autograd(d(S), d(dST), d(L), [d(w) for w in W[:8]], steps, agg)
  e32 = GM.propagate_e32(S, dST, L, W[:8], truth, steps, agg)
  return truth, e32


def _padded(x, pad):
  """x [B, N, W] as a view of a [B, N, W + pad] device buffer filled with NaN beyond the width"""
  buf = torch.full(x.shape[:2] + (x.shape[2] + pad,), float('nan'), device='cuda')
  buf[:, :, :x.shape[2]] = x.cuda()
  return buf[:, :, :x.shape[2]], buf


def _hip_backward(S, dST, Ld, W, steps, agg, pad=0):
  """the trajectory, then the step kernel for t = steps-1 .. 0 with the library GEMMs -> (the nine gradients,
  the two padded dS buffers)"""
  from lanczosnet_amd import ops
  B, N, D = S.shape
  C = Ld.shape[3]
  Wd = [w.cuda() for w in W]
  avg = agg == 'avg'
  _, states = ops.ggnn_forward_states(S.cuda(), Ld, None, *Wd, steps, avg=avg)
  tr = ops.ggnn_pack_transposes(Wd[0], Wd[2], Wd[4], Wd[6])
  bufs = ops.ggnn_step_buffers(B, N, C, D, 'cuda')
  dS, buf_a = _padded(dST, pad)
  spare, buf_b = _padded(torch.zeros(B, N, D), pad)
  grads = [torch.zeros_like(w) for w in Wd[:8]]
  for t in range(steps - 1, -1, -1):
    St, _ = _padded(states[t], pad)
    spare, _ = ops.ggnn_backward_step(St, dS, Ld, *Wd[:8], transposes=tr, avg=avg, dS=spare, buffers=bufs)
    assert ops.last_kernel() == 'ggnn_backward_step_kernel<%d>' % D
    dS, spare = spare, dS
    grads = ops.ggnn_step_weight_grads(St, bufs, C, grads)
  return [dS] + list(grads), (buf_a, buf_b)


def _hold(tag, got, truth, e32, agg):
  for name, x, t, e in zip(GM.STEP_NAMES, got, truth, e32):
    x = x.double().cpu().reshape(t.shape)
    assert torch.isfinite(x).all(), name
    scale = float(t.abs().max())
    if scale == 0.0:
      assert float(x.abs().max()) == 0.0, name
      continue
    err, bar = float((x - t).abs().max()) / scale, max(K[agg] * e, 4.0 * ULP)
    print('ggnn backward %s %s: %.2e of the scale, float32 reference %.2e, bar %.2e' % (tag, name, err, e, bar))
    assert err <= bar, name


@pytest.mark.parametrize('N,C,D,B,steps,agg,pad,lkind', STEP_CASES)
def test_ggnn_backward_steps_match_float64_autograd(N, C, D, B, steps, agg, pad, lkind):
  S, L, W, dST = step_case_inputs(N, C, D, B, lkind)
  if lkind == 'expanded':
    Ld = L[..., :1].cuda().expand(B, N, N, C)
    assert Ld.stride(3) == 0
  elif lkind == 'sliced':   # channels 1, 3, .. of a wider tensor: stride_ch = 2, stride_c = 2 C + 1
    wide = torch.zeros(B, N, N, 2 * C + 1, device='cuda')
    wide[..., 1:2 * C:2] = L.cuda()
    Ld = wide[..., 1:2 * C:2]
    assert Ld.stride(3) == 2 and Ld.stride(2) == 2 * C + 1
  else:
    Ld = L.cuda()
  before = Ld.clone()
  got, bufs = _hip_backward(S, dST, Ld, W, steps, agg, pad)
  assert torch.equal(Ld, before)                                  # L is read, never written
  truth, e32 = _step_truth(N, C, D, B, steps, agg, lkind)
  _hold('N %d C %d D %d B %d steps %d %s' % (N, C, D, B, steps, agg), got, truth, e32, agg)
  if pad:
    for b in bufs:
      assert torch.isnan(b[:, :, D:]).all()                       # nothing written beyond the width


def test_saturated_gates_give_finite_gradients_within_the_bar():
  """the forward test's construction: weights scaled until the gate pre-activations pass +-100"""
  N, C, D, B, steps = 17, 2, 64, 3, 2
  S, L, W = GM.draw_operands(91, B, N, C, D, scale=5.0, density=0.5)
  S = 2.0 * S
  Sd, Ld = S.double(), L.double()
  Wd = [w.double() for w in W]
  A = G.adjacency(Ld, 'avg', torch.float64)
  gi = sum((A[:, c] @ (torch.relu(Sd @ Wd[0][c].t() + Wd[1][c]) @ Wd[2][c].t() + Wd[3][c])) @ Wd[4][:, c * D:(c + 1) * D].t()
           for c in range(C)) + Wd[5]
  gh = Sd @ Wd[6].t() + Wd[7]
  pre_rz, pre_n = (gi + gh)[..., :2 * D], gi[..., 2 * D:]
  assert float(pre_rz.max()) > 100.0 and float(pre_rz.min()) < -100.0
  assert float(pre_n.max()) > 100.0 and float(pre_n.min()) < -100.0
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(12))
  truth = GM.propagate_autograd(Sd, dST.double(), Ld, Wd[:8], steps, 'avg')
  e32 = GM.propagate_e32(S, dST, L, W[:8], truth, steps, 'avg')
  got, _ = _hip_backward(S, dST, L.cuda(), W, steps, 'avg')
  _hold('saturated gates', got, truth, e32, 'avg')


def test_degree_zero_rows_an_empty_channel_and_any_nonzero_entry_counts_as_an_edge():
  N, C, D, B, steps = 9, 3, 32, 4, 2
  S, L, W = GM.draw_operands(92, B, N, C, D)
  L[0, 2] = 0.0                                                # a row without an edge in every channel
  L[1, :, :, 1] = 0.0                                          # a whole channel without an edge
  L[2, 3, 4, 0], L[2, 4, 3, 2], L[3, 0, 0, 1] = -0.5, float('nan'), float('nan')
  ones = (torch.isnan(L) | (L != 0)).float()                   # what `L != 0` says
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(13))
  d = lambda x: x.double()  # noqa: E731
  for agg in ('avg', 'sum'):
    Ld = L.cuda()
    bits = Ld.clone().view(torch.int32)
    got, _ = _hip_backward(S, dST, Ld, W, steps, agg)
    assert torch.equal(Ld.view(torch.int32), bits)             # bit-identical before and after
    truth = GM.propagate_autograd(d(S), d(dST), d(ones), [d(w) for w in W[:8]], steps, agg)
    e32 = GM.propagate_e32(S, dST, ones, W[:8], truth, steps, agg)
    _hold('degree-0 / NaN entries %s' % agg, got, truth, e32, agg)


def _mask(kind, B, N, seed):
  if kind is None:
    return None
  g = torch.Generator().manual_seed(seed)
  n = torch.randint(1, N + 1, (B,), generator=g) if kind == 'ragged' else torch.ones(B, dtype=torch.long)
  return (torch.arange(N).unsqueeze(0) < n.unsqueeze(1)).to(torch.uint8)


# (N, D, P, mask, B, row padding)
READOUT_CASES = [
    (1, 32, 1, None, 1, 0),
    (17, 96, 16, 'ragged', 5, 4),
    (32, 128, 16, 'one', 5, 0),
    (32, 128, 1, 'ragged', 1, 8),
    (17, 32, 16, None, 5, 0),
]


@pytest.mark.parametrize('N,D,P,mkind,B,pad', READOUT_CASES)
def test_ggnn_readout_backward_matches_float64_autograd(N, D, P, mkind, B, pad):
  from lanczosnet_amd import ops
  S, _, W = GM.draw_operands(5000 + N + D + P, B, N, 1, D, P=P)
  head = W[8:]
  mask = _mask(mkind, B, N, 23 + N)
  dscore = torch.randn(B, P, generator=torch.Generator().manual_seed(14))
  d = lambda x: x.double()  # noqa: E731
  truth = GM.readout_autograd(d(S), mask, *[d(w) for w in head], d(dscore))
  e32 = GM.readout_e32(S, mask, *head, dscore, truth)
  Sv, _ = _padded(S, pad)
  out, outbuf = _padded(torch.zeros(B, N, D), pad)
  got = ops.ggnn_readout_backward(Sv, None if mask is None else mask.cuda(), *[w.cuda() for w in head],
                                  dscore.cuda(), dSlast=out)
  for name, x, t, e in zip(GM.RO_NAMES, got, truth, e32):
    x = x.double().cpu().reshape(t.shape)
    err, bar = float((x - t).abs().max()) / float(t.abs().max()), max(4.0 * e, 4.0 * ULP)
    print('ggnn readout backward N %d D %d P %d %s: %.2e of the scale, float32 reference %.2e, bar %.2e'
          % (N, D, P, name, err, e, bar))
    assert torch.isfinite(x).all() and err <= bar, name
  if mask is not None:
    outside = got[0].cpu()[mask == 0]
    assert outside.numel() == 0 or float(outside.abs().max()) == 0.0     # an exact 0 outside the mask
  if pad:
    assert torch.isnan(outbuf[:, :, D:]).all()
  again = ops.ggnn_readout_backward(Sv, None if mask is None else mask.cuda(), *[w.cuda() for w in head], dscore.cuda())
  assert all(torch.equal(a, b) for a, b in zip(got, again))              # the same bits from call to call


def test_the_ops_are_bitwise_reproducible_and_the_raw_ops_give_the_same_bits():
  from lanczosnet_amd import ops
  N, C, D, B, P = 13, 3, 64, 5, 16
  S, L, W = GM.draw_operands(94, B, N, C, D)
  Sd, Ld, Wd = S.cuda(), L.cuda(), [w.cuda() for w in W]
  dSn = torch.randn(B, N, D, generator=torch.Generator().manual_seed(15)).cuda()
  tr = ops.ggnn_pack_transposes(Wd[0], Wd[2], Wd[4], Wd[6])
  d1, b1 = ops.ggnn_backward_step(Sd, dSn, Ld, *Wd[:8], transposes=tr, avg=True)
  d2, b2 = ops.ggnn_backward_step(Sd, dSn, Ld, *Wd[:8], avg=True)       # packs the transposes itself
  assert torch.equal(d1, d2) and all(torch.equal(x, y) for x, y in zip(b1, b2))
  raw = [torch.full_like(x, float('nan')) for x in (d1,) + tuple(b1)]
  torch.ops.lanczosnet.raw_ggnn_backward_step(Sd, D, dSn, D, Ld, Ld.stride(0), Ld.stride(1), Ld.stride(2), Ld.stride(3),
                                              *Wd[:8], *tr, B, N, C, D, 1, raw[0], D, *raw[1:])
  assert all(torch.equal(x, y) for x, y in zip(raw, (d1,) + tuple(b1)))
  g1 = ops.ggnn_step_weight_grads(Sd, b1, C)
  g2 = ops.ggnn_step_weight_grads(Sd, b2, C)
  assert all(torch.equal(x, y) for x, y in zip(g1, g2))
  dscore = torch.randn(B, P, generator=torch.Generator().manual_seed(16)).cuda()
  mask = _mask('ragged', B, N, 5).cuda()
  r1 = ops.ggnn_readout_backward(Sd, mask, *Wd[8:], dscore)
  rr = [torch.full_like(x, float('nan')) for x in r1]
  ws = torch.empty(B * (P * D + P + D + 1), device='cuda')
  torch.ops.lanczosnet.raw_ggnn_readout_backward(Sd, D, mask, Wd[8], Wd[9], Wd[10].reshape(-1), Wd[11], dscore, B, N, D,
                                                 P, ws, rr[0], D, rr[1], rr[2], rr[3], rr[4])
  assert all(torch.equal(x, y) for x, y in zip(rr, r1))


@pytest.mark.parametrize('N,C,D,B,steps,tile', [(5, 2, 32, 3, 2, 0), (31, 7, 128, 5, 3, 64), (17, 2, 64, 4, 15, 32),
                                                 (8, 1, 96, 2, 0, 0), (5, 3, 96, 14, 3, 64), (11, 2, 64, 7, 3, 32)])
def test_forward_states_has_the_bits_of_the_forward_and_leaves_the_trajectory(N, C, D, B, steps, tile):
  from lanczosnet_amd import ops
  S, L, W = GM.draw_operands(97 + N, B, N, C, D)
  Sd, Ld, Wd = S.cuda(), L.cuda(), [w.cuda() for w in W]
  mask = _mask('ragged', B, N, 6).cuda()
  score, final = ops.ggnn_forward(Sd, Ld, mask, *Wd, steps, avg=True, return_state=True, tile_rows=tile)
  s2, states = ops.ggnn_forward_states(Sd, Ld, mask, *Wd, steps, avg=True, tile_rows=tile)
  if tile:
    assert ops.last_kernel() == 'ggnn_forward_kernel<%d, %d>' % (D, tile // 16)
  assert tuple(states.shape) == (steps + 1, B, N, D)
  assert torch.equal(s2, score) and torch.equal(states[steps], final) and torch.equal(states[0], Sd)
  for t in range(steps):   # every S_t is the state after t steps of the forward
    assert torch.equal(states[t + 1], ops.ggnn_forward(states[t], Ld, mask, *Wd, 1, avg=True, return_state=True)[1])
  raw_s = torch.empty_like(score)
  raw_states = torch.full_like(states, float('nan'))
  torch.ops.lanczosnet.raw_ggnn_forward_states(Sd, D, Ld, Ld.stride(0), Ld.stride(1), Ld.stride(2), Ld.stride(3), mask,
                                               *Wd[:10], Wd[10].reshape(-1), Wd[11], B, N, C, D, 16, steps, 1, raw_s,
                                               None, D, raw_states, tile)
  assert torch.equal(raw_s, score) and torch.equal(raw_states, states)


def test_out_of_envelope_arguments_raise():
  from lanczosnet_amd import ops
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def operands(C, D, P):
    return [z(C, 128, D), z(C, 128), z(C, D, 128), z(C, D), z(3 * D, C * D), z(3 * D), z(3 * D, D), z(3 * D),
            z(P, D), z(P), z(1, D), z(1)]

  def step(N=8, C=2, D=32, S=None, short=False):
    W = operands(C, D, 16)[:8]
    if short:
      W[3] = z(C, D - 1)
    return ops.ggnn_backward_step(z(1, N, D) if S is None else S, z(1, N, D), z(1, N, N, C), *W)

  def readout(N=8, D=32, P=16, S=None, short=False):
    W = operands(1, D, P)[8:]
    if short:
      W[1] = z(P - 1) if P > 1 else z(2)
    return ops.ggnn_readout_backward(z(1, N, D) if S is None else S, None, *W, z(1, P))

  def states(N=8, C=2, D=32, P=16, steps=1, S=None):
    return ops.ggnn_forward_states(z(1, N, D) if S is None else S, z(1, N, N, C), None, *operands(C, D, P), steps)
  step(), readout(), states()
  for kw in (dict(N=33), dict(C=9), dict(D=48), dict(D=160)):
    with pytest.raises(ops.NotSupported):
      step(**kw)
    with pytest.raises(ops.NotSupported):
      states(**kw)
  for kw in (dict(N=33), dict(D=48), dict(D=160), dict(P=17)):
    with pytest.raises(ops.NotSupported):
      readout(**kw)
  with pytest.raises(ops.NotSupported):
    states(P=17)
  with pytest.raises(ops.NotSupported):
    states(steps=-1)
  for fn in (step, states):
    with pytest.raises(ops.NotSupported):
      fn(S=z(1, 8, 36)[:, :, 2:34])                            # rows not 16-byte aligned
  for fn in (step, readout):
    with pytest.raises(ops.LnzError):
      fn(short=True)                                           # a short operand
  for fn in (step, readout, states):
    with pytest.raises(RuntimeError):
      fn(S=torch.zeros(1, 8, 32))                              # a host tensor


# ------------------------------------------------------------------------------------------ module
def _net(name, g, switch='hip', **over):
  from lanczosnet_amd.model import GGNN
  cfg, batch, use_mask = G.case_inputs(name)
  if over:
    cfg = G.make_config(**dict(G.CASES[name][0], **over))
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])
  net = GGNN(cfg)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net.ggnn_backward_impl = switch
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  d = {k: t(v) for k, v in batch.items()}
  if not use_mask:
    d['node_mask'] = None
  return net.cuda(), cfg, batch, P, d, use_mask


@functools.lru_cache(maxsize=None)
def _net_truth(name):
  g = load_golden('ggnn.npz')
  cfg, batch, use_mask = G.case_inputs(name)
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])
  truth, _ = GM.net_gradients(P, cfg, batch, torch.float64, use_mask)
  return truth, GM.net_e32(P, cfg, batch, truth, use_mask)


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_ggnn_module_trains_on_the_hip_route_and_matches_the_reference_gradients(name):
  g = load_golden('ggnn.npz')
  net, cfg, batch, P, d, use_mask = _net(name, g)
  net.train()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
    first = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
  assert net.last_route == 'ggnn_hip_train' and not [w for w in rec if 'lanczosnet_amd' in str(w.message)]
  assert abs(float(loss.detach()) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))
  gd = dict(net.named_parameters())
  for k, gs, ga in zip(g[name + '_names'], g[name + '_gsum'], g[name + '_gabs']):
    gr = gd[str(k)].grad
    assert gr is not None, k
    assert torch.equal(gr, first[str(k)]), k                              # bitwise from pass to pass
    tol = 2e-4 * float(ga) + 1e-9
    assert abs(float(gr.double().sum()) - float(gs)) < tol, (k, float(gr.double().sum()), float(gs))
    assert abs(float(gr.double().abs().sum()) - float(ga)) < tol, k
  # the score has the bits of the inference route
  net.eval()
  with torch.no_grad():
    inf = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'ggnn_hip' and torch.equal(inf, score.detach())
  truth, e32 = _net_truth(name)
  for k, t in truth.items():
    x = gd[k].grad.double().cpu()
    scale = float(t.abs().max())
    err, bar = float((x - t).abs().max()) / scale, max(1e-5, 4.0 * e32[k])
    print('GGNN case %s %s: ggnn_hip_train vs float64 autograd %.2e (float32 autograd %.2e, bar %.2e)'
          % (name, k, err, e32[k], bar))
    assert err <= bar, k


def test_one_adam_step_moves_both_routes_equally():
  g = load_golden('ggnn.npz')
  after = {}
  for switch in ('torch', 'hip'):
    net, cfg, batch, P, d, _ = _net('c', g, switch=switch)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      _, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    assert net.last_route == ('ggnn_hip_train' if switch == 'hip' else 'ggnn_torch')
    loss.backward()
    opt.step()
    net.eval()
    with torch.no_grad():
      after[switch] = net(d['node_feat'], d['L'], mask=d['node_mask'])
    assert net.last_route == 'ggnn_hip'                                   # the packed operands followed the step
  scale = float(after['torch'].abs().max())
  assert float((after['hip'] - after['torch']).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize('switch', ['torch', 'hip'])
def test_dropout_and_the_rnn_update_still_take_the_torch_route(switch):
  g = load_golden('ggnn.npz')
  for name, over, reason in (('c', dict(dropout=0.5), 'dropout'), ('e', {}, 'RNN update' if switch == 'hip' else 'gradients')):
    net, cfg, batch, P, d, _ = _net(name, g, switch=switch, **over)
    net.train()
    with warnings.catch_warnings(record=True) as rec:
      warnings.simplefilter('always')
      for _ in range(2):
        _, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
        loss.backward()
    mine = [w for w in rec if issubclass(w.category, UserWarning) and 'ggnn_torch' in str(w.message)]
    assert net.last_route == 'ggnn_torch' and len(mine) == 1
    if switch == 'hip' or name == 'e':
      assert reason in str(mine[0].message)


def test_without_propagation_steps_only_the_readout_and_the_input_train():
  g = load_golden('ggnn.npz')
  net, cfg, batch, P, d, use_mask = _net('c', g, num_prop=0)
  net.train()
  _, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  loss.backward()
  assert net.last_route == 'ggnn_hip_train'
  truth, _ = GM.net_gradients(P, cfg, batch, torch.float64, use_mask)
  e32 = GM.net_e32(P, cfg, batch, truth, use_mask)
  for k, p in net.named_parameters():
    if k.startswith('update_func') or k.startswith('msg_func'):
      assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
      assert truth[k] is None or float(truth[k].abs().max()) == 0.0
    else:
      t = truth[k]
      err = float((p.grad.double().cpu() - t).abs().max()) / float(t.abs().max())
      assert err <= max(1e-5, 4.0 * e32[k]), k
