"""GPU: the MPNN propagation backward (csrc/mpnn_grad.hip, the trajectory entry of csrc/mpnn.hip) against
float64 autograd through tests/mpnn_mirror.py, and route 'mpnn_hip_train' of the module against the reference's
own numbers in tests/golden/mpnn.npz.

Bar of the kernel-level cases: truth is float64 autograd (mpnn_grad_mirror.propagate_autograd); e32 is the error
of the CPU float32 autograd of the same formula, the largest of eight evaluations (the inputs as given and seven
with molecules, nodes and channel order consistently permuted), per gradient tensor in units of max|truth|.  The
kernel has to be within max(K e32, 4 * 2^-23) max|truth| per gradient tensor; where the truth is identically zero
the kernel's gradient is exactly 0.  K starts at the project's 4: another summation order draws another sample
of the same rounding.  Measured before relying on it (CPU, tools/mpnn_grad_reference_spread.py: the cases of
mpnn_grad_mirror.STEP_CASES with their seeds, the spread worst / best e32 of the eight evaluations per gradient
tensor, the largest over the nine tensors of a case): see SPREAD below.  The kernel's own output never enters
the bar.  Every kernel-level case is kink-free (mpnn_grad_mirror's header; tests/test_mpnn_train_cpu.py asserts
it for every draw used here): no edge pre-activation is close enough to zero for float32 to land on the other
side of a ReLU.
Module level: the fixture's loss to 1e-5, its _gsum / _gabs to 2e-4 gabs + 1e-9, and for cases c and f per
parameter max(1e-5, 4 e32) max|truth| against float64 autograd of the whole net."""
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import mpnn_grad_mirror as GM
import mpnn_mirror as M

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
# SPREAD: measured on the CPU over STEP_CASES (worst / best e32 of the eight evaluations, largest over the nine
# gradient tensors of a case; e32 itself 6e-8 .. 8e-6): 'avg' 1.55 .. 2.37 (2.37 at N 5: dbhh, 1.82 at N 16,
# 1.89 at N 31, 1.55 at N 32, 1.91 at N 5, D 96) — below 4, so K stays at the project's 4; 'sum' 1.00 .. 6.16
# (1.00 at N 1, 6.16 at N 17, D 64, 3 steps: dWih, 3.68 at N 32, D 96: dS, 3.26 at N 11: dS) — above 4, so K for
# 'sum' is the measured 6.16.
K = {'avg': 4.0, 'sum': 6.16}


@functools.lru_cache(maxsize=None)
def _step_truth(N, C, D, B, steps, agg, lkind):
  """(truth: the nine float64 gradients, e32: nine numbers) — computed once, shared, never changed"""
  S, L, W, dST = GM.step_case_inputs(N, C, D, B, steps, agg, lkind)
  d = lambda x: x.double()  # noqa: E731
  truth = GM.propagate_autograd(d(S), d(dST), d(L), [d(w) for w in W], steps, agg)
  e32 = GM.propagate_e32(S, dST, L, W, truth, steps, agg)
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
  states = ops.mpnn_forward_states(S.cuda(), Ld, *Wd, steps, avg=avg)
  tr = ops.mpnn_pack_transposes(Wd[0], Wd[2], Wd[4], Wd[6])
  bufs = ops.mpnn_step_buffers(B, N, C, D, 'cuda')
  deg = ops.mpnn_edge_degrees(Ld)
  dS, buf_a = _padded(dST, pad)
  spare, buf_b = _padded(torch.zeros(B, N, D), pad)
  grads = [torch.zeros_like(w) for w in Wd]
  for t in range(steps - 1, -1, -1):
    St, _ = _padded(states[t], pad)
    spare, _ = ops.mpnn_backward_step(St, dS, Ld, *Wd, transposes=tr, avg=avg, dS=spare, buffers=bufs)
    assert ops.last_kernel() == 'mpnn_backward_step_kernel<%d>' % D
    dS, spare = spare, dS
    grads = ops.mpnn_step_weight_grads(St, bufs, C, deg, grads)
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
    print('mpnn backward %s %s: %.2e of the scale, float32 reference %.2e, bar %.2e' % (tag, name, err, e, bar))
    assert err <= bar, name


@pytest.mark.parametrize('N,C,D,B,steps,agg,pad,lkind', GM.STEP_CASES)
def test_mpnn_backward_steps_match_float64_autograd(N, C, D, B, steps, agg, pad, lkind):
  S, L, W, dST = GM.step_case_inputs(N, C, D, B, steps, agg, lkind)
  if N == 32 and C == 8:
    assert int((L[0, 0, :, 0] != 0).sum()) == 32                  # the row with all 32 bits set
    assert float((L != 0).float().mean()) <= 0.05
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
  assert torch.equal(Ld.view(torch.int32), before.view(torch.int32))   # L is read, never written
  truth, e32 = _step_truth(N, C, D, B, steps, agg, lkind)
  _hold('N %d C %d D %d B %d steps %d %s' % (N, C, D, B, steps, agg), got, truth, e32, agg)
  if pad:
    for b in bufs:
      assert torch.isnan(b[:, :, D:]).all()                       # nothing written beyond the width


@pytest.mark.parametrize('N,C,D,B,steps,tile', [(5, 2, 32, 3, 2, 32), (31, 7, 128, 5, 3, 64), (17, 2, 64, 4, 7, 32),
                                                 (8, 1, 96, 2, 0, 0), (5, 3, 96, 14, 3, 64), (11, 2, 64, 7, 3, 32),
                                                 (32, 8, 128, 3, 2, 64), (32, 8, 128, 3, 2, 32)])
def test_forward_states_has_the_bits_of_the_forward_and_leaves_the_trajectory(N, C, D, B, steps, tile):
  from lanczosnet_amd import ops
  S, L, W = GM.draw_operands(97 + N, B, N, C, D)
  Sd, Ld, Wd = S.cuda(), L.cuda(), [w.cuda() for w in W]
  final = ops.mpnn_forward(Sd, Ld, *Wd, steps, avg=True, tile_rows=tile)
  states = ops.mpnn_forward_states(Sd, Ld, *Wd, steps, avg=True, tile_rows=tile)
  if tile:
    assert ops.last_kernel() == 'mpnn_forward_states_kernel<%d, %d>' % (D, tile // 16)
  assert tuple(states.shape) == (steps + 1, B, N, D)
  assert torch.equal(states[steps], final) and torch.equal(states[0], Sd)
  for other in (32, 64):   # ... at both tile heights
    assert torch.equal(ops.mpnn_forward_states(Sd, Ld, *Wd, steps, avg=True, tile_rows=other)[steps], final)
  for t in range(steps):   # every S_t is the state after t steps of the forward
    assert torch.equal(states[t + 1], ops.mpnn_forward(states[t], Ld, *Wd, 1, avg=True))
  raw_states = torch.full_like(states, float('nan'))
  raw_out = torch.full_like(final, float('nan'))
  torch.ops.lanczosnet.raw_mpnn_forward_states(Sd, D, Ld, Ld.stride(0), Ld.stride(1), Ld.stride(2), Ld.stride(3),
                                               *Wd, B, N, C, D, steps, 1, raw_out, D, raw_states, tile)
  assert torch.equal(raw_states, states) and torch.equal(raw_out, final)


def test_saturated_gates_give_finite_gradients_within_the_bar():
  """the forward test's construction: weights scaled until the gate pre-activations pass +-100"""
  S, L, W, dST, pre_rz, pre_n = GM.saturated_case()
  steps = GM.SATURATED_DRAW[5]
  assert float(pre_rz.max()) > 100.0 and float(pre_rz.min()) < -100.0
  assert float(pre_n.max()) > 100.0 and float(pre_n.min()) < -100.0
  d = lambda x: x.double()  # noqa: E731
  truth = GM.propagate_autograd(d(S), d(dST), d(L), [d(w) for w in W], steps, 'avg')
  e32 = GM.propagate_e32(S, dST, L, W, truth, steps, 'avg')
  got, _ = _hip_backward(S, dST, L.cuda(), W, steps, 'avg')
  _hold('saturated gates', got, truth, e32, 'avg')


def test_degree_zero_rows_an_empty_channel_and_any_nonzero_entry_counts_as_an_edge():
  S, L, ones, W, dST = GM.edge_case()
  steps = GM.EDGE_DRAW[5]
  assert bool(torch.isnan(L).any()) and bool((L < 0).any())
  d = lambda x: x.double()  # noqa: E731
  for agg in ('avg', 'sum'):
    Ld = L.cuda()
    bits = Ld.clone().view(torch.int32)
    got, _ = _hip_backward(S, dST, Ld, W, steps, agg)
    assert torch.equal(Ld.view(torch.int32), bits)             # bit-identical before and after
    truth = GM.propagate_autograd(d(S), d(dST), d(ones), [d(w) for w in W], steps, agg)
    e32 = GM.propagate_e32(S, dST, ones, W, truth, steps, agg)
    _hold('degree-0 / NaN entries %s' % agg, got, truth, e32, agg)


def test_the_ops_are_bitwise_reproducible_and_the_raw_op_gives_the_same_bits():
  from lanczosnet_amd import ops
  seed, N, C, D, B, _, density = GM.REPEAT_DRAW
  S, L, W = GM.draw_operands(seed, B, N, C, D, density=density)
  Sd, Ld, Wd = S.cuda(), L.cuda(), [w.cuda() for w in W]
  dSn = torch.randn(B, N, D, generator=torch.Generator().manual_seed(15)).cuda()
  tr = ops.mpnn_pack_transposes(Wd[0], Wd[2], Wd[4], Wd[6])
  d1, b1 = ops.mpnn_backward_step(Sd, dSn, Ld, *Wd, transposes=tr, avg=True)
  d2, b2 = ops.mpnn_backward_step(Sd, dSn, Ld, *Wd, avg=True)         # packs the transposes itself
  assert torch.equal(d1, d2) and all(torch.equal(x, y) for x, y in zip(b1, b2))
  raw = [torch.full_like(x, float('nan')) for x in (d1,) + tuple(b1)]
  torch.ops.lanczosnet.raw_mpnn_backward_step(Sd, D, dSn, D, Ld, Ld.stride(0), Ld.stride(1), Ld.stride(2), Ld.stride(3),
                                              *Wd, *tr, B, N, C, D, 1, raw[0], D, *raw[1:])
  assert all(torch.equal(x, y) for x, y in zip(raw, (d1,) + tuple(b1)))
  deg = ops.mpnn_edge_degrees(Ld)
  g1 = ops.mpnn_step_weight_grads(Sd, b1, C, deg)
  g2 = ops.mpnn_step_weight_grads(Sd, b2, C, deg)
  assert all(torch.equal(x, y) for x, y in zip(g1, g2))


def test_out_of_envelope_arguments_raise():
  from lanczosnet_amd import ops
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def operands(C, D):
    return [z(C, 64, 2 * D), z(C, 64), z(C, D, 64), z(C, D), z(3 * D, C * D), z(3 * D), z(3 * D, D), z(3 * D)]

  def step(N=8, C=2, D=32, S=None, short=False):
    W = operands(C, D)
    if short:
      W[3] = z(C, D - 1)
    return ops.mpnn_backward_step(z(1, N, D) if S is None else S, z(1, N, D), z(1, N, N, C), *W)

  def states(N=8, C=2, D=32, steps=1, S=None, short=False):
    W = operands(C, D)
    if short:
      W[0] = z(C, 64, D)
    return ops.mpnn_forward_states(z(1, N, D) if S is None else S, z(1, N, N, C), *W, steps)
  step(), states()
  for kw in (dict(N=33), dict(C=9), dict(D=48), dict(D=160)):
    with pytest.raises(ops.NotSupported):
      step(**kw)
    with pytest.raises(ops.NotSupported):
      states(**kw)
  with pytest.raises(ops.NotSupported):
    states(steps=-1)
  for fn in (step, states):
    with pytest.raises(ops.NotSupported):
      fn(S=z(1, 8, 36)[:, :, 2:34])                            # rows not 16-byte aligned
    with pytest.raises(ops.LnzError):
      fn(short=True)                                           # a short operand
    with pytest.raises(RuntimeError):
      fn(S=torch.zeros(1, 8, 32))                              # a host tensor


# ------------------------------------------------------------------------------------------ module
def _net(name, g, switch='hip', **over):
  from lanczosnet_amd.model import MPNN
  cfg, batch, use_mask = M.case_inputs(name)
  if over:
    cfg = M.make_config(**dict(M.CASES[name][0], **over))
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = M.draw_params(zip([str(k) for k in g[name + '_names']], shapes), M.PARAM_SEED[name])
  net = MPNN(cfg)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net.mpnn_backward_impl = switch
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  d = {k: t(v) for k, v in batch.items()}
  if not use_mask:
    d['node_mask'] = None
  return net.cuda(), cfg, batch, P, d, use_mask


@functools.lru_cache(maxsize=None)
def _net_truth(name):
  g = load_golden('mpnn.npz')
  cfg, batch, use_mask = M.case_inputs(name)
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = M.draw_params(zip([str(k) for k in g[name + '_names']], shapes), M.PARAM_SEED[name])
  truth, _ = GM.net_gradients(P, cfg, batch, torch.float64, use_mask)
  return truth, GM.net_e32(P, cfg, batch, truth, use_mask)


@pytest.mark.parametrize('name', ['b', 'c', 'd', 'f'])
def test_mpnn_module_trains_on_the_hip_route_and_matches_the_reference_gradients(name):
  g = load_golden('mpnn.npz')
  net, cfg, batch, P, d, use_mask = _net(name, g)
  net.train()
  Lbits = d['L'].clone()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
    first = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
  assert net.last_route == 'mpnn_hip_train' and not [w for w in rec if 'lanczosnet_amd' in str(w.message)]
  assert torch.equal(d['L'], Lbits)
  assert abs(float(loss.detach()) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))
  gd = dict(net.named_parameters())
  for k, gs, ga in zip(g[name + '_names'], g[name + '_gsum'], g[name + '_gabs']):
    gr = gd[str(k)].grad
    assert gr is not None, k
    assert torch.equal(gr, first[str(k)]), k                              # bitwise from pass to pass
    tol = 2e-4 * float(ga) + 1e-9
    assert abs(float(gr.double().sum()) - float(gs)) < tol, (k, float(gr.double().sum()), float(gs))
    assert abs(float(gr.double().abs().sum()) - float(ga)) < tol, k
  if name not in ('c', 'f'):
    return
  truth, e32 = _net_truth(name)
  for k, t in truth.items():
    x = gd[k].grad.double().cpu()
    scale = float(t.abs().max())
    err, bar = float((x - t).abs().max()) / scale, max(1e-5, 4.0 * e32[k])
    print('MPNN case %s %s: mpnn_hip_train vs float64 autograd %.2e (float32 autograd %.2e, bar %.2e)'
          % (name, k, err, e32[k], bar))
    assert err <= bar, k


@pytest.mark.parametrize('switch', ['torch', 'hip'])
def test_the_edge_embedding_and_dropout_still_take_the_torch_route(switch):
  g = load_golden('mpnn.npz')
  for name, over, reason in (('c', dict(dropout=0.5), 'dropout'),
                             ('e', {}, 'edge embedding' if switch == 'hip' else 'gradients')):
    net, cfg, batch, P, d, _ = _net(name, g, switch=switch, **over)
    net.train()
    with warnings.catch_warnings(record=True) as rec:
      warnings.simplefilter('always')
      for _ in range(2):
        _, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
        loss.backward()
    mine = [w for w in rec if issubclass(w.category, UserWarning) and 'mpnn_torch' in str(w.message)]
    assert net.last_route == 'mpnn_torch' and len(mine) == 1
    if switch == 'hip' or name == 'e':
      assert reason in str(mine[0].message)


def test_the_switch_off_takes_the_torch_route_and_an_optimizer_step_invalidates_the_transposes():
  g = load_golden('mpnn.npz')
  net, cfg, batch, P, d, _ = _net('c', g, switch='torch')
  net.train()
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    _, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  assert net.last_route == 'mpnn_torch' and net._transpose_cache is None
  after = {}
  for switch in ('torch', 'hip'):
    net, cfg, batch, P, d, _ = _net('c', g, switch=switch)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      _, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    assert net.last_route == ('mpnn_hip_train' if switch == 'hip' else 'mpnn_torch')
    loss.backward()
    if switch == 'hip':
      old = net._transposes()
      assert net._transposes() is old                                   # cached per weight version
    opt.step()
    if switch == 'hip':
      new = net._transposes()
      assert new is not old and not torch.equal(new[0], old[0])         # the step dropped the packs
      W1 = torch.stack([f[0].weight for f in net.edge_func]).detach()
      assert torch.equal(new[0][:, 0], W1[:, :, :cfg.model.hidden_dim].transpose(1, 2))
      assert torch.equal(new[0][:, 1], W1[:, :, cfg.model.hidden_dim:].transpose(1, 2))
    net.eval()
    with torch.no_grad():
      after[switch] = net(d['node_feat'], d['L'], mask=d['node_mask'])
    assert net.last_route == 'mpnn_hip'                                 # the packed operands followed the step
  scale = float(after['torch'].abs().max())
  assert float((after['hip'] - after['torch']).abs().max()) <= 1e-5 * scale


def test_without_propagation_steps_only_the_readout_and_the_input_train():
  g = load_golden('mpnn.npz')
  net, cfg, batch, P, d, use_mask = _net('c', g, num_prop=0)
  net.train()
  _, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  loss.backward()
  assert net.last_route == 'mpnn_hip_train'
  truth, _ = GM.net_gradients(P, cfg, batch, torch.float64, use_mask)
  e32 = GM.net_e32(P, cfg, batch, truth, use_mask)
  for k, p in net.named_parameters():
    if k.startswith('update_func') or k.startswith('edge_func'):
      assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
      assert truth[k] is None or float(truth[k].abs().max()) == 0.0
    else:
      t = truth[k]
      err = float((p.grad.double().cpu() - t).abs().max()) / float(t.abs().max())
      assert err <= max(1e-5, 4.0 * e32[k]), k
