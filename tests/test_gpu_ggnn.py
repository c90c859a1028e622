"""GPU: the fused GGNN kernel (csrc/ggnn.hip) against the float64 restatement of tests/ggnn_mirror.py,
and the module's two routes against the reference's own numbers in tests/golden/ggnn.npz.

Bar of the kernel-level cases: the reference arithmetic is the CPU float32 torch evaluation of the
same formula on the same inputs; its error e32 against float64 is measured at run time and the
kernel's final state and score each have to be within max(K e32, 4 fp32 ulps) max|ref64| of float64.
K starts at the project's 4: another summation order draws another sample of the same rounding.
Measured before relying on it (CPU, the float32 mirror with one-ulp-perturbed operands and permuted
channel order against float64, eight runs per shape, the eight shapes below (B <= 9) at num_prop 1 and
15, each with 'avg' and with 'sum'), worst / best e32 of the eight runs: 'avg' 1.1 .. 2.8 (worst: N 5,
C 2, D 32, 15 steps; e32 itself 1e-7 .. 6e-7), so K = 4 holds for 'avg'; 'sum' 1.2 .. 2.6 at one step
but 1.9 .. 10.5 at 15 steps (7.9 at N 31, C 2, D 32; 10.5 at N 32, C 1, D 96; e32 up to 5.9e-5: an
unnormalised sum over up to 32 neighbours grows the state's sensitivity step by step), so for 'sum'
K is that measured spread, 10.5.  tools/ggnn_reference_spread.py (CPU only) re-measures these figures from
this file's own operand draws, the thirteen shapes below, state and score: 'avg' 1.2 .. 2.9, 'sum' at a
shape's own num_prop 1.3 .. 5.7 and at 15 steps up to 7.2 (N 32, C 1, D 96) and 13.1 (the score at N 31, C 2,
D 32, which the test runs at 2 steps: 4.0); the five rows with several molecules per tile give 'avg' <= 2.9
and 'sum' <= 4.6.  The figure of a 15-step 'sum' moves with the draws; K stays at 10.5, the lower of the two
measurements and so the stricter bar.  The kernel's own output never enters the bar.
Module level: max(1e-5, 4 e_ref) max|s64| with e_ref read from the fixture."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import ggnn_mirror as G

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
K = {'avg': 4.0, 'sum': 10.5}   # measured spread of the reference arithmetic, see above


def _bar(got, ref32, ref64, agg):
  scale = float(ref64.abs().max())
  e32 = float((ref32.double() - ref64).abs().max()) / scale
  err = float((got.double().cpu() - ref64).abs().max()) / scale
  return err, e32, max(K[agg] * e32, 4.0 * ULP)


def _operands(seed, B, N, C, D, P=16, scale=1.0, density=0.3):
  """(state0, L, the twelve operands): Xavier-bounded weights, biases +-0.1, a sparse L with negative
  entries (only != 0 matters)"""
  g = torch.Generator().manual_seed(seed)
  u = lambda bound, *s: (torch.rand(*s, generator=g) * 2 - 1) * bound  # noqa: E731
  xav = lambda *s: u(scale * float(np.sqrt(6.0 / (s[-1] + s[-2]))), *s)  # noqa: E731
  S = 0.5 * torch.randn(B, N, D, generator=g)
  L = (torch.rand(B, N, N, C, generator=g) < density).float() * (torch.rand(B, N, N, C, generator=g) - 0.5)
  W = [xav(C, G.HIDDEN, D), u(0.1, C, G.HIDDEN), xav(C, D, G.HIDDEN), u(0.1, C, D), xav(3 * D, C * D), u(0.1, 3 * D),
       xav(3 * D, D), u(0.1, 3 * D), xav(P, D), u(0.1, P), xav(1, D), u(0.1, 1)]
  return S, L, W


def _mask(kind, B, N, seed):
  if kind is None:
    return None
  g = torch.Generator().manual_seed(seed)
  n = torch.randint(1, N + 1, (B,), generator=g) if kind == 'ragged' else torch.ones(B, dtype=torch.long)
  return (torch.arange(N).unsqueeze(0) < n.unsqueeze(1)).to(torch.uint8)


def _padded(x, pad):
  """x [B, N, W] as a view of a [B, N, W + pad] device buffer filled with NaN beyond the width"""
  buf = torch.full(x.shape[:2] + (x.shape[2] + pad,), float('nan'), device='cuda')
  buf[:, :, :x.shape[2]] = x.cuda()
  return buf[:, :, :x.shape[2]]


def _mirror(S, L, W, mask, num_prop, agg, dtype):
  c = lambda x: x.to(dtype)  # noqa: E731
  Sf = G.propagate(c(S), c(L), *[c(w) for w in W[:8]], num_prop, agg=agg)
  return Sf, G.readout(Sf, mask, *[c(w) for w in W[8:]])


def _run(S, L, W, mask, num_prop, agg, Ld=None, pad=0, tile_rows=0):
  from lanczosnet_amd import ops
  B, N, D = S.shape
  outbuf = torch.full((B, N, D + pad), float('nan'), device='cuda')
  score, state = ops.ggnn_forward(_padded(S, pad), L.cuda() if Ld is None else Ld, None if mask is None else mask.cuda(),
                                  *[w.cuda() for w in W], num_prop, avg=agg == 'avg', state_out=outbuf[:, :, :D],
                                  tile_rows=tile_rows)
  return score, state, outbuf


def _check(tag, S, L, W, mask, num_prop, agg, **kw):
  from lanczosnet_amd import ops
  score, state, outbuf = _run(S, L, W, mask, num_prop, agg, tile_rows=64, **kw)
  assert ops.last_kernel() == 'ggnn_forward_kernel<%d, 4>' % S.shape[2]
  score32, state32, _ = _run(S, L, W, mask, num_prop, agg, tile_rows=32, **kw)
  assert ops.last_kernel() == 'ggnn_forward_kernel<%d, 2>' % S.shape[2]
  assert torch.equal(score32, score) and torch.equal(state32, state)   # a row's bits do not depend on the tile height
  s32, y32 = _mirror(S, L, W, mask, num_prop, agg, torch.float32)
  s64, y64 = _mirror(S, L, W, mask, num_prop, agg, torch.float64)
  for what, got, r32, r64 in (('state', state, s32, s64), ('score', score, y32, y64)):
    err, e32, bar = _bar(got, r32, r64, agg)
    print('ggnn_forward %s %s: %.2e of the scale, float32 reference %.2e, bar %.2e' % (tag, what, err, e32, bar))
    assert torch.isfinite(got).all(), what
    assert err <= bar, what
  return score, state, outbuf, y64


# (N, C, D, B, num_prop, agg, mask, row padding, how L reaches the kernel); every case runs with 64-row
# and with 32-row tiles (_check).  B = 65 crosses a tile boundary with a remainder (a tile holds
# floor(64 / N) or floor(32 / N) molecules)
KERNEL_CASES = [
    (1, 1, 32, 1, 1, 'sum', None, 0, 'plain'),
    (5, 2, 32, 3, 2, 'avg', 'ragged', 0, 'plain'),
    (16, 7, 128, 3, 1, 'avg', 'ragged', 8, 'plain'),
    (17, 2, 64, 1, 3, 'sum', 'one', 0, 'sliced'),
    (31, 2, 32, 65, 2, 'avg', 'ragged', 4, 'expanded'),
    (32, 8, 128, 3, 15, 'avg', 'ragged', 0, 'plain'),
    (32, 7, 128, 65, 2, 'avg', None, 0, 'plain'),
    (32, 1, 96, 1, 0, 'sum', 'one', 0, 'plain'),
    # several molecules per tile and a further tile behind its dead rows; steps at D = 96 and D = 64 at both heights
    (5, 3, 96, 14, 3, 'avg', 'ragged', 4, 'plain'),       # tiles of 6, 6, 2 molecules (32 rows), of 12, 2 (64 rows)
    (32, 2, 96, 3, 2, 'sum', None, 0, 'sliced'),          # D = 96 with all 32 bits of a row mask
    (11, 2, 64, 7, 3, 'sum', 'one', 0, 'expanded'),       # 2, 2, 2, 1 and 5, 2
    (3, 1, 128, 23, 2, 'avg', 'ragged', 8, 'plain'),      # 10 per 32-row tile, 21 per 64-row tile: 63 live rows
    (16, 8, 64, 5, 2, 'avg', None, 0, 'plain'),           # C at its limit, tiles exactly full, one molecule left
]


@pytest.mark.parametrize('N,C,D,B,num_prop,agg,mkind,pad,lkind', KERNEL_CASES)
def test_ggnn_forward_matches_float64(N, C, D, B, num_prop, agg, mkind, pad, lkind):
  S, L, W = _operands(3000 + N + 7 * C + D, B, N, C, D)
  mask = _mask(mkind, B, N, 17 + N)
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
  before = Ld.clone()
  score, state, outbuf, _ = _check('N %d C %d D %d B %d steps %d %s' % (N, C, D, B, num_prop, agg), S, L, W, mask,
                                   num_prop, agg, Ld=Ld, pad=pad)
  assert tuple(score.shape) == (B, 16) and tuple(state.shape) == (B, N, D)
  assert torch.equal(Ld, before)                               # L is read, never written
  if pad:
    assert torch.isnan(outbuf[:, :, D:]).all()                 # nothing written beyond the width
  if num_prop == 0:
    assert torch.equal(state.cpu(), S)                         # the readout of state_0


def test_ggnn_gates_stay_finite_when_they_saturate():
  """weights scaled until the gate pre-activations pass +-100: a tanh built from exp(2 x) gives inf / inf"""
  N, C, D, B = 17, 2, 64, 3
  S, L, W = _operands(91, B, N, C, D, scale=5.0, density=0.5)   # first-step pre-activations of about +-150
  S = 2.0 * S
  W[8:] = _operands(91, B, N, C, D)[2][8:]                     # the readout weights stay Xavier-sized
  Sd, Ld = S.double(), L.double()
  Wd = [w.double() for w in W]
  A = G.adjacency(Ld, 'avg', torch.float64)
  gi = sum((A[:, c] @ (torch.relu(Sd @ Wd[0][c].t() + Wd[1][c]) @ Wd[2][c].t() + Wd[3][c])) @ Wd[4][:, c * D:(c + 1) * D].t()
           for c in range(C)) + Wd[5]
  gh = Sd @ Wd[6].t() + Wd[7]
  pre_rz, pre_n = (gi + gh)[..., :2 * D], gi[..., 2 * D:]
  assert float(pre_rz.max()) > 100.0 and float(pre_rz.min()) < -100.0
  assert float(pre_n.max()) > 100.0 and float(pre_n.min()) < -100.0
  _check('saturated gates', S, L, W, _mask('ragged', B, N, 3), 2, 'avg')


def test_degree_zero_rows_and_any_nonzero_entry_counts_as_an_edge():
  N, C, D, B = 9, 3, 32, 4
  S, L, W = _operands(92, B, N, C, D)
  L[0, 2] = 0.0                                                # a row without an edge in every channel
  L[1, :, :, 1] = 0.0                                          # a whole channel without an edge
  L[2, 3, 4, 0], L[2, 4, 3, 2], L[3, 0, 0, 1] = -0.5, float('nan'), float('nan')
  ones = (torch.isnan(L) | (L != 0)).float()                   # what `L != 0` says
  assert float(ones[2, 4, 3, 2]) == 1.0 and float(ones[0, 2].sum()) == 0.0
  for agg in ('avg', 'sum'):
    Ld = L.cuda()
    bits = Ld.clone().view(torch.int32)
    score, state, _ = _run(S, L, W, None, 2, agg, Ld=Ld)
    assert torch.equal(Ld.view(torch.int32), bits)             # bit-identical before and after
    s32, y32 = _mirror(S, ones, W, None, 2, agg, torch.float32)
    s64, y64 = _mirror(S, ones, W, None, 2, agg, torch.float64)
    for got, r32, r64 in ((state, s32, s64), (score, y32, y64)):
      err, e32, bar = _bar(got, r32, r64, agg)
      print('ggnn_forward degree-0 / NaN entries %s: %.2e, float32 reference %.2e, bar %.2e' % (agg, err, e32, bar))
      assert torch.isfinite(got).all() and err <= bar


def test_padded_rows_take_part_and_mask_none_averages_all_rows():
  N, C, D, B = 16, 2, 32, 3
  S, L, W = _operands(93, B, N, C, D)
  mask = (torch.arange(N).unsqueeze(0) < torch.tensor([16, 9, 1]).unsqueeze(1)).to(torch.uint8)
  for b, n in enumerate((16, 9, 1)):
    L[b, n:] = 0.0
    L[b, :, n:] = 0.0
  masked, _, _, y_masked = _check('ragged, masked', S, L, W, mask, 2, 'avg')
  plain, state, _, y_plain = _check('ragged, mask=None', S, L, W, None, 2, 'avg')
  assert float((plain[1:] - masked[1:]).abs().max()) > 1e-3     # the padded rows enter the mean
  assert float((state[1, 9:].cpu() - S[1, 9:]).abs().max()) > 1e-3   # ... and evolved: GRU(0, h)


def test_ggnn_forward_is_bitwise_reproducible_and_the_raw_op_gives_the_same_bits():
  from lanczosnet_amd import ops
  N, C, D, B, P = 31, 7, 128, 5, 16
  S, L, W = _operands(94, B, N, C, D)
  Sd, Ld, Wd = S.cuda(), L.cuda(), [w.cuda() for w in W]
  mask = _mask('ragged', B, N, 5).cuda()
  s1, st1 = ops.ggnn_forward(Sd, Ld, mask, *Wd, 3, avg=True, return_state=True)
  s2, st2 = ops.ggnn_forward(Sd, Ld, mask, *Wd, 3, avg=True, return_state=True)
  assert torch.equal(s1, s2) and torch.equal(st1, st2)
  raw, raw_state = torch.empty_like(s1), torch.empty_like(st1)
  torch.ops.lanczosnet.raw_ggnn_forward(Sd, D, Ld, Ld.stride(0), Ld.stride(1), Ld.stride(2), Ld.stride(3), mask,
                                        Wd[0], Wd[1], Wd[2], Wd[3], Wd[4], Wd[5], Wd[6], Wd[7], Wd[8], Wd[9],
                                        Wd[10].reshape(-1), Wd[11], B, N, C, D, P, 3, 1, raw, raw_state, D, 0)
  assert torch.equal(raw, s1) and torch.equal(raw_state, st1)
  # without a state_out the score has the same bits
  assert torch.equal(ops.ggnn_forward(Sd, Ld, mask, *Wd, 3, avg=True), s1)


def test_the_tile_height_follows_the_batch():
  """tile_rows = 0: 32-row tiles while they all fit in one round of the compute units, 64-row tiles from
  the first batch that does not; the bits are the same"""
  from lanczosnet_amd import ops
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  N, C, D = 17, 1, 32                                          # one molecule per 32-row tile
  S, L, W = _operands(96, cus + 1, N, C, D)
  Sd, Ld, Wd = S.cuda(), L.cuda(), [w.cuda() for w in W]
  small = ops.ggnn_forward(Sd[:cus], Ld[:cus], None, *Wd, 1)
  assert ops.last_kernel() == 'ggnn_forward_kernel<32, 2>'
  large = ops.ggnn_forward(Sd, Ld, None, *Wd, 1)
  assert ops.last_kernel() == 'ggnn_forward_kernel<32, 4>'
  assert torch.equal(large[:cus], small)
  assert torch.equal(large, ops.ggnn_forward(Sd, Ld, None, *Wd, 1, tile_rows=32))
  with pytest.raises(ops.LnzError):
    ops.ggnn_forward(Sd, Ld, None, *Wd, 1, tile_rows=48)


def test_a_molecule_without_nodes_scores_nan_and_its_neighbours_stay_finite():
  from lanczosnet_amd import ops
  N, C, D, B = 5, 2, 32, 4
  S, L, W = _operands(95, B, N, C, D)
  mask = torch.tensor([[1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]], dtype=torch.uint8)
  s = ops.ggnn_forward(S.cuda(), L.cuda(), mask.cuda(), *[w.cuda() for w in W], 2, avg=True)
  assert torch.isnan(s[1]).all() and torch.isfinite(s[[0, 2, 3]]).all()


def test_out_of_envelope_arguments_raise():
  from lanczosnet_amd import ops
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def run(N=8, C=2, D=32, P=16, steps=1, state0=None, short=False):
    W = [z(C, 128, D), z(C, 128), z(C, D, 128), z(C, D), z(3 * D, C * D), z(3 * D), z(3 * D, D), z(3 * D),
         z(P, D), z(P), z(1, D), z(1)]
    if short:
      W[3] = z(C, D - 1)
    return ops.ggnn_forward(z(1, N, D) if state0 is None else state0, z(1, N, N, C), None, *W, steps)
  run()
  for kw in (dict(N=33), dict(C=9), dict(D=48), dict(D=160), dict(P=17), dict(steps=-1)):
    with pytest.raises(ops.NotSupported):
      run(**kw)
  with pytest.raises(ops.NotSupported):
    run(state0=z(1, 8, 36)[:, :, 2:34])                        # rows not 16-byte aligned
  with pytest.raises(ops.LnzError):
    run(short=True)                                            # a short bias
  with pytest.raises(RuntimeError):
    run(state0=torch.zeros(1, 8, 32))                          # a host tensor


# ------------------------------------------------------------------------------------------ module
def _net(name, g):
  from lanczosnet_amd.model import GGNN
  cfg, batch, use_mask = G.case_inputs(name)
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])
  net = GGNN(cfg)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  d = {k: t(v) for k, v in batch.items()}
  if not use_mask:
    d['node_mask'] = None
  return net.cuda(), cfg, batch, P, d


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_ggnn_module_matches_the_reference_float64_scores(name):
  g = load_golden('ggnn.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.eval()
  Lbits = d['L'].clone()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      s1 = net(d['node_feat'], d['L'], mask=d['node_mask'])
      s2 = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'ggnn_hip' and not [w for w in rec if 'lanczosnet_amd' in str(w.message)]
  assert torch.equal(s1, s2)                                            # bitwise from call to call
  assert torch.equal(d['L'], Lbits)                                     # the caller's L is not overwritten
  ref = g[name + '_score64']
  err = float(np.abs(s1.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
  bar = max(1e-5, 4.0 * float(g[name + '_e_ref']))
  print('GGNN case %s: ggnn_hip vs reference float64 %.2e (reference float32 %.2e, bar %.2e)'
        % (name, err, float(g[name + '_e_ref']), bar))
  assert err <= bar
  # with a label the call returns (score, loss); no gradient is needed under no_grad -> still the kernel
  with torch.no_grad():
    s3, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  assert net.last_route == 'ggnn_hip' and torch.equal(s3, s1)
  assert abs(float(loss) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))


def _train_and_compare(name, reason):
  g = load_golden('ggnn.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.train()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
    net.zero_grad(set_to_none=True)
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
  assert net.last_route == 'ggnn_torch'
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'ggnn_torch' in str(w.message)]
  assert len(mine) == 1 and reason in str(mine[0].message)              # once per module
  assert abs(float(loss.detach()) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))
  gd = dict(net.named_parameters())
  for k, gs, ga in zip(g[name + '_names'], g[name + '_gsum'], g[name + '_gabs']):
    gr = gd[str(k)].grad
    assert gr is not None, k
    tol = 2e-4 * float(ga) + 1e-9
    assert abs(float(gr.double().sum()) - float(gs)) < tol, (k, float(gr.double().sum()), float(gs))
    assert abs(float(gr.double().abs().sum()) - float(ga)) < tol, k
  return net, d, g


def test_ggnn_training_takes_the_torch_route_and_matches_the_reference_gradients():
  _train_and_compare('b', 'gradients')


def test_the_rnn_update_takes_the_torch_route_and_matches_the_reference():
  net, d, g = _train_and_compare('e', 'gradients')
  # ... and in inference the reason is the update itself
  from lanczosnet_amd.model import GGNN
  fresh = GGNN(G.case_inputs('e')[0]).cuda().eval()
  fresh.load_state_dict(net.state_dict())
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      s = fresh(d['node_feat'], d['L'], mask=d['node_mask'])
      fresh(d['node_feat'], d['L'], mask=d['node_mask'])
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'ggnn_torch' in str(w.message)]
  assert fresh.last_route == 'ggnn_torch' and len(mine) == 1 and 'RNN update' in str(mine[0].message)
  ref = g['e_score64']
  err = float(np.abs(s.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
  assert err <= max(1e-5, 4.0 * float(g['e_e_ref']))


def test_an_in_place_update_invalidates_the_packed_operands():
  g = load_golden('ggnn.npz')
  net, cfg, batch, P, d = _net('c', g)
  net.eval()
  with torch.no_grad():
    before = net(d['node_feat'], d['L'], mask=d['node_mask'])
    net.msg_func[1][2].weight.mul_(1.5)
    after = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'ggnn_hip' and not torch.equal(before, after)
  Q = dict(P)
  Q['msg_func.1.2.weight'] = P['msg_func.1.2.weight'] * np.float32(1.5)
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
