"""GPU: the fused GPNN kernel (csrc/gpnn.hip) against the float64 restatement of tests/gpnn_mirror.py, and
the module's two routes against the reference's own numbers in tests/golden/gpnn.npz.

Bar of the kernel-level cases: the reference arithmetic is the CPU float32 torch evaluation of the same
formula on the same inputs; its error e32 against float64 is measured at run time and the kernel's final
state and score each have to be within max(K e32, 4 fp32 ulps) max|ref64| of float64.  K starts at the
project's 4, per aggregate: another summation order draws another sample of the same rounding.  Measured
before relying on it (tools/gpnn_reference_spread.py, CPU only: the float32 mirror with one-ulp-perturbed
operands and a permuted channel order of the gate sum against float64, eight runs per shape, exactly the nine
shapes of KERNEL_CASES from this file's own draws, each at its own step counts with 'avg' and with 'sum'),
worst / best e32 of the eight runs, the larger of state and score: 'avg' 1.25 .. 2.51 (worst: the score at N 31,
C 2, D 32, counts (1, 2); e32 itself 1.3e-7 .. 9.6e-7), 'sum' 1.38 .. 3.53 (worst: the score at N 32, C 8, D 128,
10 steps, where e32 reaches 1.3e-5 on the state: the binary 'sum' over up to 32 neighbours of the GGNN step, held
in check by state_func between the steps).  Neither exceeds 4, so K = 4 holds for both aggregates.  The shape
without a step has e32 = 0 on the state (the state is state0 itself) and is held to the 4 ulps.  The kernel's own
output never enters the bar.
Module level: max(1e-5, 4 e_ref) max|s64| with e_ref read from the fixture."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import gpnn_mirror as M

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
K = {'avg': 4.0, 'sum': 4.0}   # measured spread of the reference arithmetic, see above


def _bar(got, ref32, ref64, agg):
  scale = float(ref64.abs().max())
  e32 = float((ref32.double() - ref64).abs().max()) / scale
  err = float((got.double().cpu() - ref64).abs().max()) / scale
  return err, e32, max(K[agg] * e32, 4.0 * ULP)


def _operands(seed, B, N, C, D, P=16, scale=1.0, density=0.3):
  """(state0, L, L_cluster, L_cut, the twenty operands): Xavier-bounded weights, biases +-0.1, a sparse L with
  negative entries (only != 0 matters), the partition graphs = the L4 matrices of channel 0's graph split by
  node labels drawn in [0, 3) (non-negative, a positive diagonal on every row)"""
  g = torch.Generator().manual_seed(seed)
  u = lambda bound, *s: (torch.rand(*s, generator=g) * 2 - 1) * bound  # noqa: E731
  xav = lambda *s: u(scale * float(np.sqrt(6.0 / (s[-1] + s[-2]))), *s)  # noqa: E731
  one = lambda *s: u(float(np.sqrt(6.0 / (s[-1] + s[-2]))), *s)  # noqa: E731
  S = 0.5 * torch.randn(B, N, D, generator=g)
  L = (torch.rand(B, N, N, C, generator=g) < density).float() * (torch.rand(B, N, N, C, generator=g) - 0.5)
  labels = torch.randint(0, M.NUM_PARTITION, (B, N), generator=g)
  Lcl, Lct = (torch.from_numpy(x) for x in M.partition_laplacians(L[..., 0].numpy(), labels.numpy()))
  W = [xav(C, M.HIDDEN, D), u(0.1, C, M.HIDDEN), xav(C, D, M.HIDDEN), u(0.1, C, D),
       xav(3 * D, C * D), u(0.1, 3 * D), xav(3 * D, D), u(0.1, 3 * D),
       xav(3 * D, D), u(0.1, 3 * D), xav(3 * D, D), u(0.1, 3 * D),
       one(M.STATE_HIDDEN, 3 * D), u(0.1, M.STATE_HIDDEN), one(D, M.STATE_HIDDEN), u(0.1, D),
       one(P, D), u(0.1, P), one(1, D), u(0.1, 1)]
  return S, L, Lcl, Lct, W


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


def _mirror(S, L, Lcl, Lct, W, mask, counts, agg, dtype):
  c = lambda x: x.to(dtype)  # noqa: E731
  Sf = M.propagate(c(S), c(L), c(Lcl), c(Lct), *[c(w) for w in W[:16]], *counts, agg=agg)
  return Sf, M.readout(Sf, mask, *[c(w) for w in W[16:]])


def _run(S, L, Lcl, Lct, W, mask, counts, agg, graphs=None, pad=0, tile_rows=0):
  from lanczosnet_amd import ops
  B, N, D = S.shape
  outbuf = torch.full((B, N, D + pad), float('nan'), device='cuda')
  Ld, Lcld, Lctd = (L.cuda(), Lcl.cuda(), Lct.cuda()) if graphs is None else graphs
  score, state = ops.gpnn_forward(_padded(S, pad), Ld, Lcld, Lctd, None if mask is None else mask.cuda(),
                                  *[w.cuda() for w in W], *counts, avg=agg == 'avg', state_out=outbuf[:, :, :D],
                                  tile_rows=tile_rows)
  assert ops.last_kernel() == 'gpnn_forward_kernel<%d, 2>' % D
  return score, state, outbuf


def _check(tag, S, L, Lcl, Lct, W, mask, counts, agg, **kw):
  score, state, outbuf = _run(S, L, Lcl, Lct, W, mask, counts, agg, **kw)
  s32, y32 = _mirror(S, L, Lcl, Lct, W, mask, counts, agg, torch.float32)
  s64, y64 = _mirror(S, L, Lcl, Lct, W, mask, counts, agg, torch.float64)
  for what, got, r32, r64 in (('state', state, s32, s64), ('score', score, y32, y64)):
    err, e32, bar = _bar(got, r32, r64, agg)
    print('gpnn_forward %s %s: %.2e of the scale, float32 reference %.2e, bar %.2e' % (tag, what, err, e32, bar))
    assert torch.isfinite(got).all(), what
    assert err <= bar, what
  return score, state, outbuf, (s32, y32, s64, y64)


# (N, C, D, B, num_prop, num_prop_cluster, num_prop_cut, agg, mask, row padding, how the graphs reach the kernel)
KERNEL_CASES = [
    (1, 1, 32, 1, 1, 1, 1, 'sum', None, 0, 'plain'),             # smallest
    (5, 2, 32, 3, 2, 1, 1, 'avg', 'ragged', 0, 'plain'),         # several molecules per tile
    (17, 2, 64, 1, 3, 2, 0, 'sum', 'one', 0, 'sliced'),          # a zero count, dead rows; L sliced, L_cluster strided
    (31, 2, 32, 9, 2, 1, 2, 'avg', 'ragged', 4, 'expanded'),     # tiles of one molecule, a batch remainder
    (32, 8, 128, 3, 10, 1, 1, 'avg', 'ragged', 0, 'plain'),      # yaml depth, C and D at their limits, all 32 bits
    (32, 7, 128, 5, 1, 0, 0, 'avg', None, 0, 'plain'),           # both counts zero
    (32, 1, 96, 1, 0, 1, 1, 'sum', 'one', 0, 'plain'),           # no step: the readout of state0
    (3, 1, 128, 23, 2, 1, 1, 'avg', 'ragged', 8, 'plain'),       # ten molecules per tile, 30 live rows
    (16, 3, 96, 5, 2, 1, 1, 'avg', None, 0, 'plain'),            # tiles exactly full, one molecule left
]


def _case_seed(N, C, D):
  return 5000 + N + 7 * C + D


def _case_graphs(lkind, L, Lcl, Lct):
  """-> (the host L the mirror sees, the three device tensors the kernel sees)"""
  B, N, _, C = L.shape
  if lkind == 'expanded':   # one channel, seen C times through a zero stride
    L = L[..., :1].expand(B, N, N, C)
    Ld = L[..., :1].cuda().expand(B, N, N, C)
    assert Ld.stride(3) == 0
    return L, (Ld, Lcl.cuda(), Lct.cuda())
  if lkind == 'sliced':     # channels 1, 3, .. of a wider tensor; L_cluster every other column of a wider one
    wide = torch.zeros(B, N, N, 2 * C + 1, device='cuda')
    wide[..., 1:2 * C:2] = L.cuda()
    Ld = wide[..., 1:2 * C:2]
    assert Ld.stride(3) == 2 and Ld.stride(2) == 2 * C + 1
    widec = torch.full((B, N, 2 * N + 1), float('nan'), device='cuda')
    widec[..., 1:2 * N:2] = Lcl.cuda()
    Lcld = widec[..., 1:2 * N:2]
    assert Lcld.stride(2) == 2 and Lcld.stride(1) == 2 * N + 1
    return L, (Ld, Lcld, Lct.cuda())
  return L, (L.cuda(), Lcl.cuda(), Lct.cuda())


@pytest.mark.parametrize('N,C,D,B,num_prop,ncl,nct,agg,mkind,pad,lkind', KERNEL_CASES)
def test_gpnn_forward_matches_float64(N, C, D, B, num_prop, ncl, nct, agg, mkind, pad, lkind):
  S, L, Lcl, Lct, W = _operands(_case_seed(N, C, D), B, N, C, D)
  mask = _mask(mkind, B, N, 17 + N)
  L, graphs = _case_graphs(lkind, L, Lcl, Lct)
  before = [x.clone().view(torch.int32) for x in graphs]
  score, state, outbuf, _ = _check('N %d C %d D %d B %d steps %d (%d, %d) %s' % (N, C, D, B, num_prop, ncl, nct, agg),
                                   S, L, Lcl, Lct, W, mask, (num_prop, ncl, nct), agg, graphs=graphs, pad=pad)
  assert tuple(score.shape) == (B, 16) and tuple(state.shape) == (B, N, D)
  for x, b in zip(graphs, before):
    assert torch.equal(x.view(torch.int32), b)                 # the three graphs are bit-identical after the call
  if pad:
    assert torch.isnan(outbuf[:, :, D:]).all()                 # nothing written beyond the width
  if num_prop == 0:
    assert torch.equal(state.cpu(), S)                         # the readout of state_0, the state bit-equal


def test_the_partition_graphs_enter_by_value():
  """binarising L_cluster moves the 'sum' result; scaling it by 2 moves 'sum' and leaves 'avg' within the bar
  (the row normalisation takes the factor out again, up to the FLT_EPSILON in the denominator: 1e-7 of a weight)"""
  N, C, D, B = 9, 2, 32, 4
  S, L, Lcl, Lct, W = _operands(81, B, N, C, D)
  counts = (2, 1, 1)
  base, _, _, (_, _, s64, y64) = _check('by value', S, L, Lcl, Lct, W, None, counts, 'sum')
  ones = (Lcl != 0).float()
  assert not torch.equal(ones, Lcl)
  binar, _, _, _ = _check('binarised L_cluster', S, L, ones, Lct, W, None, counts, 'sum')
  scale = float(y64.abs().max())
  assert float((binar - base).abs().max()) > 1e-3 * scale
  twice, _, _, _ = _check('2 L_cluster, sum', S, L, 2.0 * Lcl, Lct, W, None, counts, 'sum')
  assert float((twice - base).abs().max()) > 1e-3 * scale
  # 'avg': the scaled graph's result against the UNSCALED graph's float64 reference
  score, state, _ = _run(S, L, 2.0 * Lcl, Lct, W, None, counts, 'avg')
  s32, y32 = _mirror(S, L, Lcl, Lct, W, None, counts, 'avg', torch.float32)
  s64, y64 = _mirror(S, L, Lcl, Lct, W, None, counts, 'avg', torch.float64)
  for got, r32, r64 in ((state, s32, s64), (score, y32, y64)):
    err, e32, bar = _bar(got, r32, r64, 'avg')
    print('gpnn_forward 2 L_cluster, avg: %.2e, float32 reference %.2e, bar %.2e' % (err, e32, bar))
    assert err <= bar


def test_a_zero_row_of_l_cut_gives_gru_of_zero_and_stays_finite():
  """the one exception to the positive diagonal: a row set to zero on purpose has the weight 0 / FLT_EPSILON = 0
  ('avg') or 0 ('sum'), its aggregate is exactly 0 and the row's cut state is GRU(0, h)"""
  N, C, D, B = 7, 2, 32, 3
  S, L, Lcl, Lct, W = _operands(82, B, N, C, D)
  Lct[1, 3] = 0.0
  Lct[2] = 0.0
  for agg in ('avg', 'sum'):
    _check('zero rows of L_cut, %s' % agg, S, L, Lcl, Lct, W, None, (2, 1, 1), agg)
  # one outer step of cut propagation only and no edge in L: the rows of molecule 2, whose L_cut is all zero, have
  # the cut state GRU(0, h) — restated by hand and held against the mirror that sets the kernel's bar
  z = torch.zeros_like(L)
  _, _, _, (_, _, s64, _) = _check('cut only', S, z, Lcl, Lct, W, None, (1, 0, 1), 'avg')
  d = [w.double() for w in W]
  h = S.double()[2]
  gru0 = M.cell(torch.zeros_like(h), h, d[8], d[9], d[10], d[11])
  mixed = torch.relu(torch.cat([h, h, gru0], dim=1) @ d[12].t() + d[13]) @ d[14].t() + d[15]
  after = M.G.propagate(mixed.unsqueeze(0), z.double()[2:3], *d[:8], 1)
  assert float((s64[2] - after[0]).abs().max()) <= 1e-12 * float(s64.abs().max())


def test_gpnn_gates_stay_finite_when_they_saturate():
  """the message and cell weights scaled until the gate pre-activations of both cells pass +-100"""
  N, C, D, B = 17, 2, 64, 3
  S, L, Lcl, Lct, W = _operands(83, B, N, C, D, scale=5.0, density=0.5)
  S = 2.0 * S
  d = [w.double() for w in W]
  Sd = S.double()
  Mp = torch.relu(Sd @ d[0][0].t() + d[1][0]) @ d[2][0].t() + d[3][0]
  gi = (M.partition_weights(Lcl.double(), 'avg', torch.float64) @ Mp) @ d[8].t() + d[9]
  gh = Sd @ d[10].t() + d[11]
  pre_rz, pre_n = (gi + gh)[..., :2 * D], gi[..., 2 * D:]
  print('partition cell pre-activations: r, z %.0f .. %.0f, n %.0f .. %.0f'
        % (float(pre_rz.min()), float(pre_rz.max()), float(pre_n.min()), float(pre_n.max())))
  assert float(pre_rz.max()) > 100.0 and float(pre_rz.min()) < -100.0
  assert float(pre_n.max()) > 100.0 and float(pre_n.min()) < -100.0
  _check('saturated gates', S, L, Lcl, Lct, W, _mask('ragged', B, N, 3), (2, 1, 1), 'avg')


def test_degree_zero_rows_and_any_nonzero_entry_of_l_counts_as_an_edge():
  N, C, D, B = 9, 3, 32, 4
  S, L, Lcl, Lct, W = _operands(84, B, N, C, D)
  L[0, 2] = 0.0                                                # a row without an edge in every channel
  L[1, :, :, 1] = 0.0                                          # a whole channel without an edge
  L[2, 3, 4, 0], L[2, 4, 3, 2], L[3, 0, 0, 1] = -0.5, float('nan'), float('nan')
  ones = (torch.isnan(L) | (L != 0)).float()                   # what `L != 0` says
  assert float(ones[2, 4, 3, 2]) == 1.0 and float(ones[0, 2].sum()) == 0.0
  for agg in ('avg', 'sum'):
    graphs = (L.cuda(), Lcl.cuda(), Lct.cuda())
    bits = graphs[0].clone().view(torch.int32)
    score, state, _ = _run(S, L, Lcl, Lct, W, None, (2, 1, 1), agg, graphs=graphs)
    assert torch.equal(graphs[0].view(torch.int32), bits)      # bit-identical before and after
    s32, y32 = _mirror(S, ones, Lcl, Lct, W, None, (2, 1, 1), agg, torch.float32)
    s64, y64 = _mirror(S, ones, Lcl, Lct, W, None, (2, 1, 1), agg, torch.float64)
    for got, r32, r64 in ((state, s32, s64), (score, y32, y64)):
      err, e32, bar = _bar(got, r32, r64, agg)
      print('gpnn_forward degree-0 / NaN entries %s: %.2e, float32 reference %.2e, bar %.2e' % (agg, err, e32, bar))
      assert torch.isfinite(got).all() and err <= bar


def test_padded_rows_take_part_and_mask_none_averages_all_rows():
  N, C, D, B = 16, 2, 32, 3
  S, L, Lcl, Lct, W = _operands(85, B, N, C, D)
  mask = (torch.arange(N).unsqueeze(0) < torch.tensor([16, 9, 1]).unsqueeze(1)).to(torch.uint8)
  for b, n in enumerate((16, 9, 1)):
    L[b, n:] = 0.0
    L[b, :, n:] = 0.0
  labels = torch.randint(0, M.NUM_PARTITION, (B, N), generator=torch.Generator().manual_seed(5))
  Lcl, Lct = (torch.from_numpy(x) for x in M.partition_laplacians(L[..., 0].numpy(), labels.numpy()))
  assert torch.equal(Lcl[1, 9:, 9:], torch.eye(N - 9))         # the padded rows: isolated nodes, 1 on the diagonal
  masked, _, _, _ = _check('ragged, masked', S, L, Lcl, Lct, W, mask, (2, 1, 1), 'avg')
  plain, state, _, _ = _check('ragged, mask=None', S, L, Lcl, Lct, W, None, (2, 1, 1), 'avg')
  assert float((plain[1:] - masked[1:]).abs().max()) > 1e-3     # the padded rows enter the mean
  assert float((state[1, 9:].cpu() - S[1, 9:]).abs().max()) > 1e-3   # ... and evolved


def test_gpnn_forward_is_bitwise_reproducible_and_the_raw_op_gives_the_same_bits():
  from lanczosnet_amd import ops
  N, C, D, B, P = 31, 7, 128, 5, 16
  S, L, Lcl, Lct, W = _operands(86, B, N, C, D)
  Sd, Ld, Lcld, Lctd, Wd = S.cuda(), L.cuda(), Lcl.cuda(), Lct.cuda(), [w.cuda() for w in W]
  mask = _mask('ragged', B, N, 5).cuda()
  s1, st1 = ops.gpnn_forward(Sd, Ld, Lcld, Lctd, mask, *Wd, 3, 1, 1, avg=True, return_state=True)
  s2, st2 = ops.gpnn_forward(Sd, Ld, Lcld, Lctd, mask, *Wd, 3, 1, 1, avg=True, return_state=True)
  assert torch.equal(s1, s2) and torch.equal(st1, st2)
  raw, raw_state = torch.empty_like(s1), torch.empty_like(st1)
  Wr = list(Wd)
  Wr[18] = Wd[18].reshape(-1)
  torch.ops.lanczosnet.raw_gpnn_forward(Sd, D, Ld, Ld.stride(0), Ld.stride(1), Ld.stride(2), Ld.stride(3), Lcld,
                                        Lcld.stride(0), Lcld.stride(1), Lcld.stride(2), Lctd, Lctd.stride(0),
                                        Lctd.stride(1), Lctd.stride(2), mask, *Wr, B, N, C, D, P, 3, 1, 1, 1, raw,
                                        raw_state, D, 0)
  assert torch.equal(raw, s1) and torch.equal(raw_state, st1)
  # without a state_out the score has the same bits; tile_rows = 32 is what 0 chooses
  assert torch.equal(ops.gpnn_forward(Sd, Ld, Lcld, Lctd, mask, *Wd, 3, 1, 1, avg=True), s1)
  assert torch.equal(ops.gpnn_forward(Sd, Ld, Lcld, Lctd, mask, *Wd, 3, 1, 1, avg=True, tile_rows=32), s1)
  assert ops.last_kernel() == 'gpnn_forward_kernel<128, 2>'


@pytest.mark.parametrize('N,D,B,k', [(5, 32, 14, 3), (3, 128, 23, 7), (17, 64, 4, 1), (32, 96, 3, 2)])
def test_a_molecules_bits_do_not_depend_on_its_position_in_the_batch(N, D, B, k):
  """the first k molecules of a batch, run alone, give the slice's bits (k is no multiple of the molecules per
  tile: the tiles of the short run end elsewhere); so does the batch reversed"""
  from lanczosnet_amd import ops
  C = 2
  S, L, Lcl, Lct, W = _operands(87 + N, B, N, C, D)
  Sd, Ld, Lcld, Lctd, Wd = S.cuda(), L.cuda(), Lcl.cuda(), Lct.cuda(), [w.cuda() for w in W]
  mask = _mask('ragged', B, N, 9).cuda()
  run = lambda *a: ops.gpnn_forward(*a, *Wd, 2, 1, 1, avg=True, return_state=True)  # noqa: E731
  full, full_state = run(Sd, Ld, Lcld, Lctd, mask)
  part, part_state = run(Sd[:k], Ld[:k], Lcld[:k], Lctd[:k], mask[:k])
  assert torch.equal(part, full[:k]) and torch.equal(part_state, full_state[:k])
  flip = lambda x: x.flip(0).contiguous()  # noqa: E731
  back, back_state = run(flip(Sd), flip(Ld), flip(Lcld), flip(Lctd), flip(mask))
  assert torch.equal(back.flip(0), full) and torch.equal(back_state.flip(0), full_state)


@pytest.mark.parametrize('D', [32, 64, 96, 128])
def test_the_ggnn_step_and_readout_have_the_same_bits_in_ggnn_forward_and_in_gpnn_forward(D):
  """ggnn_tile.hpp's LNZ_GGNN_TILE_STEP and gated_readout are the step and the readout of both forwards.  With both partition
  counts 0 and the identity state MLP (gpnn_mirror.identity_state_mlp: state_func returns S exactly in float32, in
  any summation order; tests/test_gpnn_cpu.py) gpnn_forward is the GGNN recurrence, so it has to give
  ggnn_forward's final state and score to the bit, at the shape of test_gpu_mpnn.ZERO_MESSAGE: tiles of 6, 6 and
  2 molecules."""
  from lanczosnet_amd import ops
  N, B, C, T = 5, 14, 2, 3
  S, L, Lcl, Lct, W = _operands(6000 + D, B, N, C, D)
  W[12:16] = M.identity_state_mlp(D)
  Sd, Ld, Lcld, Lctd, Wd = S.cuda(), L.cuda(), Lcl.cuda(), Lct.cuda(), [w.cuda() for w in W]
  mask = _mask('ragged', B, N, 17 + D).cuda()
  assert len(set(mask.sum(dim=1).tolist())) > 1                              # ragged
  for agg in ('avg', 'sum'):
    p_score, p_state = ops.gpnn_forward(Sd, Ld, Lcld, Lctd, mask, *Wd, T, 0, 0, avg=agg == 'avg', return_state=True)
    assert ops.last_kernel() == 'gpnn_forward_kernel<%d, 2>' % D
    g_score, g_state = ops.ggnn_forward(Sd, Ld, mask, *Wd[:8], *Wd[16:], T, avg=agg == 'avg', return_state=True,
                                        tile_rows=32)
    assert ops.last_kernel() == 'ggnn_forward_kernel<%d, 2>' % D
    differ = (p_state != g_state).nonzero()
    print('GGNN step in gpnn_forward vs ggnn_forward D %d %s: %d of %d state elements differ%s'
          % (D, agg, len(differ), p_state.numel(), '' if len(differ) == 0 else ', first at %s: %r vs %r' % (
              tuple(differ[0].tolist()), float(p_state[tuple(differ[0])]), float(g_state[tuple(differ[0])]))))
    assert torch.isfinite(g_state).all() and float((g_state - Sd).abs().max()) > 1e-3    # the steps did run
    assert torch.equal(p_state, g_state), agg
    assert torch.equal(p_score, g_score), agg


def test_a_molecule_without_nodes_scores_nan_and_its_neighbours_stay_finite():
  from lanczosnet_amd import ops
  N, C, D, B = 5, 2, 32, 4
  S, L, Lcl, Lct, W = _operands(88, B, N, C, D)
  mask = torch.tensor([[1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]], dtype=torch.uint8)
  s = ops.gpnn_forward(S.cuda(), L.cuda(), Lcl.cuda(), Lct.cuda(), mask.cuda(), *[w.cuda() for w in W], 2, 1, 1)
  assert torch.isnan(s[1]).all() and torch.isfinite(s[[0, 2, 3]]).all()


def test_out_of_envelope_arguments_raise():
  from lanczosnet_amd import ops
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def run(N=8, C=2, D=32, P=16, steps=1, ncl=1, nct=1, state0=None, short=False, tile_rows=0):
    W = [z(C, 128, D), z(C, 128), z(C, D, 128), z(C, D), z(3 * D, C * D), z(3 * D), z(3 * D, D), z(3 * D),
         z(3 * D, D), z(3 * D), z(3 * D, D), z(3 * D), z(512, 3 * D), z(512), z(D, 512), z(D),
         z(P, D), z(P), z(1, D), z(1)]
    if short:
      W[13] = z(511)
    return ops.gpnn_forward(z(1, N, D) if state0 is None else state0, z(1, N, N, C), z(1, N, N), z(1, N, N), None,
                            *W, steps, ncl, nct, tile_rows=tile_rows)
  run()
  for kw in (dict(N=33), dict(C=9), dict(D=48), dict(D=160), dict(P=17), dict(steps=-1), dict(ncl=-1), dict(nct=-1),
             dict(tile_rows=64)):
    with pytest.raises(ops.NotSupported):
      run(**kw)
  with pytest.raises(ops.NotSupported):
    run(state0=z(1, 8, 36)[:, :, 2:34])                        # rows not 16-byte aligned
  with pytest.raises(ops.LnzError):
    run(short=True)                                            # a short bias
  with pytest.raises(ops.LnzError):
    run(tile_rows=48)
  with pytest.raises(RuntimeError):
    run(state0=torch.zeros(1, 8, 32))                          # a host tensor


# ------------------------------------------------------------------------------------------ module
def _net(name, g):
  from lanczosnet_amd.model import GPNN
  cfg, batch, use_mask = M.case_inputs(name)
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = M.draw_params(zip([str(k) for k in g[name + '_names']], shapes), M.PARAM_SEED[name])
  net = GPNN(cfg)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  d = {k: t(v) for k, v in batch.items()}
  if not use_mask:
    d['node_mask'] = None
  return net.cuda(), cfg, batch, P, d


def _fwd(net, d, **kw):
  return net(d['node_feat'], d['L'], d['L_cluster'], d['L_cut'], mask=d['node_mask'], **kw)


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_gpnn_module_matches_the_reference_float64_scores(name):
  g = load_golden('gpnn.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.eval()
  bits = [d[k].clone() for k in ('L', 'L_cluster', 'L_cut')]
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      s1 = _fwd(net, d)
      s2 = _fwd(net, d)
  assert net.last_route == 'gpnn_hip' and not [w for w in rec if 'lanczosnet_amd' in str(w.message)]
  assert torch.equal(s1, s2)                                            # bitwise from call to call
  for k, b in zip(('L', 'L_cluster', 'L_cut'), bits):
    assert torch.equal(d[k], b)                                         # the caller's graphs are not overwritten
  ref = g[name + '_score64']
  err = float(np.abs(s1.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
  bar = max(1e-5, 4.0 * float(g[name + '_e_ref']))
  print('GPNN case %s: gpnn_hip vs reference float64 %.2e (reference float32 %.2e, bar %.2e)'
        % (name, err, float(g[name + '_e_ref']), bar))
  assert err <= bar
  # with a label the call returns (score, loss); no gradient is needed under no_grad -> still the kernel
  with torch.no_grad():
    s3, loss = _fwd(net, d, label=d['label'])
  assert net.last_route == 'gpnn_hip' and torch.equal(s3, s1)
  assert abs(float(loss) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))


def _train_and_compare(name, reason):
  g = load_golden('gpnn.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.train()
  bits = [d[k].clone() for k in ('L', 'L_cluster', 'L_cut')]
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score, loss = _fwd(net, d, label=d['label'])
    loss.backward()
    net.zero_grad(set_to_none=True)
    score, loss = _fwd(net, d, label=d['label'])
    loss.backward()
  assert net.last_route == 'gpnn_torch'
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'gpnn_torch' in str(w.message)]
  assert len(mine) == 1 and reason in str(mine[0].message)              # once per module
  for k, b in zip(('L', 'L_cluster', 'L_cut'), bits):
    assert torch.equal(d[k], b)
  assert abs(float(loss.detach()) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))
  gd = dict(net.named_parameters())
  for k, gs, ga in zip(g[name + '_names'], g[name + '_gsum'], g[name + '_gabs']):
    gr = gd[str(k)].grad
    assert gr is not None, k
    tol = 2e-4 * float(ga) + 1e-9
    assert abs(float(gr.double().sum()) - float(gs)) < tol, (k, float(gr.double().sum()), float(gs))
    assert abs(float(gr.double().abs().sum()) - float(ga)) < tol, k
  return net, d, g


def test_gpnn_training_takes_the_torch_route_and_matches_the_reference_gradients():
  _train_and_compare('b', 'gradients')


def test_the_rnn_update_takes_the_torch_route_and_matches_the_reference():
  from lanczosnet_amd.model import GPNN
  g = load_golden('gpnn.npz')
  net, cfg, batch, P, d = _net('e', g)
  net.eval()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      s = _fwd(net, d)
      _fwd(net, d)
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'gpnn_torch' in str(w.message)]
  assert net.last_route == 'gpnn_torch' and len(mine) == 1 and 'RNN update' in str(mine[0].message)
  ref = g['e_score64']
  err = float(np.abs(s.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
  assert err <= max(1e-5, 4.0 * float(g['e_e_ref']))
  assert isinstance(net, GPNN)


def test_an_in_place_update_invalidates_the_packed_operands_and_host_inputs_are_moved():
  g = load_golden('gpnn.npz')
  net, cfg, batch, P, d = _net('c', g)
  net.eval()
  with torch.no_grad():
    before = _fwd(net, d)
    net.state_func[2].weight.mul_(1.5)
    after = _fwd(net, d)
  assert net.last_route == 'gpnn_hip' and not torch.equal(before, after)
  Q = dict(P)
  Q['state_func.2.weight'] = P['state_func.2.weight'] * np.float32(1.5)
  ref = M.forward(Q, cfg, batch['node_feat'], batch['L'], batch['L_cluster'], batch['L_cut'], batch['node_mask']).numpy()
  err = float(np.abs(after.cpu().numpy() - ref).max() / np.abs(ref).max())
  assert err <= 1e-5
  # host inputs are moved with one warning
  h = lambda k: torch.from_numpy(batch[k])  # noqa: E731
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      host = net(h('node_feat'), h('L'), h('L_cluster'), h('L_cut'), mask=h('node_mask'))
      net(h('node_feat'), h('L'), d['L_cluster'], h('L_cut'), mask=d['node_mask'])
  assert torch.equal(host, after) and len([w for w in rec if 'moved there' in str(w.message)]) == 1


def test_partition_laplacians_on_the_device_match_the_reference():
  from lanczosnet_amd.utils.spectral_graph_partition import get_L_cluster_cut
  g = load_golden('gpnn.npz')
  _, batch, _ = M.case_inputs('c')
  L_simple = torch.from_numpy(batch['L'][..., 0].copy()).cuda()
  keep = L_simple.clone()
  Lcl, Lct = get_L_cluster_cut(L_simple, torch.from_numpy(g['part_node_label'].astype(np.int64)).cuda())
  assert Lcl.is_cuda and Lcl.dtype == torch.float32 and torch.equal(L_simple, keep)
  assert np.abs(Lcl.cpu().numpy() - g['part_L_cluster']).max() <= 1e-6
  assert np.abs(Lct.cpu().numpy() - g['part_L_cut']).max() <= 1e-6
