"""GPU: the fused MPNN kernels (csrc/mpnn.hip) against the float64 restatements of tests/mpnn_mirror.py, and
the module's two routes against the reference's own numbers in tests/golden/mpnn.npz.

Bar of the kernel-level cases (the scheme of test_gpu_ggnn.py): the reference arithmetic is the CPU float32
torch evaluation of the reference's own formula on the same inputs — the unfactored pairwise MLP for the
propagation, the per-molecule loop for Set2Vec; its error e32 against float64 is measured at run time and
the kernel has to be within max(K e32, 4 fp32 ulps) max|ref64| of float64.  (The float64 yardstick of the
propagation is the factored mirror: it agrees with the pairwise one to 1e-15, test_mpnn_cpu.py.)
K starts at the project's 4: another summation order draws another sample of the same rounding.
Measured before relying on it (CPU, the float32 pairwise mirror with one-ulp-perturbed operands and a
permuted channel order against float64, eight draws per shape, the thirteen shapes below (B <= 9) at their own
num_prop and at 7, each with 'avg' and with 'sum'), worst / best e32 of the eight draws: 'avg' 1.2 .. 5.0
(worst: N 1, C 1, D 32, 7 steps; e32 itself 5e-8 .. 6e-7), 'sum' 1.5 .. 5.3 (worst: N 32, C 8, D 128, 7 steps;
e32 up to 1.3e-4: an unnormalised sum over up to 32 neighbours grows the state's sensitivity step by step).
The five rows with several molecules per tile stay below both: 'avg' 1.17 .. 1.72 (worst: N 16, C 8, D 64,
2 steps), 'sum' 1.45 .. 2.95 (worst: N 32, C 2, D 96, 7 steps).
Set2Vec (the shapes below, one-ulp-perturbed operands, eight draws): 1.2 .. 4.2 (worst: N 5, D 32, 3 steps;
the two D = 96 shapes 1.97 and 1.24).  GRU(0, S), the zero-L case of the cell test, both float32 mirrors,
D 32 .. 128: 1.1 .. 2.0.
All three exceed 4, so K is the measured spread: 5.0, 5.3 and 4.2.
tools/mpnn_reference_spread.py (CPU only) re-measures these figures from this file's own operand draws.
The kernel's own output never enters the bar.
Module level: max(1e-5, 4 e_ref) max|s64| with e_ref read from the fixture."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

import mpnn_mirror as G

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
K = {'avg': 5.0, 'sum': 5.3, 'set2vec': 4.2}   # measured spread of the reference arithmetic, see above


def _bar(got, ref32, ref64, kind):
  scale = float(ref64.abs().max())
  e32 = float((ref32.double() - ref64).abs().max()) / scale
  err = float((got.double().cpu() - ref64).abs().max()) / scale
  return err, e32, max(K[kind] * e32, 4.0 * ULP)


def _operands(seed, B, N, C, D, density=0.3):
  """(state0, L, the eight operands): Xavier-bounded weights, biases +-0.1, a sparse ASYMMETRIC L with
  negative entries (only != 0 matters), self loops, a row with every bit set and (N > 1) a row without an edge"""
  g = torch.Generator().manual_seed(seed)
  u = lambda bound, *s: (torch.rand(*s, generator=g) * 2 - 1) * bound  # noqa: E731
  xav = lambda *s: u(float(np.sqrt(6.0 / (s[-1] + s[-2]))), *s)  # noqa: E731
  S = 0.5 * torch.randn(B, N, D, generator=g)
  L = (torch.rand(B, N, N, C, generator=g) < density).float() * (torch.rand(B, N, N, C, generator=g) - 0.5)
  L[B - 1, N // 2, N // 2, C - 1] = 0.5       # a self loop
  L[0, 0, :, 0] = -0.25                       # all N bits of a row (32 at N = 32), its self loop among them
  if N > 1:
    L[0, N - 1] = 0.0                         # a row without an edge in every channel
  W = [xav(C, G.HIDDEN, 2 * D), u(0.1, C, G.HIDDEN), xav(C, D, G.HIDDEN), u(0.1, C, D), xav(3 * D, C * D),
       u(0.1, 3 * D), xav(3 * D, D), u(0.1, 3 * D)]
  return S, L, W


def _padded(x, pad):
  """x [B, N, W] as a view of a [B, N, W + pad] device buffer filled with NaN beyond the width"""
  buf = torch.full(x.shape[:2] + (x.shape[2] + pad,), float('nan'), device='cuda')
  buf[:, :, :x.shape[2]] = x.cuda()
  return buf[:, :, :x.shape[2]]


def _run(S, Ld, W, num_prop, agg, pad=0, tile_rows=0):
  from lanczosnet_amd import ops
  B, N, D = S.shape
  outbuf = torch.full((B, N, D + pad), float('nan'), device='cuda')
  state = ops.mpnn_forward(_padded(S, pad), Ld, *[w.cuda() for w in W], num_prop, avg=agg == 'avg',
                           state_out=outbuf[:, :, :D], tile_rows=tile_rows)
  return state, outbuf


# (N, C, D, B, num_prop, agg, row padding, how L reaches the kernel); every case runs with 64-row and with
# 32-row tiles.  B = 65 crosses a tile boundary with a remainder (a tile holds floor(64 / N) or floor(32 / N)
# molecules)
KERNEL_CASES = [
    (1, 1, 32, 1, 1, 'sum', 0, 'plain'),
    (5, 2, 32, 3, 2, 'avg', 0, 'plain'),
    (16, 7, 128, 3, 1, 'avg', 8, 'plain'),
    (17, 2, 64, 1, 3, 'sum', 0, 'sliced'),
    (31, 2, 32, 65, 2, 'avg', 0, 'expanded'),
    (32, 8, 128, 3, 7, 'avg', 0, 'plain'),
    (32, 7, 128, 65, 2, 'avg', 0, 'plain'),
    (32, 1, 96, 1, 0, 'sum', 0, 'plain'),
    # several molecules per tile and a further tile behind its dead rows; steps at D = 96 (six of the eight waves
    # own features, all eight produce [P|Q]) and at D = 64 at both heights
    (5, 3, 96, 14, 3, 'avg', 4, 'plain'),                 # tiles of 6, 6, 2 molecules (32 rows), of 12, 2 (64 rows)
    (32, 2, 96, 3, 2, 'sum', 0, 'sliced'),                # D = 96 with all 32 bits of a row mask
    (11, 2, 64, 7, 3, 'sum', 0, 'expanded'),              # 2, 2, 2, 1 and 5, 2
    (3, 1, 128, 23, 2, 'avg', 8, 'plain'),                # 10 per 32-row tile, 21 per 64-row tile: 63 live rows
    (16, 8, 64, 5, 2, 'avg', 0, 'plain'),                 # C at its limit, tiles exactly full, one molecule left
]


@pytest.mark.parametrize('N,C,D,B,num_prop,agg,pad,lkind', KERNEL_CASES)
def test_mpnn_forward_matches_float64(N, C, D, B, num_prop, agg, pad, lkind):
  from lanczosnet_amd import ops
  S, L, W = _operands(4000 + N + 7 * C + D, B, N, C, D)
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
  assert ((L != 0) != (L.transpose(1, 2) != 0)).any() or N == 1         # asymmetric: swapped halves of W1 show
  assert (L < 0).any() and bool((L[0, 0, :, 0] != 0).all())
  before = Ld.clone()
  state, outbuf = _run(S, Ld, W, num_prop, agg, pad=pad, tile_rows=64)
  assert ops.last_kernel() == 'mpnn_forward_kernel<%d, 4>' % D
  state32, _ = _run(S, Ld, W, num_prop, agg, pad=pad, tile_rows=32)
  assert ops.last_kernel() == 'mpnn_forward_kernel<%d, 2>' % D
  assert torch.equal(state32, state)                          # a row's bits do not depend on the tile height
  again, _ = _run(S, Ld, W, num_prop, agg, pad=pad, tile_rows=64)
  assert torch.equal(again, state)                            # bitwise from call to call
  assert torch.equal(Ld, before)                              # L is read, never written
  r32 = G.propagate_pairwise(S, L, *W, num_prop, agg=agg)
  r64 = G.propagate_factored(S.double(), L.double(), *[w.double() for w in W], num_prop, agg=agg)
  err, e32, bar = _bar(state, r32, r64, agg)
  print('mpnn_forward N %d C %d D %d B %d steps %d %s: %.2e of the scale, float32 reference %.2e, bar %.2e'
        % (N, C, D, B, num_prop, agg, err, e32, bar))
  assert tuple(state.shape) == (B, N, D) and torch.isfinite(state).all()
  assert err <= bar
  if pad:
    assert torch.isnan(outbuf[:, :, D:]).all()                # nothing written beyond the width
  if num_prop == 0:
    assert torch.equal(state.cpu(), S)                        # the state copied through


def test_any_nonzero_entry_is_an_edge_and_padded_rows_evolve():
  N, C, D, B = 9, 3, 32, 4
  S, L, W = _operands(92, B, N, C, D)
  L[1, :, :, 1] = 0.0                                          # a whole channel without an edge
  L[2, 3, 4, 0], L[2, 4, 3, 2], L[3, 0, 0, 1] = -0.5, float('nan'), float('nan')
  L[3, 5:] = 0.0                                               # padded rows of molecule 3: degree 0
  L[3, :, 5:] = 0.0
  ones = (torch.isnan(L) | (L != 0)).float()                   # what `L != 0` says
  for agg in ('avg', 'sum'):
    Ld = L.cuda()
    bits = Ld.clone().view(torch.int32)
    state, _ = _run(S, Ld, W, 2, agg)
    assert torch.equal(Ld.view(torch.int32), bits)             # bit-identical before and after
    r32 = G.propagate_pairwise(S, ones, *W, 2, agg=agg)
    r64 = G.propagate_factored(S.double(), ones.double(), *[w.double() for w in W], 2, agg=agg)
    err, e32, bar = _bar(state, r32, r64, agg)
    print('mpnn_forward degree-0 / NaN entries %s: %.2e, float32 reference %.2e, bar %.2e' % (agg, err, e32, bar))
    assert torch.isfinite(state).all() and err <= bar
    assert float((state[3, 5:].cpu() - S[3, 5:]).abs().max()) > 1e-3   # the padded rows evolved: GRU(0, h)


def test_the_tile_height_follows_the_batch_and_bad_arguments_raise():
  from lanczosnet_amd import ops
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  N, C, D = 17, 1, 32                                          # one molecule per 32-row tile
  S, L, W = _operands(96, cus + 1, N, C, D)
  Sd, Ld, Wd = S.cuda(), L.cuda(), [w.cuda() for w in W]
  small = ops.mpnn_forward(Sd[:cus], Ld[:cus], *Wd, 1)
  assert ops.last_kernel() == 'mpnn_forward_kernel<32, 2>'
  large = ops.mpnn_forward(Sd, Ld, *Wd, 1)
  assert ops.last_kernel() == 'mpnn_forward_kernel<32, 4>'
  assert torch.equal(large[:cus], small)
  with pytest.raises(ops.LnzError):
    ops.mpnn_forward(Sd, Ld, *Wd, 1, tile_rows=48)
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def run(N=8, C=2, D=32, steps=1):
    W = [z(C, 64, 2 * D), z(C, 64), z(C, D, 64), z(C, D), z(3 * D, C * D), z(3 * D), z(3 * D, D), z(3 * D)]
    return ops.mpnn_forward(z(1, N, D), z(1, N, N, C), *W, steps)
  run()
  for kw in (dict(N=33), dict(C=9), dict(D=48), dict(D=160), dict(steps=-1)):
    with pytest.raises(ops.NotSupported):
      run(**kw)
  with pytest.raises(RuntimeError):
    ops.mpnn_forward(S, Ld, *Wd, 1)                            # a host tensor


# ------------------------------------------------------------------- the cell, across the two forwards
ZERO_MESSAGE = dict(N=5, B=14, C=2, steps=3)   # tiles of 6, 6, 2 molecules (32 rows) and of 12, 2 (64 rows)


def zero_message_case(D):
  """CPU.  With L identically zero every message is exactly 0 in both models (GGNN: an empty bit row sums nothing
  and the gate product of zeros is +0; MPNN: R = 0, deg = 0, 0 / (0 + eps) = 0), so ggnn_forward and mpnn_forward
  both compute GRU(0, S) step by step.  -> (S, L, the MPNN operands, the GGNN operands with the MPNN draw's four
  cell operands, the float64 truth, e32 of the float32 MPNN mirror, e32 of the float32 GGNN mirror); the truth is
  the float64 MPNN mirror, and the float64 GGNN mirror and torch.nn.GRUCell on a zero input agree with it."""
  import ggnn_mirror as GG
  import test_gpu_ggnn as TG
  N, B, C, steps = (ZERO_MESSAGE[k] for k in ('N', 'B', 'C', 'steps'))
  S, _, W = _operands(4500 + D, B, N, C, D)
  Wg = TG._operands(3500 + D, B, N, C, D)[2]
  Wg[4:8] = W[4:8]                                             # one cell: Wih, bih, Whh, bhh
  L = torch.zeros(B, N, N, C)
  d = lambda ws: [w.double() for w in ws]  # noqa: E731
  truth = G.propagate_factored(S.double(), L.double(), *d(W), steps, agg='avg')
  cell = torch.nn.GRUCell(C * D, D).double()
  with torch.no_grad():
    for p, w in zip((cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh), W[4:8]):
      p.copy_(w.double())
    h = S.double().reshape(B * N, D)
    for _ in range(steps):
      h = cell(torch.zeros(B * N, C * D, dtype=torch.float64), h)
  scale = float(truth.abs().max())
  for agg in ('avg', 'sum'):
    for other in (h.reshape(B, N, D), G.propagate_factored(S.double(), L.double(), *d(W), steps, agg=agg),
                  GG.propagate(S.double(), L.double(), *d(Wg[:8]), steps, agg=agg)):
      assert float((other - truth).abs().max()) <= 1e-14 * scale
  e32 = [float((r.double() - truth).abs().max()) / scale
         for r in (G.propagate_pairwise(S, L, *W, steps, agg='avg'), GG.propagate(S, L, *Wg[:8], steps, agg='avg'))]
  return S, L, W, Wg, truth, e32[0], e32[1]


@pytest.mark.parametrize('D', [32, 64, 96, 128])
def test_the_cell_has_the_same_bits_in_ggnn_forward_and_in_mpnn_forward(D):
  """ggnn_tile.hpp: "the arithmetic all three kernels promise to share to the bit".  GRU(0, S) from both forwards
  with the same cell operands: each within this file's bar of float64, the same bits at both tile heights, and
  the same bits in the two kernels."""
  from lanczosnet_amd import ops
  S, L, W, Wg, truth, e32_m, e32_g = zero_message_case(D)
  steps = ZERO_MESSAGE['steps']
  scale = float(truth.abs().max())
  Sd, Ld, Wd, Wgd = S.cuda(), L.cuda(), [w.cuda() for w in W], [w.cuda() for w in Wg]
  for agg in ('avg', 'sum'):
    states = {}
    for rows in (32, 64):
      m = ops.mpnn_forward(Sd, Ld, *Wd, steps, avg=agg == 'avg', tile_rows=rows)
      assert ops.last_kernel() == 'mpnn_forward_kernel<%d, %d>' % (D, rows // 16)
      g = ops.ggnn_forward(Sd, Ld, None, *Wgd, steps, avg=agg == 'avg', return_state=True, tile_rows=rows)[1]
      assert ops.last_kernel() == 'ggnn_forward_kernel<%d, %d>' % (D, rows // 16)
      states[rows] = (m, g)
      for who, got, e32 in (('mpnn_forward', m, e32_m), ('ggnn_forward', g, e32_g)):
        err, bar = float((got.double().cpu() - truth).abs().max()) / scale, max(K[agg] * e32, 4.0 * ULP)
        print('%s GRU(0, S) D %d %s, %d-row tiles: %.2e of the scale, float32 reference %.2e, bar %.2e'
              % (who, D, agg, rows, err, e32, bar))
        assert torch.isfinite(got).all() and err <= bar, who
    for k, who in enumerate(('mpnn_forward', 'ggnn_forward')):
      assert torch.equal(states[32][k], states[64][k]), who       # a row's bits do not depend on the tile height
    for rows in (32, 64):
      assert torch.equal(states[rows][0], states[rows][1]), rows  # one cell: the same bits in both kernels


# ----------------------------------------------------------------------------------------- Set2Vec
def _set_operands(seed, B, N, D, P, mkind, w2_scale=1.0):
  g = torch.Generator().manual_seed(seed)
  u = lambda bound, *s: (torch.rand(*s, generator=g) * 2 - 1) * bound  # noqa: E731
  xav = lambda *s: u(float(np.sqrt(6.0 / (s[-1] + s[-2]))), *s)  # noqa: E731
  X = 0.5 * torch.randn(B, N, D, generator=g)
  W = [xav(4, D, 2 * D), u(0.1, 4, D), xav(D, D), w2_scale * xav(D, 1), xav(P, 2 * D), u(0.1, P)]
  if mkind is None:
    return X, None, W
  n = torch.randint(1, N + 1, (B,), generator=g) if mkind == 'ragged' else torch.ones(B, dtype=torch.long)
  n[0] = N if mkind == 'ragged' else 1
  if B >= 3:
    n[1] = 0                                                   # a molecule with an empty mask
  mask = (torch.arange(N).unsqueeze(0) < n.unsqueeze(1)).to(torch.uint8)
  return X, mask, W


def _set_run(X, mask, W, steps, pad=4, mols_per_group=0):
  from lanczosnet_amd import ops
  Xd = _padded(X, pad)
  if mask is not None:
    Xd[mask.cuda() == 0] = float('nan')                        # rows outside the mask must never be read
  Wg, bg, W1T = ops.set2vec_pack([(W[0][t].cuda(), W[1][t].cuda()) for t in range(4)], W[2].cuda())
  return ops.set2vec_readout(Xd, None if mask is None else mask.cuda(), Wg, bg, W1T, W[3].cuda(), W[4].cuda(),
                             W[5].cuda(), steps, mols_per_group=mols_per_group)


SET_CASES = [
    (1, 32, 1, 1, 16, 'one'),
    (5, 32, 3, 3, 4, 'ragged'),
    (32, 128, 17, 10, 16, 'ragged'),
    (32, 128, 2, 10, 16, None),
    (7, 64, 3, 0, 1, 'ragged'),
    # D = 96: the energy loop gives lanes 0 .. 7 of a sixteen-lane group two float4 and lanes 8 .. 15 one
    (9, 96, 19, 4, 16, 'ragged'),                         # groups of 16 + 3, of 5, 5, 5, 4
    (32, 96, 3, 3, 16, 'ragged'),
]


@pytest.mark.parametrize('N,D,B,steps,P,mkind', SET_CASES)
def test_set2vec_readout_matches_float64(N, D, B, steps, P, mkind):
  X, mask, W = _set_operands(5000 + N + D + B, B, N, D, P, mkind)
  from lanczosnet_amd import ops
  score = _set_run(X, mask, W, steps, mols_per_group=16)       # B = 17: a full tile of 16 and a remainder of one
  assert ops.last_kernel() == 'set2vec_readout_kernel<%d> x 16' % D
  assert torch.equal(_set_run(X, mask, W, steps, mols_per_group=16), score)   # bitwise from call to call
  for mpw in (0, 1, 5):   # a molecule's bits do not depend on the molecules per workgroup (0: chosen by the batch)
    assert torch.equal(_set_run(X, mask, W, steps, mols_per_group=mpw), score), mpw
  r32 = G.set2vec(X, mask, *W, steps)
  r64 = G.set2vec(X.double(), mask, *[w.double() for w in W], steps)
  err, e32, bar = _bar(score, r32, r64, 'set2vec')
  print('set2vec_readout N %d D %d B %d steps %d P %d %s: %.2e of the scale, float32 reference %.2e, bar %.2e'
        % (N, D, B, steps, P, mkind, err, e32, bar))
  assert tuple(score.shape) == (B, P) and torch.isfinite(score).all()
  assert err <= bar
  if mask is not None and B >= 3:
    assert int(mask[1].sum()) == 0                             # the empty set: finite, equal to the mirror
    assert float((score[1].double().cpu() - r64[1]).abs().max()) <= bar * float(r64.abs().max())
  if steps == 0:
    assert torch.equal(score.cpu(), W[5].unsqueeze(0).expand(B, P))   # score = b_out


def test_set2vec_batches_molecules_by_itself_beyond_one_round_of_the_compute_units():
  """mols_per_group = 0 just beyond B = 2 CUs: three molecules per workgroup, the last workgroup holds fewer; ragged
  masks with NaN outside them and an empty set, the same float64 bar, the bits of one molecule per workgroup"""
  from lanczosnet_amd import ops
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  N, D, steps, P = 5, 32, 3, 4
  B = 2 * cus + 1 if (2 * cus + 1) % 3 else 2 * cus + 2     # ceil(B / cus) = 3, and B is no multiple of 3
  X, mask, W = _set_operands(78, B, N, D, P, 'ragged')
  assert int(mask[1].sum()) == 0 and int(mask.sum(dim=1).max()) == N
  score = _set_run(X, mask, W, steps)
  assert ops.last_kernel() == 'set2vec_readout_kernel<32> x 3'
  assert torch.equal(_set_run(X, mask, W, steps, mols_per_group=1), score)
  assert torch.equal(_set_run(X, mask, W, steps, mols_per_group=16), score)
  r32 = G.set2vec(X, mask, *W, steps)
  r64 = G.set2vec(X.double(), mask, *[w.double() for w in W], steps)
  err, e32, bar = _bar(score, r32, r64, 'set2vec')
  print('set2vec_readout N %d D %d B %d steps %d, 3 molecules per workgroup: %.2e of the scale, float32 reference '
        '%.2e, bar %.2e' % (N, D, B, steps, err, e32, bar))
  assert torch.isfinite(score).all() and err <= bar


def test_set2vec_stays_finite_with_large_energies():
  N, D, B, P = 32, 128, 17, 16
  X, mask, W = _set_operands(77, B, N, D, P, 'ragged', w2_scale=50.0)
  score = _set_run(X, mask, W, 10)
  r64 = G.set2vec(X.double(), mask, *[w.double() for w in W], 10)
  print('set2vec_readout W_2 x 50: %.2e of the scale'
        % (float((score.double().cpu() - r64).abs().max()) / float(r64.abs().max())))
  assert torch.isfinite(score).all()


def test_set2vec_bad_arguments_raise():
  from lanczosnet_amd import ops
  z = lambda *s: torch.zeros(*s, device='cuda')  # noqa: E731

  def run(N=8, D=32, P=16, steps=1):
    return ops.set2vec_readout(z(1, N, D), None, z(4, D, 2 * D), z(4, D), z(D, D), z(D, 1), z(P, 2 * D), z(P), steps)
  run()
  for kw in (dict(N=33), dict(D=48), dict(D=160), dict(P=17), dict(steps=-1)):
    with pytest.raises(ops.NotSupported):
      run(**kw)
  for mpw in (-1, 17):
    with pytest.raises(ops.LnzError):
      ops.set2vec_readout(z(1, 8, 32), None, z(4, 32, 64), z(4, 32), z(32, 32), z(32, 1), z(16, 64), z(16), 1,
                          mols_per_group=mpw)


# ------------------------------------------------------------------------------------------ module
def _net(name, g):
  from lanczosnet_amd.model import MPNN
  cfg, batch, use_mask = G.case_inputs(name)
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  P = G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])
  net = MPNN(cfg)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  d = {k: t(v) for k, v in batch.items()}
  if not use_mask:
    d['node_mask'] = None
  return net.cuda(), cfg, batch, P, d


def _score_error(s, g, name):
  ref = g[name + '_score64']
  return float(np.abs(s.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'f'])
def test_mpnn_module_matches_the_reference_float64_scores(name):
  g = load_golden('mpnn.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.eval()
  Lbits = d['L'].clone()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      s1 = net(d['node_feat'], d['L'], mask=d['node_mask'])
      s2 = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'mpnn_hip' and not [w for w in rec if 'lanczosnet_amd' in str(w.message)]
  assert torch.equal(s1, s2)                                            # bitwise from call to call
  assert torch.equal(d['L'], Lbits)                                     # the caller's L is not overwritten
  err, bar = _score_error(s1, g, name), max(1e-5, 4.0 * float(g[name + '_e_ref']))
  print('MPNN case %s: mpnn_hip vs reference float64 %.2e (reference float32 %.2e, bar %.2e)'
        % (name, err, float(g[name + '_e_ref']), bar))
  assert err <= bar
  # with a label the call returns (score, loss); no gradient is needed under no_grad -> still the kernels
  with torch.no_grad():
    s3, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  assert net.last_route == 'mpnn_hip' and torch.equal(s3, s1)
  assert abs(float(loss) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))


def test_b_equals_one_with_sum_is_served():
  """the reference's .squeeze() (model/mpnn.py:170) breaks this call; both routes serve it and agree with the mirror"""
  from lanczosnet_amd.model import MPNN
  g = load_golden('mpnn.npz')
  cfg = G.make_config(**dict(G.CASES['f'][0], agg='sum'))
  _, batch, _ = G.case_inputs('f')
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g['f_shapes']]
  P = G.draw_params(zip([str(k) for k in g['f_names']], shapes), G.PARAM_SEED['f'])
  net = MPNN(cfg)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.cuda().eval()
  t = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
  with torch.no_grad():
    s = net(t(batch['node_feat']), t(batch['L']), mask=t(batch['node_mask']))
  assert net.last_route == 'mpnn_hip'
  ref = G.forward(P, cfg, batch['node_feat'], batch['L'], batch['node_mask']).numpy()
  assert float(np.abs(s.cpu().numpy() - ref).max() / np.abs(ref).max()) <= 1e-5


def _train_and_compare(name, reason):
  g = load_golden('mpnn.npz')
  net, cfg, batch, P, d = _net(name, g)
  net.train()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
    net.zero_grad(set_to_none=True)
    score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
    loss.backward()
  assert net.last_route == 'mpnn_torch'
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'mpnn_torch' in str(w.message)]
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


@pytest.mark.parametrize('name', ['b', 'c'])
def test_mpnn_training_takes_the_torch_route_and_matches_the_reference_gradients(name):
  _train_and_compare(name, 'gradients')


def test_the_edge_embedding_takes_the_torch_route_and_matches_the_reference():
  net, d, g = _train_and_compare('e', 'gradients')
  # ... and in inference the reason is the message function itself
  from lanczosnet_amd.model import MPNN
  fresh = MPNN(G.case_inputs('e')[0]).cuda().eval()
  fresh.load_state_dict(net.state_dict())
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      s = fresh(d['node_feat'], d['L'], mask=d['node_mask'])
      fresh(d['node_feat'], d['L'], mask=d['node_mask'])
  mine = [w for w in rec if issubclass(w.category, UserWarning) and 'mpnn_torch' in str(w.message)]
  assert fresh.last_route == 'mpnn_torch' and len(mine) == 1 and 'edge embedding' in str(mine[0].message)
  err, bar = _score_error(s, g, 'e'), max(1e-5, 4.0 * float(g['e_e_ref']))
  print('MPNN case e: mpnn_torch vs reference float64 %.2e (bar %.2e)' % (err, bar))
  assert err <= bar


def test_an_optimizer_step_invalidates_the_packed_operands():
  g = load_golden('mpnn.npz')
  net, cfg, batch, P, d = _net('c', g)
  opt = torch.optim.SGD(net.parameters(), lr=0.05)
  net.eval()
  with torch.no_grad():
    before = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'mpnn_hip'
  score, loss = net(d['node_feat'], d['L'], label=d['label'], mask=d['node_mask'])
  assert net.last_route == 'mpnn_torch'
  loss.backward()
  opt.step()
  with torch.no_grad():
    after = net(d['node_feat'], d['L'], mask=d['node_mask'])
  assert net.last_route == 'mpnn_hip' and not torch.equal(before, after)
  Q = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
  ref = G.forward(Q, cfg, batch['node_feat'], batch['L'], batch['node_mask']).numpy()
  assert float(np.abs(after.cpu().numpy() - ref).max() / np.abs(ref).max()) <= 1e-5
  # host inputs are moved with one warning
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    with torch.no_grad():
      host = net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']),
                 mask=torch.from_numpy(batch['node_mask']))
      net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']), mask=d['node_mask'])
  assert torch.equal(host, after) and len([w for w in rec if 'moved there' in str(w.message)]) == 1
