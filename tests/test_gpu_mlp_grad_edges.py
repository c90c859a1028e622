"""lnz_spectral_mlp_grad (csrc/spectral_gains_grad.hip) at its seams, against float64 autograd through the
reference's nn.Sequential (model/lanczos_net.py:95-123, 146-149) on operands drawn on the host
(tests/train_kernel_cases.py: MLP_CASES; the CPU side: tests/test_train_kernel_cases_cpu.py).

Cases (live rows R, parts): (1, 1); (63 | 64 | 65, 1) around one 64-row tile; (129, 1) three tiles in ONE
workgroup, whose dW2 / dW4 accumulators live in registers across the tiles, with a one-row last tile; (129, 3) one
tile per workgroup; (65, 5) three workgroups that own no tile — their partials must be zeros, which only the sums
can show (the partial buffer is ops.spectral_mlp_grad's own torch.empty: nothing is pre-filled here on purpose;
a buffer of NaN of the same size is allocated and freed first, so that stale memory, where the allocator hands it
back, is NaN and not the previous call's sums).  Each with every row of D live and with a live-row list: a strict
subset, ascending or (R = 129, parts = 1) shuffled, whose unused tail points at a row with NaN in D and dG — read
once and a result is NaN.  L in {1, 2, 16}; S = 8, and every S in 1 .. 7 at R = 65, L = 2; the power 30 is always
among the S powers.  D holds exact 0, +-1, 1e-3 and 0.05 (whose 30th power underflows) and negative values under
odd and even powers.

ReLU kink: test_gpu_mlp_grad.py's treatment with its margin of 1e-5 — the incoming gradient of a (layer, row) with a
float64 hidden pre-activation that close to 0 is zeroed; at most 5 % of the pairs per case, decided by the float64
reference alone (asserted on the CPU; printed here: 0 .. 3.1 %), and nothing at R = 1.

Bar (the scheme of test_gpu_gat_train.py), per tensor and per conv layer: truth = float64; e32 = the error of the
same autograd in CPU float32 in units of max|truth|, the LARGEST of eight evaluations (rows as listed, and seven
permutations of them); the kernel within max(k e32, 4 * 2^-23) of max|truth|.  k = 4, except where the reference
alone spreads wider (tools/train_kernel_reference_spread.py, worst / best of the eight): 8.14 at S = 1 (db6 of layer
1: the one feature D^30 is ~0 on most rows and the gradients nearly cancel; e32 there 7.3e-6) and 4.88 at S = 4
(db6 of layer 0); every other case spreads by at most 2.84 and has e32 1.8e-7 .. 7.9e-7."""
import functools

import pytest
import torch

import train_kernel_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def _device_operands(case):
  o = C.mlp_operands(*case)
  rows = None
  if o['rows'] is not None:
    rows = (o['rows'][0].to(DEV), torch.tensor([o['rows'][1]], dtype=torch.int32, device=DEV))
  return dict(D=o['D'].to(DEV), dG=o['dG'].to(DEV), rows=rows,
              layers=[[(w.to(DEV), b.to(DEV)) for (w, b) in lins] for lins in o['layers']])


def _call(case, d):
  from lanczosnet_amd import ops
  R, parts, L, S, _ = case
  T = ops._abi().spectral_mlp_grad_floats(S)
  stale = torch.full((L, parts, T), float('nan'), device=DEV)   # (see the docstring: what torch.empty may hand back)
  del stale
  return ops.spectral_mlp_grad(d['D'], C.mlp_dist(S), d['layers'], d['dG'], rows=d['rows'], rows_max=R, parts=parts)


@pytest.mark.parametrize('case', C.MLP_CASES, ids=[C.mlp_id(c) for c in C.MLP_CASES])
def test_mlp_grad_at_its_seams(case):
  R, parts, L, S, live = case
  d = _device_operands(case)
  truth, e32, _ = C.mlp_reference(*case)
  k = C.mlp_k(case)
  got = _call(case, d)
  again = _call(case, d)
  worst = 0.0
  for li in range(4):
    for which in range(2):
      name = C.MLP_NAMES[2 * li + which]
      g = got[li][which]
      assert torch.isfinite(g).all(), name
      assert torch.equal(g, again[li][which]), 'two calls with parts = %d differ in %s' % (parts, name)
      g = g.double().cpu()
      for l in range(L):
        t = truth['%s/%d' % (name, l)]
        assert tuple(g[l].shape) == tuple(t.shape), name
        e, bar = float((g[l] - t).abs().max()) / float(t.abs().max()), C.bar(e32['%s/%d' % (name, l)], k)
        worst = max(worst, e / bar)
        if l < 2 or e > bar:
          print('spectral_mlp_grad %s %s layer %d: %.2e of max|truth|, float32 autograd (worst of 8) %.2e, bar %.2e'
                % (C.mlp_id(case), name, l, e, e32['%s/%d' % (name, l)], bar))
        assert e <= bar, (name, l, e, bar)
  print('spectral_mlp_grad %s: worst error / bar %.2f over %d tensors; %.2f %% of the (layer, row) pairs on the ReLU '
        'kink (incoming gradient zeroed)' % (C.mlp_id(case), worst, 8 * L, 100 * C.mlp_operands(*case)['kink']))


def test_default_parts_is_the_library_choice():
  """parts=None keeps lnz_spectral_mlp_grad_parts' choice: the same gradients within the bar, and for one tile
  (one workgroup either way) the same bits as parts = 1."""
  from lanczosnet_amd import ops
  case = (63, 1, 2, 8, 'asc')
  d = _device_operands(case)
  a = ops.spectral_mlp_grad(d['D'], C.mlp_dist(8), d['layers'], d['dG'], rows=d['rows'], rows_max=63)
  b = _call(case, d)
  for x, y in zip(a, b):
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def test_mlp_grad_refusals():
  from lanczosnet_amd import ops
  from lanczosnet_amd.ops import _abi

  def operands(S, L, R=4):
    layers = [[(torch.ones((o, i), device=DEV), torch.ones((o,), device=DEV))
               for (o, i) in ((128, S), (128, 128), (128, 128), (S, 128))] for _ in range(L)]
    return torch.ones((R, 1), device=DEV), list(range(1, S + 1)), layers, torch.ones((L, R, S), device=DEV)

  ops.spectral_mlp_grad(*operands(8, 16), parts=1)
  with pytest.raises(ops.NotSupported):
    ops.spectral_mlp_grad(*operands(9, 1), parts=1)
  with pytest.raises(ops.LnzError) as e:
    ops.spectral_mlp_grad(*operands(8, 17), parts=1)
  assert not isinstance(e.value, ops.NotSupported)
  # rows without n_rows, through the raw ABI
  D, dist, layers, dG = operands(8, 1)
  keep = [t for lins in layers for wb in lins for t in wb]
  partials = torch.zeros((1, 1, _abi().spectral_mlp_grad_floats(8)), device=DEV)
  rows = torch.zeros((4,), dtype=torch.int32, device=DEV)
  with pytest.raises(ops.LnzError) as e:
    _abi().spectral_mlp_grad(D, 4, 1, dist, 8, 1, rows, None, dG, keep, 1, partials)
  assert not isinstance(e.value, ops.NotSupported)
