#!/usr/bin/env python
"""CPU only: the spread of the float32 reference arithmetic that the K of tests/test_gpu_mpnn.py rests on.
For every kernel-level shape of that file (its own operand draws; B capped at 9), at the shape's own
num_prop and at 7, with 'avg' and with 'sum': the float32 pairwise mirror (tests/mpnn_mirror.py) is
evaluated eight times — once as drawn, seven times with every operand moved by -1, 0 or +1 ulp and the
channels of the gate sum in a random order — and each run's error against the float64 mirror is taken;
the figure is worst / best of the eight.  The same for Set2Vec (the per-molecule loop, operands moved by
an ulp), and for GRU(0, S), the zero-L case of the test that compares the cell of the two forwards (both
float32 mirrors).  No kernel runs and no GPU is needed: the bar of the GPU tests comes from the reference alone.
Prints one line per shape and the largest ratio per kind (measured: 'avg' 5.00, 'sum' 5.29, Set2Vec 4.17 — all
three at the shapes they had before; the rows with several molecules per tile and D = 96 / 64 steps give
'avg' <= 1.72, 'sum' <= 2.95, Set2Vec at D = 96 <= 1.97, GRU(0, S) <= 1.98).

    python tools/mpnn_reference_spread.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import mpnn_mirror as G  # noqa: E402
import test_gpu_mpnn as T  # noqa: E402

DRAWS = 8


def one_ulp(x, g):
  """every element moved by -1, 0 or +1 ulp"""
  d = torch.randint(-1, 2, x.shape, generator=g)
  up = torch.nextafter(x, torch.full_like(x, float('inf')))
  down = torch.nextafter(x, torch.full_like(x, float('-inf')))
  return torch.where(d > 0, up, torch.where(d < 0, down, x))


def ratio(errors):
  return max(errors) / min(errors)


def propagation():
  worst = {'avg': 0.0, 'sum': 0.0}
  for N, C, D, B, num_prop, _, _, _ in T.KERNEL_CASES:
    B = min(B, 9)
    for agg in ('avg', 'sum'):
      for steps in sorted({max(num_prop, 1), 7}):
        S, L, W = T._operands(4000 + N + 7 * C + D, B, N, C, D)
        r64 = G.propagate_factored(S.double(), L.double(), *[w.double() for w in W], steps, agg=agg)
        scale = float(r64.abs().max())
        g = torch.Generator().manual_seed(1)
        errors = []
        for k in range(DRAWS):
          Sp = one_ulp(S, g) if k else S
          Wp = [one_ulp(w, g) for w in W] if k else W
          order = torch.randperm(C, generator=g).tolist() if k else None
          r32 = G.propagate_pairwise(Sp, L, *Wp, steps, agg=agg, order=order)
          errors.append(float((r32.double() - r64).abs().max()) / scale)
        worst[agg] = max(worst[agg], ratio(errors))
        print('N %d C %d D %d B %d steps %d %s: e32 %.2e .. %.2e, worst / best %.2f'
              % (N, C, D, B, steps, agg, min(errors), max(errors), ratio(errors)), flush=True)
  return worst


def cell():
  """the zero-message case of the test that compares the cell across the two forwards: GRU(0, S), both mirrors"""
  import ggnn_mirror as GG
  worst = 0.0
  steps = T.ZERO_MESSAGE['steps']
  for D in (32, 64, 96, 128):
    S, L, W, Wg, r64, _, _ = T.zero_message_case(D)
    scale = float(r64.abs().max())
    for who, ws, fn in (('mpnn', W, G.propagate_pairwise), ('ggnn', Wg[:8], GG.propagate)):
      g = torch.Generator().manual_seed(3)
      errors = []
      for k in range(DRAWS):
        Sp = one_ulp(S, g) if k else S
        Wp = [one_ulp(w, g) for w in ws] if k else ws
        order = torch.randperm(L.shape[3], generator=g).tolist() if k else None
        errors.append(float((fn(Sp, L, *Wp, steps, agg='avg', order=order).double() - r64).abs().max()) / scale)
      worst = max(worst, ratio(errors))
      print('GRU(0, S) %s D %d steps %d: e32 %.2e .. %.2e, worst / best %.2f'
            % (who, D, steps, min(errors), max(errors), ratio(errors)), flush=True)
  return worst


def set2vec():
  worst = 0.0
  for N, D, B, steps, P, mkind in T.SET_CASES:
    if steps == 0:
      continue   # score = b_out: no arithmetic
    X, mask, W = T._set_operands(5000 + N + D + B, B, N, D, P, mkind)
    r64 = G.set2vec(X.double(), mask, *[w.double() for w in W], steps)
    scale = float(r64.abs().max())
    g = torch.Generator().manual_seed(2)
    errors = []
    for k in range(DRAWS):
      Xp = one_ulp(X, g) if k else X
      Wp = [one_ulp(w, g) for w in W] if k else W
      errors.append(float((G.set2vec(Xp, mask, *Wp, steps).double() - r64).abs().max()) / scale)
    worst = max(worst, ratio(errors))
    print('set2vec N %d D %d B %d steps %d: e32 %.2e .. %.2e, worst / best %.2f'
          % (N, D, B, steps, min(errors), max(errors), ratio(errors)), flush=True)
  return worst


if __name__ == '__main__':
  torch.set_num_threads(min(8, os.cpu_count() or 1))
  w = propagation()
  c = cell()
  s = set2vec()
  print("largest worst / best: 'avg' %.2f, 'sum' %.2f, GRU(0, S) %.2f, Set2Vec %.2f" % (w['avg'], w['sum'], c, s))
