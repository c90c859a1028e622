#!/usr/bin/env python
"""CPU only: the spread of the float32 reference arithmetic that the K of tests/test_gpu_ggnn.py rests on.
For every kernel-level shape of that file (its own operand draws, mask and L kind; B capped at 9), at the
shape's own num_prop and at 15, with 'avg' and with 'sum': the float32 mirror (tests/ggnn_mirror.py) is
evaluated eight times — once as drawn, seven times with every operand moved by -1, 0 or +1 ulp and the
channels of the gate sum in a random order — and each run's error against the float64 mirror is taken, for
the final state and for the score; the figure is worst / best of the eight, the larger of the two.  No
kernel runs and no GPU is needed: the bar of the GPU tests comes from the reference alone.
Prints one line per shape and the largest ratio per aggregate.  Measured with these draws: 'avg' 2.85 (score,
N 32, C 2, D 96, 15 steps; states <= 2.22); 'sum' at a shape's own num_prop <= 4.35 (state) and <= 5.74 (score),
at 15 steps 5.86 (state) and 7.24 (score) at N 32, C 1, D 96 and 4.85 (state) and 13.12 (score) at N 31, C 2,
D 32, where e32 itself reaches 3e-4.  The rows with several molecules per tile: 'avg' <= 1.61 (state), 2.85
(score), 'sum' <= 3.44 (state), 4.55 (score).  The figures move with the draws: the test file's 10.5 for 'sum'
comes from an earlier measurement of the same recipe and is kept, being the lower bar.

    python tools/ggnn_reference_spread.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import ggnn_mirror as G  # noqa: E402
import test_gpu_ggnn as T  # noqa: E402

DRAWS = 8
LONG = 15


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
  for N, C, D, B, num_prop, _, mkind, _, lkind in T.KERNEL_CASES:
    B = min(B, 9)
    for agg in ('avg', 'sum'):
      for steps in sorted({max(num_prop, 1), LONG}):
        S, L, W = T._operands(3000 + N + 7 * C + D, B, N, C, D)
        if lkind == 'expanded':
          L = L[..., :1].expand(B, N, N, C)
        mask = T._mask(mkind, B, N, 17 + N)
        d = lambda x: x.double()  # noqa: E731
        s64 = G.propagate(d(S), d(L), *[d(w) for w in W[:8]], steps, agg=agg)
        y64 = G.readout(s64, mask, *[d(w) for w in W[8:]])
        g = torch.Generator().manual_seed(1)
        es, ey = [], []
        for k in range(DRAWS):
          Sp = one_ulp(S, g) if k else S
          Wp = [one_ulp(w, g) for w in W] if k else W
          order = torch.randperm(C, generator=g).tolist() if k else None
          s32 = G.propagate(Sp, L, *Wp[:8], steps, agg=agg, order=order)
          y32 = G.readout(s32, mask, *Wp[8:])
          es.append(float((s32.double() - s64).abs().max()) / float(s64.abs().max()))
          ey.append(float((y32.double() - y64).abs().max()) / float(y64.abs().max()))
        worst[agg] = max(worst[agg], ratio(es), ratio(ey))
        print('N %d C %d D %d B %d steps %d %s: state e32 %.2e .. %.2e, worst / best %.2f; score e32 %.2e .. %.2e, '
              'worst / best %.2f' % (N, C, D, B, steps, agg, min(es), max(es), ratio(es), min(ey), max(ey), ratio(ey)),
              flush=True)
  return worst


if __name__ == '__main__':
  torch.set_num_threads(min(8, os.cpu_count() or 1))
  w = propagation()
  print("largest worst / best: 'avg' %.2f, 'sum' %.2f" % (w['avg'], w['sum']))
