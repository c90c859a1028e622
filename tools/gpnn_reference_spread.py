#!/usr/bin/env python
"""CPU only: the spread of the float32 reference arithmetic that the K of tests/test_gpu_gpnn.py rests on.
For every kernel-level shape of that file (its own operand draws, mask and graph kind, its own three step
counts), with 'avg' and with 'sum': the float32 mirror (tests/gpnn_mirror.py) is evaluated eight times — once
as drawn, seven times with every operand (state, weights, L_cluster, L_cut) moved by -1, 0 or +1 ulp and the
channels of the GGNN step's gate sum in a random order — and each run's error against the float64 mirror of
the UNPERTURBED operands is taken, for the final state and for the score; the figure is worst / best of the
eight, the larger of the two.  No kernel runs and no GPU is needed: the bar of the GPU tests comes from the
reference alone.  Prints one line per shape and the largest ratio per aggregate.  Measured with these draws:
'avg' 2.51 (score, N 31, C 2, D 32, counts (1, 2); states <= 1.60), 'sum' 3.53 (score, N 32, C 8, D 128, 10 steps;
states <= 2.10, e32 up to 1.3e-5 there): both below the project's K = 4, which the test file keeps.

    python tools/gpnn_reference_spread.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import gpnn_mirror as M  # noqa: E402
import test_gpu_gpnn as T  # noqa: E402

DRAWS = 8


def one_ulp(x, g):
  """every element moved by -1, 0 or +1 ulp (a zero stays a zero: the graphs keep their pattern)"""
  d = torch.randint(-1, 2, x.shape, generator=g)
  up = torch.nextafter(x, torch.full_like(x, float('inf')))
  down = torch.nextafter(x, torch.full_like(x, float('-inf')))
  return torch.where(x == 0, x, torch.where(d > 0, up, torch.where(d < 0, down, x)))


def ratio(errors):
  return max(errors) / min(errors) if min(errors) > 0 else float('inf')


def propagation():
  worst = {'avg': 0.0, 'sum': 0.0}
  for N, C, D, B, num_prop, ncl, nct, _, mkind, _, lkind in T.KERNEL_CASES:
    if num_prop == 0:
      print('N %d C %d D %d B %d: no step, the state is state0 itself (e32 = 0): not part of the figure' % (N, C, D, B))
      continue
    counts = (num_prop, ncl, nct)
    for agg in ('avg', 'sum'):
      S, L, Lcl, Lct, W = T._operands(T._case_seed(N, C, D), B, N, C, D)
      if lkind == 'expanded':
        L = L[..., :1].expand(B, N, N, C)
      mask = T._mask(mkind, B, N, 17 + N)
      s64, y64 = T._mirror(S, L, Lcl, Lct, W, mask, counts, agg, torch.float64)
      g = torch.Generator().manual_seed(1)
      es, ey = [], []
      for k in range(DRAWS):
        Sp = one_ulp(S, g) if k else S
        Wp = [one_ulp(w, g) for w in W] if k else W
        Lclp, Lctp = (one_ulp(Lcl, g), one_ulp(Lct, g)) if k else (Lcl, Lct)
        order = torch.randperm(C, generator=g).tolist() if k else None
        s32 = M.propagate(Sp, L, Lclp, Lctp, *Wp[:16], *counts, agg=agg, order=order)
        y32 = M.readout(s32, mask, *Wp[16:])
        es.append(float((s32.double() - s64).abs().max()) / float(s64.abs().max()))
        ey.append(float((y32.double() - y64).abs().max()) / float(y64.abs().max()))
      worst[agg] = max(worst[agg], ratio(es), ratio(ey))
      print('N %d C %d D %d B %d steps %d (%d, %d) %s: state e32 %.2e .. %.2e, worst / best %.2f; score e32 %.2e .. '
            '%.2e, worst / best %.2f' % (N, C, D, B, num_prop, ncl, nct, agg, min(es), max(es), ratio(es), min(ey),
                                         max(ey), ratio(ey)), flush=True)
  return worst


if __name__ == '__main__':
  torch.set_num_threads(min(8, os.cpu_count() or 1))
  w = propagation()
  print("largest worst / best: 'avg' %.2f, 'sum' %.2f" % (w['avg'], w['sum']))
