#!/usr/bin/env python
"""CPU only: what the bar of tests/test_gpu_mpnn_train.py rests on, measured on the reference alone.

For every kernel-level case of tests/mpnn_grad_mirror.STEP_CASES (its own seeds and densities):
  * the kink figures — in float64, over every step, the smallest |edge pre-activation|, the largest
    |pre32 - pre64| of the eight float32 evaluations, their ratio (the cases need >= 4) and the number of edge
    pre-activations;
  * the spread of e32 — the CPU float32 autograd of the formula is evaluated eight times (as drawn and seven
    times with molecules, nodes and the channel order of the gate sum consistently permuted), each run's error
    against float64 autograd is taken per gradient tensor; the figure is worst / best of the eight, the largest
    over the nine tensors.  K of the test is 4 unless this exceeds 4 for an aggregate.
No kernel runs and no GPU is needed.

    python tools/mpnn_grad_reference_spread.py            # the figures of the committed seeds
    python tools/mpnn_grad_reference_spread.py --seeds    # per case: the first seed from 7000 on that is kink-free
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import mpnn_grad_mirror as GM  # noqa: E402


def figures():
  worst = {'avg': 0.0, 'sum': 0.0}
  for N, C, D, B, steps, agg, _, lkind in GM.STEP_CASES:
    S, L, W, dST = GM.step_case_inputs(N, C, D, B, steps, agg, lkind)
    smallest, widest, count = GM.kink_figures(S, L, W, steps, agg)
    d = lambda x: x.double()  # noqa: E731
    truth = GM.propagate_autograd(d(S), d(dST), d(L), [d(w) for w in W], steps, agg)
    runs = GM.propagate_e32(S, dST, L, W, truth, steps, agg, every=True)
    spread, name, lo, hi = 0.0, '', 0.0, 0.0
    for k, r in zip(GM.STEP_NAMES, runs):
      if min(r) > 0 and max(r) / min(r) > spread:
        spread, name = max(r) / min(r), k
      lo, hi = min([lo or min(r)] + [x for x in r if x > 0]), max(hi, max(r))
    worst[agg] = max(worst[agg], spread)
    print('N %d C %d D %d B %d steps %d %s %s: %d edge pre-activations, smallest %.2e, |pre32 - pre64| <= %.2e, '
          'ratio %.1f; e32 %.2e .. %.2e, worst / best %.2f (%s)'
          % (N, C, D, B, steps, agg, lkind, count, smallest, widest, smallest / widest if widest else float('inf'),
             lo, hi, spread, name), flush=True)
  print("largest worst / best: 'avg' %.2f, 'sum' %.2f" % (worst['avg'], worst['sum']))


def seeds(first=7000, tries=40):
  for N, C, D, B, steps, agg, _, lkind in GM.STEP_CASES:
    _, density = GM.CASE_DRAW[(N, C, D, B, steps, agg)]
    for seed in range(first, first + tries):
      S, L, W = GM.draw_operands(seed, B, N, C, D, density=density)
      if lkind == 'expanded':
        L = L[..., :1].expand(B, N, N, C).contiguous()
      smallest, widest, count = GM.kink_figures(S, L, W, steps, agg)
      if smallest >= GM.KINK_RATIO * widest:
        print('(%d, %d, %d, %d, %d, %r): (%d, %g),   # ratio %.1f, %d edge pre-activations'
              % (N, C, D, B, steps, agg, seed, density, smallest / widest if widest else float('inf'), count),
              flush=True)
        break
    else:
      print('(%d, %d, %d, %d, %d, %r): none of %d seeds' % (N, C, D, B, steps, agg, tries), flush=True)


if __name__ == '__main__':
  torch.set_num_threads(min(8, os.cpu_count() or 1))
  if '--seeds' in sys.argv:
    seeds()
  else:
    figures()
