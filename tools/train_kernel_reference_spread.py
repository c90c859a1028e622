#!/usr/bin/env python
"""CPU only: the float32 reference error (e32) and its spread that the bars of tests/test_gpu_head_grad_edges.py,
tests/test_gpu_mlp_grad_edges.py and tests/test_gpu_gain_grad_edges.py rest on.  For every case of
tests/train_kernel_cases.py the float32 reference is evaluated eight times — as drawn, and seven times with the
molecules and rows consistently permuted and the results un-permuted — against the float64 one; per output tensor
e32 is the largest of the eight errors and the spread worst / best (each error first raised to one ulp of the
scale).  Prints one line per case (its largest e32, its largest spread and the tensor that has it; for the filter
MLP also the share of (layer, row) pairs on the ReLU kink) and, per kernel, the largest spread.  A case whose spread
exceeds the project's 4 is marked: that spread is the k of its bar (K_MLP_CASE of train_kernel_cases.py; every other
case keeps k = 4).  No kernel runs.

    python tools/train_kernel_reference_spread.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import train_kernel_cases as C  # noqa: E402


def line(kind, name, e32, spread, extra=''):
  ke = max(e32, key=e32.get)
  ks = max(spread, key=spread.get)
  print('%-5s %-24s e32 <= %.2e (%s), worst / best <= %.2f (%s)%s%s'
        % (kind, name, e32[ke], ke, spread[ks], ks, extra, '   <-- k of this case' if spread[ks] > 4.0 else ''),
        flush=True)
  return spread[ks]


def main():
  torch.set_num_threads(min(8, os.cpu_count() or 1))
  worst = {'head': 0.0, 'mlp': 0.0, 'gain': 0.0}
  seen = set()
  for c in C.HEAD_CASES:
    key = c[:3] + (c[:4] == C.HEAD_GATE100,)
    if key in seen:
      continue
    seen.add(key)
    _, e32, spread = C.head_reference(*key)
    worst['head'] = max(worst['head'], line('head', C.head_id(c), e32, spread))
  for c in C.MLP_CASES:
    _, e32, spread = C.mlp_reference(*c)
    kink = C.mlp_operands(*c)['kink']
    worst['mlp'] = max(worst['mlp'], line('mlp', C.mlp_id(c), e32, spread, ', on the kink %.2f %%' % (100 * kink)))
  for name in sorted(C.GAIN_CASES):
    _, e32, spread = C.gain_reference(name)
    worst['gain'] = max(worst['gain'], line('gain', name, e32, spread))
  print('largest worst / best: head %.2f, filter MLP %.2f, gain gradient %.2f'
        % (worst['head'], worst['mlp'], worst['gain']))


if __name__ == '__main__':
  main()
