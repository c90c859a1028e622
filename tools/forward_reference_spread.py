#!/usr/bin/env python
"""CPU only: the float32 reference error (e32), the split-precision yardstick (e_split, gemm_mode 'f16x3' cases)
and their spread that the bars of tests/test_gpu_strip_forward_edges.py and tests/test_gpu_tile_forward_edges.py
rest on.  For every case of tests/forward_cases.py the reference forward is evaluated eight times in float32 — as
drawn, and seven times with the molecules and every molecule's nodes consistently permuted and the results
un-permuted — against the float64 one; per output tensor e is the largest of the eight errors in units of
max|truth| and the spread worst / best (each error first raised to one ulp of the scale).  Prints one line per case
and tensor (-v) or per case, and the largest bar.  A case whose spread exceeds the project's 4 is marked: that
spread is the k of its bar (K_FORWARD_CASE of forward_cases.py).  No kernel runs.

    python tools/forward_reference_spread.py [-v] [case ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import forward_cases as C  # noqa: E402


def main():
  torch.set_num_threads(min(8, os.cpu_count() or 1))
  args = [a for a in sys.argv[1:] if a != '-v']
  verbose = '-v' in sys.argv[1:]
  names = args or list(C.CASES)
  worst_bar, worst_spread = 0.0, 0.0
  for name in names:
    _, e, spread = C.forward_reference(name)
    what = 'e_split' if C.CASES[name]['gemm'] == 'f16x3' else 'e32'
    k = C.forward_k(name)
    if verbose:
      for t in e:
        print('%-24s %-8s %s %.2e  worst / best %.2f  bar %.2e' % (name, t, what, e[t], spread[t], C.bar(e[t], k)))
    ke, ks = max(e, key=e.get), max(spread, key=spread.get)
    b = max(C.bar(v, k) for v in e.values())
    print('%-24s %s <= %.2e (%s), worst / best <= %.2f (%s), k %.2f, largest bar %.2e%s%s'
          % (name, what, e[ke], ke, spread[ks], ks, k, b, '   <-- k of this case' if spread[ks] > 4.0 else '',
             '   <-- above %.0e' % C.BAR_CAP if b > C.BAR_CAP else ''), flush=True)
    worst_bar, worst_spread = max(worst_bar, b), max(worst_spread, spread[ks])
  print('largest worst / best %.2f, largest bar %.2e' % (worst_spread, worst_bar))


if __name__ == '__main__':
  main()
