#!/usr/bin/env python
"""Golden fixture for tests/test_segment_sum_reference.py: the outputs of the reference's CPU
operator (`operators/src/segment_reduction.cpp`, compiled unmodified into oracle/_ref/ by
oracle/ref_build.py) on the seeded inputs of the CPU test (`_cpu_cases`), so that the test pins the
oracle's restatement without the built operator.

    python tests/golden/make_golden_segment_sum.py    # needs oracle/_ref; writes segment_sum_ref.npz
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import test_segment_sum_reference as T  # noqa: E402


def main():
  if T.REF_OP is None:
    raise SystemExit('oracle/_ref is not built (python oracle/ref_build.py)')
  out = {}
  for i, (data, ids, shared, gout) in enumerate(T._cpu_cases()):
    out['fwd_%d' % i] = T._ref_forward(data, ids)
    out['fwd_shared_%d' % i] = T._ref_forward(data, shared)
    out['bwd_shared_%d' % i] = T._ref_backward(gout, shared)
  path = os.path.join(HERE, 'segment_sum_ref.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, sum(v.nbytes for v in out.values()), 'bytes')


if __name__ == '__main__':
  main()
