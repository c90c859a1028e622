#!/usr/bin/env python
"""Golden fixture for tests/test_graph_config_cpu.py::test_graphdata_mirror_equals_reference_collate_bitwise:
the UNMODIFIED reference's `GraphData.collate_fn` (dataset/graph_data.py) over pickles written in the
reference's format from the first six graphs of the train split of graph_config.npz (the test's own
writer), every collated tensor as it came out.

    python tests/golden/make_golden_graph_collate.py   # needs the reference tree (LANCZOS_REFERENCE); writes graph_collate.npz
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import runner_harness as H  # noqa: E402
import test_graph_config_cpu as T  # noqa: E402


def main():
  H.import_reference_runner()
  import dataset.graph_data as ref_gd
  with tempfile.TemporaryDirectory() as d:
    cfg = T.collate_config(d)
    T.write_collate_pickles(d)
    theirs = ref_gd.GraphData(cfg, split='train')
    theirs.train_data_files.sort()
    with H.numpy_expand_dims_compat():
      want = theirs.collate_fn([theirs[i] for i in range(len(theirs))])
  path = os.path.join(HERE, 'graph_collate.npz')
  np.savez_compressed(path, **{k: v.numpy() for k, v in want.items()})
  print('wrote', path)


if __name__ == '__main__':
  main()
