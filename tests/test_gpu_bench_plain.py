"""The plain benchmark command (`bench.py --gpus 1 --steps K --warmup W`): the timed steps and the
headline line only, nothing measured beside it; `--dump-outputs DIR` writes the scores of the last
timed step, the same from run to run of the same build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(*args):
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + list(args),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
  assert out.returncode == 0, out.stderr[-3000:]
  lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
  assert len(lines) == 1, out.stdout[-2000:]
  return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
  runs = []
  for i in range(2):
    d = _bench('--steps', '7', '--warmup', '2', '--dump-outputs', str(tmp_path / str(i)))
    assert d['steps'] == 7 and d['warmup'] == 2 and d['n_gpus'] == 1
    assert d['unit'] == 'molecules/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['ms_per_step'] > 0
    assert abs(d['value'] - 1024 / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    # nothing beside the headline
    for k in ('roofline', 'cpu_baseline', 'parity_rel_err'):
      assert k not in d, k
    for k in ('sustained_clock_mode', 'pipelined_stream_mode', 'split_precision_mode',
              'lanczos_large_mode', 'ada_mode', 'graph_config_mode'):
      assert k not in d['config'], k
    assert set(d['config']['stage_ms']) == {'lanczosnet_forward'}
    s = np.load(str(tmp_path / str(i) / 'score.npy'))
    assert s.dtype == np.float32 and s.shape == (1024, 16) and np.isfinite(s).all()
    runs.append(s)
  # same inputs, same build: the same scores
  np.testing.assert_array_equal(runs[0], runs[1])
