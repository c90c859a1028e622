#!/usr/bin/env python
"""Secondary measurement: the MPNN baseline at the shape of the reference's config/qm8_mpnn.yaml (D 128,
7 channels, 7 propagation steps, msg_func MLP, 'avg', 10 Set2Vec steps, input 64, 16 outputs) on the
package's synthetic QM8 batch, inference, 1 x MI355X — route 'mpnn_hip' (a gather from the [num_atom, D]
table + ONE mpnn_forward launch + ONE set2vec_readout launch) against route 'mpnn_torch' (the module's
own torch restatement in the same factored form) on the same device in the same run, the two
alternating; HIP events, medians over the repeats.  Per route: the time, the number of device kernels
of one call (torch.profiler, a pass of its own), the rate on the model of the factored propagation,
C (2 D 128 + 2 64 D + 2 D 3D) + 2 D 3D FLOP per row and step (1.130 MFLOP at the yaml shape; the
ReLU-sum over the edges and Set2Vec are not counted), over the CALL time as TFLOP/s and as a fraction of
the 155 TFLOP/s fp32 MFMA peak, and the parity of the timed batch against the restatement evaluated in
float64.  For 'mpnn_hip' also its two launches on their own (the split between propagation and
Set2Vec), the propagation with each of its two tile heights forced.  Writes profiles/mpnn_bench.json.
Not the headline bench (bench.py).

    python tools/bench_mpnn.py [--batches 64 1024] [--steps 30] [--warmup 5] [--out profiles/mpnn_bench.json]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lanczosnet_amd import ops  # noqa: E402
from lanczosnet_amd.model import MPNN  # noqa: E402
from lanczosnet_amd.synthetic import draw_batch  # noqa: E402
from lanczosnet_amd.utils.arg_helper import AttrDict  # noqa: E402

WIDTH, PROP, INPUT, OUTPUT, BONDS, ATOMS, HIDDEN, SET_STEPS = 128, 7, 64, 16, 6, 70, 64, 10
PEAK_TFLOPS = 155.0


def config():
  model = dict(name='MPNN', input_dim=INPUT, hidden_dim=WIDTH, output_dim=OUTPUT, num_layer=1, num_prop=PROP,
               update_func='GRU', msg_func='MLP', num_step_set2vec=SET_STEPS, aggregate_type='avg', dropout=0.0,
               loss='MSE')
  return AttrDict(dict(seed=1234, dataset=dict(num_atom=ATOMS, num_bond_type=BONDS), model=model))


def model_flop(B, N):
  C, D = BONDS + 1, WIDTH
  per_row_step = C * (2 * D * 2 * HIDDEN + 2 * HIDDEN * D + 2 * D * 3 * D) + 2 * D * 3 * D
  return float(B) * N * PROP * per_row_step


def median_ms(fn, steps, warmup):
  for _ in range(warmup):
    fn()
  times = []
  for _ in range(steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1))
  return float(np.median(times)), float(np.min(times)), float(np.max(times))


def device_kernels(fn):
  """the number of device kernels one call launches (None where the profiler reports no device events)"""
  from torch.profiler import ProfilerActivity, profile
  fn()
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    fn()
    torch.cuda.synchronize()
  n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
  return n or None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, nargs='+', default=[64, 1024])
  ap.add_argument('--steps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpnn_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_mpnn.py needs the MI355X'
  torch.manual_seed(1234)
  net = MPNN(config()).eval().cuda()
  net64 = copy.deepcopy(net).double()
  rows = []
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  with torch.no_grad():
    for B in args.batches:
      b = draw_batch(B, seed=0)
      L = ops.laplacian_l4(t(b['adjs']), t(b['n_nodes']))
      nf, mask = t(b['node_feat']), t(b['node_mask'])
      N = int(nf.shape[1])
      hip = lambda: net(nf, L, mask=mask)  # noqa: E731
      tor = lambda: net._torch_forward(nf, L, mask)  # noqa: E731
      table, prop, read = net._packs()
      state0 = table[nf]
      kprop = lambda: ops.mpnn_forward(state0, L, *prop, PROP, avg=True)  # noqa: E731
      stateT = kprop()
      kread = lambda: ops.set2vec_readout(stateT, mask, *read, SET_STEPS)  # noqa: E731
      score = hip()
      assert net.last_route == 'mpnn_hip'
      ref = net64._torch_forward(nf, L.double(), mask)
      scale = float(ref.abs().max())
      par_hip = float((score.double() - ref).abs().max()) / scale
      par_tor = float((tor().double() - ref).abs().max()) / scale
      # alternate the two routes, twice each; keep the better median of each
      res = {'mpnn_hip': [], 'mpnn_torch': []}
      for _ in range(2):
        res['mpnn_hip'].append(median_ms(hip, args.steps, args.warmup))
        res['mpnn_torch'].append(median_ms(tor, args.steps, args.warmup))
      prop_ms = median_ms(kprop, args.steps, args.warmup)[0]
      chosen = ops.last_kernel()
      read_ms = median_ms(kread, args.steps, args.warmup)[0]
      # the two tile heights, forced, alternating (tile_rows = 0 above chooses between them by the batch)
      tiles = {32: [], 64: []}
      for _ in range(2):
        for rows_per_tile in (32, 64):
          tiles[rows_per_tile].append(median_ms(
              lambda: ops.mpnn_forward(state0, L, *prop, PROP, avg=True, tile_rows=rows_per_tile),
              args.steps, args.warmup)[0])
      try:
        launches = {'mpnn_hip': device_kernels(hip), 'mpnn_torch': device_kernels(tor)}
      except Exception as e:   # the count is a side figure: say why it is missing
        launches = {'mpnn_hip': None, 'mpnn_torch': None, 'error': repr(e)[:200]}
      flop = model_flop(B, N)
      row = {'batch': B, 'nodes_padded': N, 'model_gflop': round(flop / 1e9, 2),
             'mpnn_hip_ms': round(min(r[0] for r in res['mpnn_hip']), 4),
             'mpnn_torch_ms': round(min(r[0] for r in res['mpnn_torch']), 4),
             'mpnn_hip_medians_ms': [round(r[0], 4) for r in res['mpnn_hip']],
             'mpnn_torch_medians_ms': [round(r[0], 4) for r in res['mpnn_torch']],
             'mpnn_forward_launch_ms': round(prop_ms, 4), 'mpnn_forward_kernel': chosen,
             'set2vec_readout_launch_ms': round(read_ms, 4),
             'mpnn_forward_launch_ms_by_tile_rows': {str(k): round(min(v), 4) for k, v in tiles.items()},
             'device_kernels_per_call': launches,
             'rel_err_vs_float64': {'mpnn_hip': par_hip, 'mpnn_torch': par_tor},
             'finite': bool(torch.isfinite(score).all())}
      for route in ('mpnn_hip', 'mpnn_torch'):
        tf = flop / (row[route + '_ms'] * 1e-3) / 1e12
        row[route + '_tflops'] = round(tf, 2)
        row[route + '_fraction_of_fp32_mfma_peak'] = round(tf / PEAK_TFLOPS, 4)
      tfk = flop / (prop_ms * 1e-3) / 1e12
      row['mpnn_forward_launch_tflops'] = round(tfk, 2)
      row['mpnn_forward_launch_fraction_of_fp32_mfma_peak'] = round(tfk / PEAK_TFLOPS, 4)
      row['speedup'] = round(row['mpnn_torch_ms'] / row['mpnn_hip_ms'], 3)
      row['hip_not_slower'] = bool(row['mpnn_hip_ms'] <= row['mpnn_torch_ms'])
      row['molecules_per_s'] = round(B / row['mpnn_hip_ms'] * 1e3, 1)
      rows.append(row)
      print(json.dumps(row))
  out = {'workload': 'MPNN forward (inference), config/qm8_mpnn.yaml shape: D %d, %d channels, %d steps, MLP, avg, '
                     '%d Set2Vec steps, synthetic QM8 batch, fp32' % (WIDTH, BONDS + 1, PROP, SET_STEPS),
         'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
         'timing': 'HIP events around one forward call, median over the steps; the two routes alternate, two '
                   'rounds each, the lower median is reported; mpnn_forward_launch_ms and set2vec_readout_launch_ms: '
                   'the one kernel launch each on operands prepared beforehand, timed the same way',
         'rate': 'the FLOP model of the factored propagation (C (2 D 128 + 2 64 D + 2 D 3D) + 2 D 3D per row and '
                 'step, every padded row counted; the ReLU-sum over the edges and Set2Vec not counted) over the time '
                 'named; fraction of the %.0f TFLOP/s fp32 MFMA peak' % PEAK_TFLOPS,
         'parity': 'max |score - s64| / max |s64|, s64 = the torch restatement in float64 on the timed batch',
         'condition': "'mpnn_hip' is not slower than 'mpnn_torch' at either batch: %s"
                      % all(r['hip_not_slower'] for r in rows),
         'results': rows}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
