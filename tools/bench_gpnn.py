#!/usr/bin/env python
"""Secondary measurement: the GPNN baseline at the shape of the reference's config/qm8_gpnn.yaml (D 128,
7 channels, 10 outer steps with one cluster and one cut propagation each, 'avg', input 64, 16 outputs) on the
package's synthetic QM8 batch, inference, 1 x MI355X — route 'gpnn_hip' (a gather from the [num_atom, D] table
+ ONE gpnn_forward launch) against route 'gpnn_torch' (the module's own torch restatement) on the same device
in the same run, the two alternating; HIP events, medians over the repeats.  The partition graphs are
utils.spectral_graph_partition.get_L_cluster_cut of node labels drawn in [0, 3) (the spectral clustering is
not ported: the labels are the caller's).  Per route: the time, the number of device kernels of one call
(torch.profiler, a pass of its own), the rate on utils.flop_model.gpnn_flop_per_row_step (2.294 MFLOP per row
and outer step at the yaml shape) over the CALL time as TFLOP/s and as a fraction of the 155 TFLOP/s fp32 MFMA
peak, and the parity of the timed batch against the float64 mirror of tests/gpnn_mirror.py (CPU).  For
'gpnn_hip' also the gpnn_forward launch on its own.  Writes profiles/gpnn_bench.json.  Not the headline bench
(bench.py).

    python tools/bench_gpnn.py [--batches 64 1024] [--steps 30] [--warmup 5] [--out profiles/gpnn_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpnn_mirror as M  # noqa: E402
from lanczosnet_amd import ops  # noqa: E402
from lanczosnet_amd.model import GPNN  # noqa: E402
from lanczosnet_amd.synthetic import draw_batch  # noqa: E402
from lanczosnet_amd.utils.flop_model import gpnn_flop_per_row_step  # noqa: E402
from lanczosnet_amd.utils.spectral_graph_partition import get_L_cluster_cut  # noqa: E402

WIDTH, PROP, CLUSTER, CUT, BONDS = 128, 10, 1, 1, 6
PEAK_TFLOPS = 155.0


def config():
  return M.make_config(hidden=WIDTH, num_prop=PROP, cluster=CLUSTER, cut=CUT, agg='avg', update='GRU',
                       num_bond_type=BONDS)


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
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gpnn_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_gpnn.py needs the MI355X'
  torch.manual_seed(1234)
  cfg = config()
  net = GPNN(cfg).eval().cuda()
  P = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
  per_row = gpnn_flop_per_row_step(WIDTH, BONDS + 1, CLUSTER, CUT)
  rows = []
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  with torch.no_grad():
    for B in args.batches:
      b = draw_batch(B, seed=0)
      L = ops.laplacian_l4(t(b['adjs']), t(b['n_nodes']))
      nf, mask = t(b['node_feat']), t(b['node_mask'])
      N = int(nf.shape[1])
      labels = torch.randint(0, M.NUM_PARTITION, (B, N), generator=torch.Generator().manual_seed(B)).cuda()
      Lcl, Lct = get_L_cluster_cut(L[..., 0], labels)
      hip = lambda: net(nf, L, Lcl, Lct, mask=mask)  # noqa: E731
      tor = lambda: net._torch_forward(nf, L, Lcl, Lct, mask)  # noqa: E731
      table, operands = net._packs()
      state0 = table[nf]
      kern = lambda: ops.gpnn_forward(state0, L, Lcl, Lct, mask, *operands, PROP, CLUSTER, CUT, avg=True)  # noqa: E731
      score = hip()
      assert net.last_route == 'gpnn_hip'
      ref = M.forward(P, cfg, b['node_feat'], L.cpu().numpy(), Lcl.cpu().numpy(), Lct.cpu().numpy(), b['node_mask'])
      scale = float(ref.abs().max())
      par_hip = float((score.double().cpu() - ref).abs().max()) / scale
      par_tor = float((tor().double().cpu() - ref).abs().max()) / scale
      # alternate the two routes, twice each; keep the better median of each
      res = {'gpnn_hip': [], 'gpnn_torch': []}
      for _ in range(2):
        res['gpnn_hip'].append(median_ms(hip, args.steps, args.warmup))
        res['gpnn_torch'].append(median_ms(tor, args.steps, args.warmup))
      kernel_ms = median_ms(kern, args.steps, args.warmup)[0]
      chosen = ops.last_kernel()
      try:
        launches = {'gpnn_hip': device_kernels(hip), 'gpnn_torch': device_kernels(tor)}
      except Exception as e:   # the count is a side figure: say why it is missing
        launches = {'gpnn_hip': None, 'gpnn_torch': None, 'error': repr(e)[:200]}
      flop = float(B) * N * PROP * per_row['total']
      row = {'batch': B, 'nodes_padded': N, 'model_gflop': round(flop / 1e9, 2),
             'workgroups': (B + 32 // N - 1) // (32 // N),
             'gpnn_hip_ms': round(min(r[0] for r in res['gpnn_hip']), 4),
             'gpnn_torch_ms': round(min(r[0] for r in res['gpnn_torch']), 4),
             'gpnn_hip_medians_ms': [round(r[0], 4) for r in res['gpnn_hip']],
             'gpnn_torch_medians_ms': [round(r[0], 4) for r in res['gpnn_torch']],
             'gpnn_forward_launch_ms': round(kernel_ms, 4), 'gpnn_forward_kernel': chosen,
             'device_kernels_per_call': launches,
             'rel_err_vs_float64': {'gpnn_hip': par_hip, 'gpnn_torch': par_tor},
             'finite': bool(torch.isfinite(score).all())}
      for route in ('gpnn_hip', 'gpnn_torch'):
        tf = flop / (row[route + '_ms'] * 1e-3) / 1e12
        row[route + '_tflops'] = round(tf, 2)
        row[route + '_fraction_of_fp32_mfma_peak'] = round(tf / PEAK_TFLOPS, 4)
      tfk = flop / (kernel_ms * 1e-3) / 1e12
      row['gpnn_forward_launch_tflops'] = round(tfk, 2)
      row['gpnn_forward_launch_fraction_of_fp32_mfma_peak'] = round(tfk / PEAK_TFLOPS, 4)
      row['speedup'] = round(row['gpnn_torch_ms'] / row['gpnn_hip_ms'], 3)
      row['hip_faster'] = bool(row['gpnn_hip_ms'] < row['gpnn_torch_ms'])
      row['molecules_per_s'] = round(B / row['gpnn_hip_ms'] * 1e3, 1)
      rows.append(row)
      print(json.dumps(row))
  out = {'workload': 'GPNN forward (inference), config/qm8_gpnn.yaml shape: D %d, %d channels, %d outer steps, counts '
                     '(%d, %d), avg, synthetic QM8 batch, node labels drawn in [0, 3), fp32'
                     % (WIDTH, BONDS + 1, PROP, CLUSTER, CUT),
         'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
         'timing': 'HIP events around one forward call, median over the steps; the two routes alternate, two '
                   'rounds each, the lower median is reported; gpnn_forward_launch_ms: the one kernel launch on a '
                   'state gathered beforehand, timed the same way',
         'flop_per_row_and_outer_step': per_row,
         'rate': 'utils.flop_model.gpnn_flop_per_row_step (every padded row counted) over the time named; fraction '
                 'of the %.0f TFLOP/s fp32 MFMA peak' % PEAK_TFLOPS,
         'parity': 'max |score - s64| / max |s64|, s64 = tests/gpnn_mirror.py in float64 (CPU) on the timed batch',
         'condition': "'gpnn_hip' is faster than 'gpnn_torch' at every batch: %s" % all(r['hip_faster'] for r in rows),
         'results': rows}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
