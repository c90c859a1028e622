#!/usr/bin/env python
"""Secondary measurement: the GAT baseline at the shape of the reference's config/qm8_gat.yaml (7
layers, 8 heads of width 16, 7 channels, input 64, 16 outputs) on the package's synthetic QM8 batch,
inference, 1 x MI355X — route 'gat_hip' (f32_linear + gat_attention per layer, gat_readout) against
route 'gat_torch' (the module's own torch restatement) on the same device in the same run, the two
alternating; HIP events, medians over the repeats.  Also: the split of the 'gat_hip' step over its
three kernels (a pass of its own with one event pair per launch) and the parity of the timed batch
against the restatement evaluated in float64.  Writes profiles/gat_bench.json.  Not the headline
bench (bench.py).

    python tools/bench_gat.py [--batches 64 1024] [--steps 30] [--warmup 5] [--out profiles/gat_bench.json]
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
from lanczosnet_amd.model import GAT  # noqa: E402
from lanczosnet_amd.synthetic import draw_batch  # noqa: E402
from lanczosnet_amd.utils.arg_helper import AttrDict  # noqa: E402

LAYERS, HEADS, WIDTH, INPUT, OUTPUT, BONDS, ATOMS = 7, 8, 16, 64, 16, 6, 70


def config():
  model = dict(name='GAT', input_dim=INPUT, hidden_dim=[WIDTH] * LAYERS, output_dim=OUTPUT, num_layer=LAYERS,
               num_heads=[HEADS] * LAYERS, dropout=0.0, loss='MSE')
  return AttrDict(dict(seed=1234, dataset=dict(num_atom=ATOMS, num_bond_type=BONDS), model=model))


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


def kernel_split(net, nf, L, mask, steps, warmup):
  """median ms per step of the three kernels of route 'gat_hip', one event pair per launch"""
  layers, head = net._packs()
  B, N = nf.shape
  acc = {'linear': [], 'attention': [], 'readout': []}
  for it in range(warmup + steps):
    ev = []

    def timed(name, fn):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      out = fn()
      e1.record()
      ev.append((name, e0, e1))
      return out
    state = net.embedding.weight.detach()[nf]
    for t in range(LAYERS):
      W, a1, b1, a2, b2, bias = layers[t]
      Wh = timed('linear', lambda: ops.f32_linear(state.reshape(B * N, -1), W))
      state = timed('attention', lambda: ops.gat_attention(Wh.view(B, N, -1), L, a1, b1, a2, b2, bias, HEADS,
                                                           elu=t < LAYERS - 1))
    timed('readout', lambda: ops.gat_readout(state, mask, *head, (BONDS + 1) * HEADS))
    torch.cuda.synchronize()
    if it >= warmup:
      for k in acc:
        acc[k].append(sum(e0.elapsed_time(e1) for name, e0, e1 in ev if name == k))
  return {k: round(float(np.median(v)), 4) for k, v in acc.items()}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, nargs='+', default=[64, 1024])
  ap.add_argument('--steps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gat_bench.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_gat.py needs the MI355X'
  torch.manual_seed(1234)
  net = GAT(config()).eval().cuda()
  net64 = copy.deepcopy(net).double()
  rows = []
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  with torch.no_grad():
    for B in args.batches:
      b = draw_batch(B, seed=0)
      L = ops.laplacian_l4(t(b['adjs']), t(b['n_nodes']))
      nf, mask = t(b['node_feat']), t(b['node_mask'])
      hip = lambda: net(nf, L, mask=mask)  # noqa: E731
      tor = lambda: net._torch_forward(nf, L, mask)  # noqa: E731
      score = hip()
      assert net.last_route == 'gat_hip'
      ref = net64._torch_forward(nf, L.double(), mask)
      scale = float(ref.abs().max())
      par_hip = float((score.double() - ref).abs().max()) / scale
      par_tor = float((tor().double() - ref).abs().max()) / scale
      # alternate the two routes, twice each; keep the better median of each
      res = {'gat_hip': [], 'gat_torch': []}
      for _ in range(2):
        res['gat_hip'].append(median_ms(hip, args.steps, args.warmup))
        res['gat_torch'].append(median_ms(tor, args.steps, args.warmup))
      split = kernel_split(net, nf, L, mask, args.steps, args.warmup)
      row = {'batch': B, 'nodes_padded': int(nf.shape[1]),
             'gat_hip_ms': round(min(r[0] for r in res['gat_hip']), 4),
             'gat_torch_ms': round(min(r[0] for r in res['gat_torch']), 4),
             'gat_hip_medians_ms': [round(r[0], 4) for r in res['gat_hip']],
             'gat_torch_medians_ms': [round(r[0], 4) for r in res['gat_torch']],
             'gat_hip_kernel_ms': split,
             'rel_err_vs_float64': {'gat_hip': par_hip, 'gat_torch': par_tor},
             'finite': bool(torch.isfinite(score).all())}
      row['speedup'] = round(row['gat_torch_ms'] / row['gat_hip_ms'], 3)
      row['molecules_per_s'] = round(B / row['gat_hip_ms'] * 1e3, 1)
      rows.append(row)
      print(json.dumps(row))
  out = {'workload': 'GAT forward (inference), config/qm8_gat.yaml shape: %d layers, %d heads x %d, %d channels, '
                     'synthetic QM8 batch, fp32' % (LAYERS, HEADS, WIDTH, BONDS + 1),
         'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
         'timing': 'HIP events around one forward call, median over the steps; the two routes alternate, two '
                   'rounds each, the lower median is reported; kernel split: one event pair per launch, summed '
                   'per kernel, median over the steps (a pass of its own)',
         'parity': 'max |score - s64| / max |s64|, s64 = the torch restatement in float64 on the timed batch',
         'results': rows}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
