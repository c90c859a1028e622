"""Training-step timing (forward + backward + Adam) of the reference's graph configuration
(config/graph_lanczos_net.yaml: LanczosNetGeneral 7 x 128, eight long scales, K = 20, one edge type,
graphs of 20..100 nodes) at the train batch (B = 10) and the test batch (B = 64), with the HIP
backward for graphs of 33..128 nodes switched off and on (`mid_backward_impl`).

    python tools/bench_graph_train_step.py [--reps 5] [--steps 30] [--out profiles/mid_train_step.json]
    python tools/bench_graph_train_step.py --only hip --batch 10 --steps 20    # under a kernel trace

The two settings alternate in ONE process, `--reps` windows of `--steps` steps each; the spread of the
window means is reported beside their median.  Only public module calls are used, so the tool also
runs on a commit without the switch (both columns then time the torch route).  `--only` runs one
setting and nothing else: the process to put under `rocprofv3 --kernel-trace --stats`, whose launch
total divided by the printed step count (warm-up included) is the launch count per step."""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import oracle
from lanczosnet_amd import ops
from lanczosnet_amd.model import LanczosNetGeneral
from lanczosnet_amd.utils.arg_helper import make_model_config

CFG = dict(num_bond_type=1, short_diffusion_dist=[], long_diffusion_dist=[1, 2, 3, 5, 7, 10, 20, 30],
           num_eig_vec=20, spectral_filter_kind='MLP', input_dim=10, hidden_dim=[128] * 7, output_dim=2,
           num_layer=7, num_atom=0)


def batch(B, seed):
  """Erdos-Renyi graphs of 20..100 nodes (dataset/get_graph_data.py:15-49), one of them of 100."""
  rs = np.random.RandomState(seed)
  N = 100
  ns = rs.randint(20, N + 1, size=B)
  ns[0] = N
  adj = np.zeros((B, N, N, 1), np.float32)
  for b in range(B):
    n = int(ns[b])
    a = np.triu((rs.rand(n, n) < 0.3).astype(np.float32), 1)
    adj[b, :n, :n, 0] = a + a.T
  mask = (np.arange(N)[None, :] < ns[:, None]).astype(np.uint8)
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  n = t(ns.astype(np.int32))
  L = ops.laplacian_l4(t(adj), n)
  D, V = ops.lanczos_ritz(L[..., 0], n, CFG['num_eig_vec'])
  X = t(rs.randn(B, N, CFG['input_dim']).astype(np.float32) * mask[:, :, None])
  return X, L, D, V, t(rs.randn(B, CFG['output_dim']).astype(np.float32)), t(mask)


def make_step(impl, data):
  net = LanczosNetGeneral(make_model_config(CFG, general=True)).train()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in
                       oracle.make_lanczosnet_params(CFG, 1, general=True).items()})
  net = net.cuda()
  net.mid_backward_impl = impl
  opt = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True)
  X, L, D, V, label, mask = data

  def step():
    opt.zero_grad(set_to_none=True)
    _, loss = net(X, L, D, V, label=label, mask=mask)
    loss.backward()
    opt.step()
    return loss
  return step


def window(step, steps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(steps):
    step()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / steps * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--steps', type=int, default=30)
  ap.add_argument('--batch', type=int, nargs='*', default=[10, 64])
  ap.add_argument('--only', choices=['torch', 'hip'])
  ap.add_argument('--out')
  a = ap.parse_args()
  if a.only:
    step = make_step(a.only, batch(a.batch[0], 0))
    for _ in range(a.steps):
      loss = step()
    torch.cuda.synchronize()
    print(json.dumps({'only': a.only, 'B': a.batch[0], 'steps_run': a.steps, 'loss': float(loss),
                      'backward_kernel': ops.last_kernel()}))
    return
  res = []
  for B in a.batch:
    data = batch(B, 0)
    steps = {impl: make_step(impl, data) for impl in ('torch', 'hip')}
    kernel = {}
    for impl, st in steps.items():
      for _ in range(3):
        loss = st()
      torch.cuda.synchronize()
      kernel[impl] = ops.last_kernel() if hasattr(ops, 'forget_autograd_kernel') else ''
    # (a full cyclic collection is a ~75 ms pause: collected here, frozen; bench_train_step.py)
    gc.collect()
    gc.freeze()
    ms = {'torch': [], 'hip': []}
    for _ in range(a.reps):
      for impl in ('torch', 'hip'):
        ms[impl].append(window(steps[impl], a.steps))
    row = {'workload': 'LanczosNetGeneral graph configuration train step (fwd + bwd + Adam)', 'B': B,
           'reps': a.reps, 'steps_per_rep': a.steps}
    for impl in ('torch', 'hip'):
      v = sorted(ms[impl])
      row['mid_backward_' + impl] = {'step_ms_median': round(v[len(v) // 2], 4), 'step_ms_min': round(v[0], 4),
                                     'step_ms_max': round(v[-1], 4), 'windows_ms': [round(x, 4) for x in ms[impl]],
                                     'backward_kernel': kernel[impl]}
    res.append(row)
    print(json.dumps(row))
    gc.unfreeze()
  if a.out:
    with open(a.out, 'w') as f:
      json.dump({'device': torch.cuda.get_device_name(0), 'rows': res}, f, indent=1)
      f.write('\n')


if __name__ == '__main__':
  main()
