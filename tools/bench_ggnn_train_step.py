#!/usr/bin/env python
"""Secondary measurement: one TRAINING step of the GGNN baseline (forward + backward + `train.make_adam`
step) at the shape of the reference's config/qm8_ggnn.yaml (D 128, 7 channels, 15 propagation steps, 'avg',
input 64, 16 outputs) on the package's synthetic QM8 batch, 1 x MI355X — the opt-in route 'ggnn_hip_train'
(`LANCZOSNET_GGNN_BACKWARD=hip`: the forward kernel leaving the state trajectory + csrc/ggnn_grad.hip)
against the default route 'ggnn_torch' (switch off) on the same device in the same run, the two
alternating; HIP events around whole steps, medians over the repeats (and the step without
`optimizer.step()`); peak memory above the resident state; from one profiled step per route
(torch.profiler, a pass of its own) the number of kernel launches and the split of the device time over
the step kernel, the readout backward, the forward kernel, the library GEMMs (the weight gradients) and
the rest; and the parity of each route's gradients on the timed batch against float64 autograd through
the module's torch restatement.  Writes profiles/ggnn_train_step.json.  Not the headline bench (bench.py).

    python tools/bench_ggnn_train_step.py [--batches 64 1024] [--steps 20] [--warmup 5]
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
from lanczosnet_amd.model import GGNN  # noqa: E402
from lanczosnet_amd.synthetic import draw_batch  # noqa: E402
from lanczosnet_amd.train import make_adam  # noqa: E402
from tools.bench_ggnn import config  # noqa: E402

ROUTES = (('ggnn_torch', 'torch'), ('ggnn_hip_train', 'hip'))   # switch off, switch on
GROUPS = (('step_kernel', ('ggnn_backward_step_kernel',)),
          ('readout_backward', ('ggnn_readout_backward_kernel', 'partial_sum_kernel')),
          ('forward_kernel', ('ggnn_forward_kernel',)),
          ('linears', ('f32_linear_kernel',)),
          ('library_gemms', ('Cijk_', 'gemm', 'Gemm')))


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
  return float(np.median(times))


def profiled_step(step):
  """(kernel launches, device ms per group) of one step, or None where the profiler is not available"""
  try:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
      step()
      torch.cuda.synchronize()
    kernels = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
    if not kernels:
      return None
    dur = lambda e: float(getattr(e, 'device_time', 0.0) or getattr(e, 'cuda_time', 0.0)) / 1e3  # noqa: E731
    split = {name: 0.0 for name, _ in GROUPS}
    split['rest'] = 0.0
    for e in kernels:
      for name, keys in GROUPS:
        if any(k in e.name for k in keys):
          split[name] += dur(e)
          break
      else:
        split['rest'] += dur(e)
    rest = {}
    for e in kernels:
      if not any(k in e.name for _, keys in GROUPS for k in keys):
        n, ms = rest.get(e.name, (0, 0.0))
        rest[e.name] = (n + 1, ms + dur(e))
    top = sorted(rest.items(), key=lambda kv: -kv[1][1])[:6]
    return {'launches': len(kernels), 'device_ms': {k: round(v, 4) for k, v in split.items()},
            'rest_longest': [{'kernel': k[:96], 'launches': n, 'device_ms': round(ms, 4)}
                                   for k, (n, ms) in top]}
  except Exception as e:   # the measurement above stands without this pass
    return {'error': '%s: %s' % (type(e).__name__, e)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, nargs='+', default=[64, 1024])
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--no-profile', action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ggnn_train_step.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_ggnn_train_step.py needs the MI355X'
  torch.manual_seed(1234)
  base = GGNN(config()).train().cuda()
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  rows = []

  def write():
    out = {'workload': 'GGNN training step (forward + backward + Adam), config/qm8_ggnn.yaml shape (D 128, 7 '
                       'channels, 15 steps, avg), synthetic QM8 batch, fp32',
           'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
           'timing': 'HIP events around one whole step, median over the steps; the two routes alternate, two '
                     'rounds each, the lower median is reported; forward_backward_ms: the same step without '
                     'optimizer.step(); peak_bytes: max_memory_allocated above what is resident before the step; '
                     'launches / device_ms: one profiled step per route (torch.profiler); grad_rel_err_vs_float64: '
                     'the largest over the parameters of max |g - g64| / max |g64|, g64 = float64 autograd through '
                     'the torch restatement on the timed batch',
           'results': rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      json.dump(out, f, indent=1)
      f.write('\n')

  for B in args.batches:
    b = draw_batch(B, seed=0)
    L = ops.laplacian_l4(t(b['adjs']), t(b['n_nodes']))
    nf, mask, label = t(b['node_feat']), t(b['node_mask']), t(b['label'])
    steps, nets, fb = {}, {}, {}
    for route, impl in ROUTES:
      net = copy.deepcopy(base)
      net.ggnn_backward_impl = impl
      net._warned_torch_route = True   # the route is chosen on purpose here
      opt = make_adam(net.parameters(), lr=1e-4)

      def step(net=net, opt=opt):
        opt.zero_grad(set_to_none=True)
        score, loss = net(nf, L, label=label, mask=mask)
        loss.backward()
        opt.step()
        return loss

      def fwd_bwd(net=net, opt=opt):
        opt.zero_grad(set_to_none=True)
        score, loss = net(nf, L, label=label, mask=mask)
        loss.backward()
      steps[route], nets[route], fb[route] = step, net, fwd_bwd
    row = {'batch': B, 'nodes_padded': int(nf.shape[1])}
    # gradient parity on the timed batch, on copies of the untouched parameters
    net64 = copy.deepcopy(base).double()
    net64._warned_torch_route = True
    _, loss64 = net64(nf, L.double(), label=label.double(), mask=mask)
    loss64.backward()
    g64 = {k: p.grad for k, p in net64.named_parameters()}
    parity = {}
    for route, impl in ROUTES:
      probe = copy.deepcopy(base)
      probe.ggnn_backward_impl = impl
      probe._warned_torch_route = True
      _, loss = probe(nf, L, label=label, mask=mask)
      loss.backward()
      assert probe.last_route == route, (probe.last_route, route)
      parity[route] = max(float((p.grad.double() - g64[k]).abs().max()) / float(g64[k].abs().max())
                          for k, p in probe.named_parameters())
    row['grad_rel_err_vs_float64'] = parity
    del net64, g64, loss64, probe, loss
    torch.cuda.empty_cache()
    losses = {}
    for route, _ in ROUTES:
      losses[route] = float(steps[route]())
      assert nets[route].last_route == route, (nets[route].last_route, route)
    row['first_loss'] = losses
    med = {route: [] for route, _ in ROUTES}
    for _ in range(2):
      for route, _ in ROUTES:
        med[route].append(median_ms(steps[route], args.steps, args.warmup))
    for route, _ in ROUTES:
      row[route + '_ms'] = round(min(med[route]), 4)
      row[route + '_medians_ms'] = [round(x, 4) for x in med[route]]
      row[route + '_forward_backward_ms'] = round(median_ms(fb[route], args.steps, args.warmup), 4)
      torch.cuda.synchronize()
      torch.cuda.reset_peak_memory_stats()
      resident = torch.cuda.memory_allocated()
      steps[route]()
      torch.cuda.synchronize()
      row[route + '_peak_bytes'] = int(torch.cuda.max_memory_allocated() - resident)
    row['speedup'] = round(row['ggnn_torch_ms'] / row['ggnn_hip_train_ms'], 3)
    row['forward_backward_speedup'] = round(row['ggnn_torch_forward_backward_ms']
                                            / row['ggnn_hip_train_forward_backward_ms'], 3)
    row['peak_bytes_ratio'] = round(row['ggnn_hip_train_peak_bytes'] / max(row['ggnn_torch_peak_bytes'], 1), 3)
    row['molecules_per_s'] = round(B / row['ggnn_hip_train_ms'] * 1e3, 1)
    rows.append(row)
    write()
    if not args.no_profile:
      for route, _ in ROUTES:
        row[route + '_profile'] = profiled_step(steps[route])
      write()
    print(json.dumps(row))


if __name__ == '__main__':
  main()
