#!/usr/bin/env python
"""Secondary measurement: one TRAINING step of the MPNN baseline (forward + backward + `train.make_adam`
step) at the shape of the reference's config/qm8_mpnn.yaml (D 128, 7 channels, 7 propagation steps, 'avg',
input 64, 16 outputs, 10 Set2Vec steps) on the package's synthetic QM8 batch, 1 x MI355X — the opt-in route
'mpnn_hip_train' (`LANCZOSNET_MPNN_BACKWARD=hip`: the forward kernel leaving the state trajectory +
csrc/mpnn_grad.hip; Set2Vec and output_func by autograd) against the default route 'mpnn_torch' (switch off) on
the same device in the same run, the two alternating; HIP events around whole steps, medians over the repeats
(and the step without `optimizer.step()`); peak memory above the resident state; from one profiled step per
route (torch.profiler, a pass of its own) the number of kernel launches and the split of the device time over
the step kernel, the trajectory forward, the linears, the library GEMMs (the weight gradients; on 'mpnn_torch'
every product) and the rest; the Set2Vec + output_func autograd on its own (forward + backward from S_T: HIP
events and its profiled device time and launches — its share of the 'mpnn_hip_train' step); and the parity of
each route's gradients on the timed batch against float64 autograd through the module's torch restatement, with
the worst parameter, the median over the parameters and the number of edge pre-activations that the kernel's
float32 trajectory puts on the other side of a ReLU from float64 (each costs a whole term of a gradient).
No speed ratio is fixed in advance: the figures are written as they fall.  Writes
profiles/mpnn_train_step.json.  Not the headline bench (bench.py).

    python tools/bench_mpnn_train_step.py [--batches 64 1024] [--steps 20] [--warmup 5]
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
from lanczosnet_amd.model.set2set import set2vec_batched  # noqa: E402
from lanczosnet_amd.synthetic import draw_batch  # noqa: E402
from lanczosnet_amd.train import make_adam  # noqa: E402
from tools.bench_mpnn import config  # noqa: E402

ROUTES = (('mpnn_torch', 'torch'), ('mpnn_hip_train', 'hip'))   # switch off, switch on
GROUPS = (('step_kernel', ('mpnn_backward_step_kernel',)),
          ('forward_kernel', ('mpnn_forward_states_kernel', 'mpnn_forward_kernel')),
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
    rest = {}
    for e in kernels:
      for name, keys in GROUPS:
        if any(k in e.name for k in keys):
          split[name] += dur(e)
          break
      else:
        split['rest'] += dur(e)
        n, ms = rest.get(e.name, (0, 0.0))
        rest[e.name] = (n + 1, ms + dur(e))
    top = sorted(rest.items(), key=lambda kv: -kv[1][1])[:6]
    return {'launches': len(kernels), 'device_ms': {k: round(v, 4) for k, v in split.items()},
            'device_ms_total': round(sum(split.values()), 4),
            'rest_longest': [{'kernel': k[:96], 'launches': n, 'device_ms': round(ms, 4)} for k, (n, ms) in top]}
  except Exception as e:   # the measurement above stands without this pass
    return {'error': '%s: %s' % (type(e).__name__, e)}


@torch.no_grad()
def relu_sign_flips(net64, net, nf, L):
  """(edge pre-activations Q_c[a] + P_c[b] of the batch over all steps, those with |value| < 2e-6 in float64, those
  whose sign differs between the float64 trajectory (the module's restatement, step by step) and the kernel's
  float32 trajectory, both evaluated in float64).  One of the last costs a whole term of a gradient."""
  B, N = nf.shape
  C, D = net64.num_edgetype + 1, net64.hidden_dim
  A = (L != 0).permute(0, 3, 1, 2)
  Ad = A.double()
  deg = Ad.sum(dim=3, keepdim=True)
  eps = float(np.finfo(np.float32).eps)

  def pre(S, c):
    lin1 = net64.edge_func[c][0]
    return (S @ lin1.weight[:, D:].t() + lin1.bias).unsqueeze(2) + (S @ lin1.weight[:, :D].t()).unsqueeze(1)
  table, prop, _ = net._packs()
  S32 = ops.mpnn_forward_states(table[nf], L, *prop, net.num_prop, avg=net.aggregate_type == 'avg')
  state = net64.input_func(net64.node_embedding(nf))
  total = close = flips = 0
  for step in range(net64.num_prop):
    msg = []
    for c in range(C):
      on = A[:, c].unsqueeze(3)
      p64, p32 = pre(state, c), pre(S32[step].double(), c)
      total += int(on.sum()) * p64.shape[3]
      close += int(((p64.abs() < 2e-6) & on).sum())
      flips += int((((p64 > 0) != (p32 > 0)) & on).sum())
      lin2 = net64.edge_func[c][2]
      Mc = (torch.relu(p64) * Ad[:, c].unsqueeze(3)).sum(dim=2) @ lin2.weight.t() + deg[:, c] * lin2.bias
      msg.append(Mc / (deg[:, c] + eps) if net64.aggregate_type == 'avg' else Mc)
    state = net64.update_func(torch.cat(msg, dim=2).view(B * N, C * D), state.reshape(B * N, D)).view(B, N, D)
  return {'edge_preactivations': total, 'float64_below_2e-6': close, 'sign_differs_float64_vs_kernel': flips}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, nargs='+', default=[64, 1024])
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--no-profile', action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpnn_train_step.json'))
  args = ap.parse_args()
  assert torch.cuda.is_available(), 'bench_mpnn_train_step.py needs the MI355X'
  torch.manual_seed(1234)
  base = MPNN(config()).train().cuda()
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  rows = []

  def write():
    out = {'workload': 'MPNN training step (forward + backward + Adam), config/qm8_mpnn.yaml shape (D 128, 7 '
                       'channels, 7 steps, avg, Set2Vec 10 steps), synthetic QM8 batch, fp32',
           'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
           'timing': 'HIP events around one whole step, median over the steps; the two routes alternate, two '
                     'rounds each, the lower median is reported; forward_backward_ms: the same step without '
                     'optimizer.step(); peak_bytes: max_memory_allocated above what is resident before the step; '
                     'launches / device_ms: one profiled step per route (torch.profiler); set2vec_autograd: Set2Vec '
                     'and output_func forward + backward by autograd from S_T alone, the part of route '
                     'mpnn_hip_train that no HIP kernel serves; grad_rel_err_vs_float64: the largest over the '
                     'parameters of max |g - g64| / max |g64|, g64 = float64 autograd through the torch '
                     'restatement on the timed batch; relu_kinks: the edge pre-activations Q_c[a] + P_c[b] of the '
                     'batch over all steps, those within 2e-6 of zero in float64, and those whose sign differs '
                     'between the float64 trajectory and the kernel float32 trajectory (each is a whole term of a '
                     'gradient on a float32 route)',
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
      net.mpnn_backward_impl = impl
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
    parity, worst, middle = {}, {}, {}
    for route, impl in ROUTES:
      probe = copy.deepcopy(base)
      probe.mpnn_backward_impl = impl
      probe._warned_torch_route = True
      _, loss = probe(nf, L, label=label, mask=mask)
      loss.backward()
      assert probe.last_route == route, (probe.last_route, route)
      errs = {k: float((p.grad.double() - g64[k]).abs().max()) / float(g64[k].abs().max())
              for k, p in probe.named_parameters()}
      parity[route] = max(errs.values())
      worst[route] = max(errs, key=errs.get)
      middle[route] = float(np.median(list(errs.values())))
    row['grad_rel_err_vs_float64'] = parity
    # a ReLU of the edge network that float32 puts on the other side of zero from float64 costs a whole term of
    # the first Linear's gradient (either route): the worst parameter and the median tell that from a wrong kernel
    row['grad_rel_err_worst_parameter'] = worst
    row['grad_rel_err_median_over_parameters'] = middle
    row['relu_kinks'] = relu_sign_flips(net64, probe, nf, L)
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
    row['speedup'] = round(row['mpnn_torch_ms'] / row['mpnn_hip_train_ms'], 3)
    row['forward_backward_speedup'] = round(row['mpnn_torch_forward_backward_ms']
                                            / row['mpnn_hip_train_forward_backward_ms'], 3)
    row['peak_bytes_ratio'] = round(row['mpnn_hip_train_peak_bytes'] / max(row['mpnn_torch_peak_bytes'], 1), 3)
    row['molecules_per_s'] = round(B / row['mpnn_hip_train_ms'] * 1e3, 1)

    # Set2Vec + output_func by autograd from S_T alone: what route 'mpnn_hip_train' leaves to torch
    net = nets['mpnn_hip_train']
    with torch.no_grad():
      table, prop, _ = net._packs()
      S_T = ops.mpnn_forward(table[nf], L, *prop, net.num_prop, avg=True)

    def readout():
      x = S_T.detach().requires_grad_(True)
      score = net.output_func(set2vec_batched(net.att_func, x, mask))
      net.loss_func(score, label).backward()
      net.zero_grad(set_to_none=True)
    row['set2vec_autograd_forward_backward_ms'] = round(median_ms(readout, args.steps, args.warmup), 4)
    row['set2vec_autograd_share_of_forward_backward'] = round(
        row['set2vec_autograd_forward_backward_ms'] / row['mpnn_hip_train_forward_backward_ms'], 3)
    rows.append(row)
    write()
    if not args.no_profile:
      for route, _ in ROUTES:
        row[route + '_profile'] = profiled_step(fb[route])
      row['set2vec_autograd_profile'] = profiled_step(readout)
      write()
    print(json.dumps(row))


if __name__ == '__main__':
  main()
