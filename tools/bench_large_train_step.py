#!/usr/bin/env python
"""One training step (forward + backward + Adam) of LanczosNetGeneral on large graphs from edge lists,
on the MI355X: the densify + autograd route (`large_backward_impl = 'torch'`, the default) against the
opt-in HIP backward on the sparse image (`'hip'`: `_LargeSparseFusedFunction`, csrc/conv_sparse_grad.hip;
DESIGN.md §4.9c), in the same run on the same batch.

Shapes: BASELINE config 5's graphs from edge lists (B 256, N 2048, G(n, 0.01), K 64, 7 x 128 — the
generator of tools/bench_edge_collate.py) and the wide corner (B 4, N 8192, M 128, K 64), which has no
dense form: the torch route is recorded there with its error, not skipped silently.
Per shape and route, warm: step_ms min / median / max over `--windows` windows of `--steps` steps (device
events around a window; the cyclic collector is collected and frozen outside the windows, as in
tools/bench_train_step.py) and peak_bytes = torch.cuda.max_memory_allocated above the resident batch,
parameters and optimizer state.

TYPED shapes (`typed`: config 5's graphs, `typed_wide`: the wide corner — (E + 1) N beyond `to_dense`'s limit, the
switch on only —, each with two edge types drawn per edge): the same two routes under the typed switch
(`large_typed_backward_impl`: the same Function on R = 3 operators), and one layer's split gather
(lnz_large_sparse_conv_split_f32) beside R launches of lnz_large_sparse_conv_f32 onto zeroed buffers on the same
operands.  They are written to profiles/large_typed_train_step.json.

DENSE shape (`dense`: config 5's graphs through `collate_graph_adjacency`, L a [B,N,N,2] float32 tensor): the dense
switch (`large_dense_backward_impl`) off — the parent's route, bit for bit: the yardstick — and on,
in the same run on the same batch; the image pass's and the symmetry kernel's own times from device events; and
the edge-list HIP step of the same graphs beside them.  Written to profiles/large_dense_train_step.json.

    python tools/bench_large_train_step.py [--shapes config5,wide | typed,typed_wide | dense] [--windows 3]
                                           [--steps 2] [--batch B] [--out profiles/large[_typed|_dense]_train_step.json]
"""
import argparse
import gc
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tools.bench_edge_collate import SHAPES, gnp_edges, stats  # noqa: E402


TYPED = {'typed': 'config5', 'typed_wide': 'wide'}   # typed shape -> the graphs it types
TYPED_E = 2


def net_for(K, dev, impl, E=1, dense=False):
  import torch
  import oracle
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  cfg = dict(num_bond_type=E, short_diffusion_dist=[], long_diffusion_dist=[1, 2, 3, 5, 7, 10, 20, 30], num_eig_vec=K,
             spectral_filter_kind='MLP', input_dim=10, hidden_dim=[128] * 7, output_dim=2, num_layer=7, num_atom=0)
  P = oracle.make_lanczosnet_params(cfg, 17, general=True)
  net = LanczosNetGeneral(make_model_config(cfg, general=True)).train()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(dev)
  net.gemm_mode = 'fp32'
  net.large_backward_impl = impl if E == 1 and not dense else 'torch'
  net.large_typed_backward_impl = impl if E > 1 and not dense else 'torch'
  net.large_dense_backward_impl = impl if dense else 'torch'
  return net


def gather_record(imgs, reps=10):
  """One layer's dZ_c = L_c dP for all R channels: the split gather against R one-operator gathers onto zeroed
  buffers (the zero fill inside the timed region: it is part of that composition), the same operands."""
  import torch
  from lanczosnet_amd import ops
  R, B, N = imgs.R, imgs.B, imgs.N
  P = torch.randn((B, N, 128), device=imgs.entries.device)
  out, ref = torch.empty((R, B, N, 128), device=P.device), torch.empty((R, B, N, 128), device=P.device)
  chans = [imgs.channel(c) for c in range(R)]

  def split():
    ops.large_sparse_conv_split(imgs, P, out=out)

  def composed():
    ref.zero_()
    for c, im in enumerate(chans):
      ops._abi().large_sparse_conv_f32(im.entries, im.values, im.counts, im.cap, P, B, N, 0, ref[c])
  rec = {}
  for name, fn in (('split_gather_ms', split), ('r_launches_onto_zeros_ms', composed)):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      fn()
      e1.record()
      torch.cuda.synchronize()
      ms.append(e0.elapsed_time(e1))
    rec[name] = stats([round(x, 4) for x in ms])
  rec['same_bits'] = bool(torch.equal(out, ref))
  rec['split_over_r_launches'] = round(rec['split_gather_ms']['median'] / rec['r_launches_onto_zeros_ms']['median'], 4)
  return rec


def route(impl, b, K, dev, windows, steps, E=1, dense=False):
  """-> the record of one route on the resident batch `b`: one warm step, then the timed windows."""
  import torch
  from lanczosnet_amd import ops
  net = net_for(K, dev, impl, E, dense)
  opt = torch.optim.Adam(net.parameters(), lr=1e-4)

  def step():
    opt.zero_grad(set_to_none=True)
    _, loss = net(b['node_feat'], b['L'], b['D'], b['V'], label=b['label'], mask=b['node_mask'])
    loss.backward()
    opt.step()
    return loss
  loss = step()   # (code objects, plans, the allocator, Adam's state)
  torch.cuda.synchronize()
  out = dict(backward_kernel=ops.last_kernel(), first_loss=float(loss))
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  gc.collect()
  gc.freeze()
  ms = []
  for _ in range(windows):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
      loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1) / steps)
  gc.unfreeze()
  out.update(step_ms=stats(ms), windows_ms=[round(x, 4) for x in ms], steps_per_window=steps,
             peak_bytes=int(torch.cuda.max_memory_allocated() - base), last_loss=float(loss))
  return out


def timed(fn, reps=10):
  """ms of fn() from device events around each of `reps` calls, after one warm call."""
  import torch
  fn()
  torch.cuda.synchronize()
  ms = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    ms.append(round(e0.elapsed_time(e1), 4))
  return stats(ms)


def dense_shape(s, args, dev):
  """config 5's graphs as the dense collate's batch: switch off / on, the two kernels alone, the edge-list step."""
  import torch
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_adjacency, collate_graph_edges
  rs = np.random.RandomState(5)
  N = s['N']
  graphs = [gnp_edges(N, s['p'], rs) for _ in range(s['B'])]
  feats = [(rs.randn(N, 10).astype(np.float32), rs.randn(1, 2)) for _ in graphs]
  rec = dict(s, edges_per_graph=int(np.mean([g.shape[0] for g in graphs])), dense_L_bytes=int(s['B'] * N * N * 4 * 2))

  def adjacency(g):
    A = np.zeros((N, N, 1), np.float32)
    A[g[:, 0], g[:, 1], 0] = 1.0
    A[g[:, 1], g[:, 0], 0] = 1.0
    return A
  b = collate_graph_adjacency([dict(adjs=adjacency(g), node_feat=x, label=y) for g, (x, y) in zip(graphs, feats)],
                              s['K'], device=dev, lanczos_steps=s['M'])
  L = b['L']
  riding = ops.attached_sparse_image(L)
  rec['image_rides_on_L'] = riding is not None and riding.values is not None
  # the two kernels alone, on this batch
  out = {}

  def image():
    out['img'] = ops.large_sparse_image(L, values=True)

  def check():
    out['status'] = ops.large_sparse_image_symmetry(out['img'])
  rec['image_pass_ms'] = timed(image)
  rec['symmetry_ms'] = timed(check)
  img, status = out['img'], out['status']
  rec['image_flags'] = int(img.flags.item())
  rec['status_nonzero_words'] = int((status != 0).sum().item())
  rec['image_entries'] = int(img.counts.sum().item())
  rec['row_cap'] = img.cap
  del out, img, status
  torch.cuda.empty_cache()
  for impl in ('torch', 'hip'):
    rec['large_dense_backward_' + impl] = route(impl, b, s['K'], dev, args.windows, args.steps, dense=True)
    torch.cuda.empty_cache()
  del b, L, riding
  torch.cuda.empty_cache()
  be = collate_graph_edges([dict(edges=g, node_feat=x, label=y) for g, (x, y) in zip(graphs, feats)], s['K'],
                           device=dev, lanczos_steps=s['M'])
  rec['edge_list_backward_hip'] = route('hip', be, s['K'], dev, args.windows, args.steps)
  t, h, e = (rec[k] for k in ('large_dense_backward_torch', 'large_dense_backward_hip', 'edge_list_backward_hip'))
  rec['hip_over_torch'] = dict(step_ms=round(h['step_ms']['median'] / t['step_ms']['median'], 4),
                               peak_bytes=round(h['peak_bytes'] / t['peak_bytes'], 4))
  rec['dense_hip_minus_edge_list_hip_ms'] = round(h['step_ms']['median'] - e['step_ms']['median'], 4)
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='config5,wide')
  ap.add_argument('--windows', type=int, default=3)
  ap.add_argument('--steps', type=int, default=2)
  ap.add_argument('--batch', type=int, default=0, help="override B (0: the shape's own)")
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  names = args.shapes.split(',')
  kinds = {'typed' if n in TYPED else 'dense' if n == 'dense' else 'plain' for n in names}
  if len(kinds) != 1:
    raise SystemExit('bench_large_train_step: typed, dense and untyped shapes go to files of their own: one kind per run')
  typed, dense = kinds == {'typed'}, kinds == {'dense'}
  if args.out is None:
    args.out = os.path.join(ROOT, 'profiles', 'large_typed_train_step.json' if typed else
                            'large_dense_train_step.json' if dense else 'large_train_step.json')
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('bench_large_train_step: needs the MI355X (no CPU fallback)')
  from lanczosnet_amd.dataset import collate_graph_edges
  dev = 'cuda:0'
  result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, workload='LanczosNetGeneral 7 x 128, '
                'eight long scales, train step (fwd + bwd + Adam), graphs from edge lists', shapes={})
  warnings.simplefilter('ignore')
  if dense:
    result['workload'] += ' and as the dense collated L'
  for name in names:
    s = dict(SHAPES[TYPED.get(name, 'config5' if dense else name)])
    E = TYPED_E if typed else 1
    if args.batch:
      s['B'] = args.batch
    if dense:
      result['shapes'][name] = rec = dense_shape(s, args, dev)
      print(json.dumps({name: rec}))
      continue
    rs = np.random.RandomState(5)
    graphs = [gnp_edges(s['N'], s['p'], rs) for _ in range(s['B'])]
    items = [dict(edges=g, node_feat=rs.randn(s['N'], 10).astype(np.float32), label=rs.randn(1, 2)) for g in graphs]
    rec = dict(s, edges_per_graph=int(np.mean([g.shape[0] for g in graphs])),
               dense_L_bytes=int(s['B'] * s['N'] * s['N'] * 4 * (E + 1)))
    if typed:
      for it, g in zip(items, graphs):
        it['edge_type'] = rs.randint(0, E, size=g.shape[0])
      rec['num_edge_type'] = E
    b = collate_graph_edges(items, s['K'], device=dev, lanczos_steps=s['M'], num_edge_type=E)
    rec['image_flags'] = int(b['L'].image.flags.item())
    if typed:
      rec['gather'] = gather_record(b['L'].images)
    impls = ('hip',) if name == 'typed_wide' else ('torch', 'hip')
    for impl in impls:
      try:
        rec['large_backward_' + impl] = route(impl, b, s['K'], dev, args.windows, args.steps, E)
      except Exception as e:   # noqa: BLE001  (recorded: the densify route does not reach every shape)
        gc.unfreeze()
        rec['large_backward_' + impl] = dict(error='%s: %s' % (type(e).__name__, str(e).splitlines()[0][:300]))
      torch.cuda.empty_cache()
    t, h = rec.get('large_backward_torch', {}), rec['large_backward_hip']
    if 'step_ms' in t and 'step_ms' in h:
      rec['hip_over_torch'] = dict(step_ms=round(h['step_ms']['median'] / t['step_ms']['median'], 4),
                                   peak_bytes=round(h['peak_bytes'] / t['peak_bytes'], 4))
    result['shapes'][name] = rec
    print(json.dumps({name: rec}))
    del b
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
