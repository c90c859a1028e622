#!/usr/bin/env python
"""Several edge types on the large-graph sparse path, measured on the MI355X: BASELINE config 5's graphs
(B 256, N 2048, G(n, 0.01), K = M = 64) with E = 2 uniformly random edge types, bf16 mode.

Steps, each in a child process of its own under its own time limit (a step that fails ends the run):
  typed     dataset.collate_graph_edges(num_edge_type=2) (wall clock to a device synchronise), the module's
            forward on the typed SparseLaplacian, and ONE lnz_large_sparse_conv_channels[_f32] launch (R = 3)
  streamed  the comparison line — the route such a batch took before: `sl.to_dense()`, forward with the
            sparse layers off (three operators packed and streamed), and ONE lnz_large_conv launch (C = 3)
  each      the dense tensor with large_sparse_channels = 'each': forward (the image pass included) and ONE
            lnz_large_sparse_image_channels launch
Device events, warm, min / median / max over five windows (a window of a single launch is `reps` launches,
reported per launch).

    python tools/bench_typed_edges.py [--batch 256] [--windows 5] [--out profiles/typed_edges_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tools.bench_edge_collate import gnp_edges, stats  # noqa: E402

SHAPE = dict(N=2048, p=0.01, M=64, K=64, E=2)
LIMITS = dict(typed=240, streamed=300, each=300)   # seconds per step
DEV = 'cuda:0'


def net_for(K, E, **attrs):
  import torch
  import oracle
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  cfg = dict(num_bond_type=E, short_diffusion_dist=[], long_diffusion_dist=[1, 2, 3, 5, 7, 10, 20, 30], num_eig_vec=K,
             spectral_filter_kind='MLP', input_dim=10, hidden_dim=[128] * 7, output_dim=2, num_layer=7, num_atom=0)
  P = oracle.make_lanczosnet_params(cfg, 17, general=True)
  net = LanczosNetGeneral(make_model_config(cfg, general=True)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV)
  net.gemm_mode = 'bf16'
  for k, v in attrs.items():
    setattr(net, k, v)
  return net


def items_for(B):
  s = SHAPE
  rs = np.random.RandomState(5)
  graphs = [gnp_edges(s['N'], s['p'], rs) for _ in range(B)]
  return [dict(edges=g, edge_type=rs.randint(0, s['E'], size=g.shape[0]).astype(np.int32),
               node_feat=rs.randn(s['N'], 10).astype(np.float32), label=np.zeros((1, 2))) for g in graphs]


def timed(fn, windows, reps=1):
  import torch
  ms = []
  for w in range(windows + 1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
      out = fn()
    e1.record()
    torch.cuda.synchronize()
    if w:   # (window 0 warms code objects, plans and the allocator)
      ms.append(e0.elapsed_time(e1) / reps)
  return stats(ms), out


def forward_of(net, b, L):
  import torch

  def run():
    with torch.no_grad():
      return net(b['node_feat'], L, b['D'], b['V'], mask=b['node_mask'])
  return run


def step(name, B, windows):
  import torch
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_edges
  s = SHAPE
  N, K, E, R = s['N'], s['K'], s['E'], s['E'] + 1
  its = items_for(B)
  rec = dict(B=B)
  collate_ms = []
  for w in range(windows + 1 if name == 'typed' else 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = collate_graph_edges(its, K, device=DEV, lanczos_steps=s['M'], num_edge_type=E)
    torch.cuda.synchronize()
    if w:
      collate_ms.append((time.perf_counter() - t0) * 1e3)
  sl = b['L']
  X = torch.randn((B, N, 128), device=DEV)
  if name == 'typed':
    rec['collate_ms'] = stats(collate_ms)
    rec['image_flags'] = int(sl.images.flags.item())
    rec['entries_per_row'] = [float(sl.images.counts[c].float().mean()) for c in range(R)]
    net = net_for(K, E)
    rec['forward_ms'], score = timed(forward_of(net, b, sl), windows)
    rec['kernel'] = ops.last_kernel()
    Z = torch.randn((R, B, N, 128), device=DEV).to(torch.bfloat16)
    im = sl.images
    rec['gather_bf16_ms'], _ = timed(lambda: ops._abi().large_sparse_conv_channels(im.entries, im.counts, im.cap, Z, B,
                                                                                    N, R, 1, X), windows, reps=10)
    Zf = Z.float()
    rec['gather_f32_ms'], _ = timed(lambda: ops._abi().large_sparse_conv_channels_f32(
        im.entries, im.values, im.counts, im.cap, Zf, B, N, R, 1, X), windows, reps=10)
  else:
    L = sl.to_dense()
    b['L'] = sl = None
    rec['dense_L_bytes'] = int(L.numel() * 4)
    if name == 'streamed':
      net = net_for(K, E, large_sparse=False)
      rec['forward_ms'], score = timed(forward_of(net, b, L), windows)
      rec['sparse_state'] = bool(getattr(net, '_large_sparse_state', {}))   # (False: the streamed kernels served it)
      Lb, Vb = ops.large_pack_operators(L, b['V'], 1)
      Zt, Tt, _ = ops.large_work_buffers(Lb)
      bias = torch.zeros((128,), device=DEV)
      rec['streamed_conv_ms'], _ = timed(lambda: ops.large_conv(Lb, Vb, Zt, Tt, bias, out=X), windows, reps=10)
    else:
      net = net_for(K, E, large_sparse_channels='each')
      rec['forward_ms'], score = timed(forward_of(net, b, L), windows)
      rec['kernel'] = ops.last_kernel()
      rec['last_flags'] = net._large_sparse_state[torch.device(DEV).index]['last_flags']
      rec['image_channels_ms'], _ = timed(lambda: ops.large_sparse_image_channels(L), windows)
  rec['score_checksum'] = float(score.double().abs().sum())
  return rec


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=256)
  ap.add_argument('--windows', type=int, default=5)
  ap.add_argument('--steps', default='typed,streamed,each')
  ap.add_argument('--step', default=None, help='(internal) run one step in this process')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'typed_edges_bench.json'))
  args = ap.parse_args()
  warnings.simplefilter('ignore')
  if args.step:
    import torch
    if not torch.cuda.is_available():
      raise SystemExit('bench_typed_edges: needs the MI355X (no CPU fallback)')
    rec = step(args.step, args.batch, args.windows)
    with open(args.out, 'w') as f:
      json.dump(rec, f)
    return
  result = dict(shape=dict(SHAPE, B=args.batch), windows=args.windows, steps={})
  for name in args.steps.split(','):
    with tempfile.TemporaryDirectory() as tmp:
      part = os.path.join(tmp, 'step.json')
      cmd = [sys.executable, os.path.abspath(__file__), '--step', name, '--batch', str(args.batch), '--windows',
             str(args.windows), '--out', part]
      try:
        r = subprocess.run(cmd, timeout=LIMITS[name], capture_output=True, text=True)
      except subprocess.TimeoutExpired:
        result['steps'][name] = dict(error='time limit of %d s' % LIMITS[name])
        break   # (nothing more is started on the GPU behind a step that did not end)
      if r.returncode != 0 or not os.path.exists(part):
        result['steps'][name] = dict(error='exit %d: %s' % (r.returncode, r.stderr.strip().splitlines()[-1:]))
        break
      result['steps'][name] = json.load(open(part))
    print(json.dumps({name: result['steps'][name]}), flush=True)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
