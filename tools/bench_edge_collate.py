#!/usr/bin/env python
"""Raw graphs -> scores through the dense collate (dataset.collate_graph_adjacency + forward) and
through the edge-list collate (dataset.collate_graph_edges + forward), on the MI355X.

Shapes: BASELINE config 5's graphs (B 256, N 2048, G(n, 0.01), K 64) and the wide corner
(B 4, N 8192, M 128, K 64).  Per shape and route, warm, min / median / max over five windows:
  collate_ms        wall clock around the collate, ending in a device synchronise (it holds host work)
  forward_ms        device events around the module's forward (bf16 mode)
  peak_bytes        torch.cuda.max_memory_allocated of collate + forward
and, device events around the entries with M = K = 1 (the image build and ONE Lanczos step):
  edges_build_ms    lnz_lanczos_ritz_kstep[_wide]_edges     (csrc/edge_image.hip: init, scatter, rows, finish, pad)
  dense_build_ms    lnz_lanczos_ritz_kstep_image / _wide on the dense L in place (ell_compact_rows_kernel + ell_pad_kernel)
A route that the library does not serve at a shape is recorded with its error, not skipped silently.

    python tools/bench_edge_collate.py [--shapes config5,wide] [--windows 5] [--out profiles/edge_collate_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

SHAPES = {'config5': dict(B=256, N=2048, p=0.01, M=64, K=64), 'wide': dict(B=4, N=8192, p=0.0025, M=128, K=64)}


def gnp_edges(n, p, rs):
  m = int(round(p * n * (n - 1) / 2))
  u, v = rs.randint(0, n, size=2 * m + 16), rs.randint(0, n, size=2 * m + 16)
  keep = u != v
  code = np.unique(np.minimum(u, v)[keep].astype(np.int64) * n + np.maximum(u, v)[keep])
  code = code[rs.permutation(code.shape[0])[:m]]
  return np.stack([code // n, code % n], axis=1).astype(np.int32)


def stats(xs):
  xs = sorted(xs)
  return dict(min=xs[0], median=xs[len(xs) // 2], max=xs[-1])


def net_for(K, dev):
  import torch
  import oracle
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  cfg = dict(num_bond_type=1, short_diffusion_dist=[], long_diffusion_dist=[1, 2, 3, 5, 7, 10, 20, 30], num_eig_vec=K,
             spectral_filter_kind='MLP', input_dim=10, hidden_dim=[128] * 7, output_dim=2, num_layer=7, num_atom=0)
  P = oracle.make_lanczosnet_params(cfg, 17, general=True)
  net = LanczosNetGeneral(make_model_config(cfg, general=True)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(dev)
  net.gemm_mode = 'bf16'
  return net


def route(collate, items, K, M, net, dev, windows):
  """collate + forward: one warm pass, then `windows` timed ones."""
  import torch
  out = dict(collate_ms=[], forward_ms=[])
  for w in range(windows + 1):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    b = collate(items, K, device=dev, lanczos_steps=M)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
      e0.record()
      score = net(b['node_feat'], b['L'], b['D'], b['V'], mask=b['node_mask'])
      e1.record()
    torch.cuda.synchronize()
    if w:   # (window 0 warms code objects, plans and the allocator)
      out['collate_ms'].append((t1 - t0) * 1e3)
      out['forward_ms'].append(e0.elapsed_time(e1))
      out['peak_bytes'] = int(torch.cuda.max_memory_allocated() - base)
    out['image_from'] = net._large_sparse_state[torch.device(dev).index].get('image_from')
    out['score_checksum'] = float(score.double().abs().sum())
    del b, score
  out['collate_ms'], out['forward_ms'] = stats(out['collate_ms']), stats(out['forward_ms'])
  return out


def timed(fn, windows):
  import torch
  ms = []
  for w in range(windows + 1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    if w:
      ms.append(e0.elapsed_time(e1))
  return stats(ms)


def build_times(graphs, s, dev, windows):
  """The entries with M = K = 1: the image build and one Lanczos step, edges against the dense L in place."""
  import torch
  from lanczosnet_amd import ops
  B, N = s['B'], s['N']
  wide = N > ops.KSTEP_MAX_N
  cap, ccap = ops.kstep_row_cap(N), ops.large_sparse_row_cap(N)
  edges = torch.from_numpy(np.concatenate(graphs)).to(dev)
  off = np.zeros(B + 1, np.int64)
  np.cumsum([g.shape[0] for g in graphs], out=off[1:])
  off, n = torch.from_numpy(off).to(dev), torch.full((B,), N, dtype=torch.int32, device=dev)
  D, V = torch.empty((B, 1), device=dev), torch.empty((B, N, 1), device=dev)
  i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)   # noqa: E731
  status, over, ent, cnt, flg = i32(B), i32(B), i32(B, N, ccap), i32(B, N), i32(1)
  val = torch.empty((B, N, ccap), device=dev)
  abi = ops._abi()
  ro, co = ops.dense_entry_orders(N)
  if wide:
    need = abi.lanczos_ritz_kstep_wide_edges_workspace_bytes(B, N, 1, cap, ccap)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    run_e = lambda: abi.lanczos_ritz_kstep_wide_edges(edges, edges.shape[0], off, n, B, N, 1, 1, cap, ro, ws, need, D,   # noqa: E731
                                                      V, None, over, ent, val, cnt, ccap, co, flg, status)
  else:
    need = abi.lanczos_ritz_kstep_edges_workspace_bytes(B, N, cap, ccap)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    run_e = lambda: abi.lanczos_ritz_kstep_edges(edges, edges.shape[0], off, n, B, N, 1, 1, cap, ro, ws, need, D, V,   # noqa: E731
                                                 None, over, ent, val, cnt, ccap, co, flg, status)
  out = dict(edges_build_ms=timed(run_e, windows), edges_status=int(status.abs().sum()), edges_over=int(over.sum()))
  del ws
  # the dense L of the same graphs, channels last, built with torch ops (only its time to compact matters here)
  L = torch.zeros((B, N, N, 2), device=dev)
  for b, g in enumerate(graphs):
    e = torch.from_numpy(g).to(dev).long()
    A = torch.zeros((N, N), dtype=torch.float64, device=dev)
    A[e[:, 0], e[:, 1]] = 1.0
    A[e[:, 1], e[:, 0]] = 1.0
    A += torch.eye(N, dtype=torch.float64, device=dev)
    sdeg = 1.0 / A.sum(1).sqrt()
    L[b] = ((sdeg[:, None] * A) * sdeg[None, :]).float()[:, :, None]
    del A
  A0 = L[..., 0]
  if wide:
    need = abi.lanczos_ritz_kstep_wide_workspace_bytes(B, N, 1, cap)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    run_d = lambda: abi.lanczos_ritz_kstep_wide(A0, A0.stride(0), A0.stride(1), A0.stride(2), n, B, N, 1, 1, cap, ws,   # noqa: E731
                                                need, D, V, None, over)
  else:
    need = abi.lanczos_ritz_kstep_workspace_bytes(B, N, 3, cap)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    run_d = lambda: abi.lanczos_ritz_kstep_image(A0, A0.stride(0), A0.stride(1), A0.stride(2), n, B, N, 1, 1, 3, cap, ws,   # noqa: E731
                                                 need, D, V, None, over, ent, val, cnt, ccap, flg)
  out['dense_build_ms'] = timed(run_d, windows)
  out['dense_L_bytes'] = int(L.numel() * 4)
  out['edge_bytes'] = int(edges.numel() * 4)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='config5,wide')
  ap.add_argument('--windows', type=int, default=5)
  ap.add_argument('--batch', type=int, default=0, help='override B (0: the shape\'s own)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'edge_collate_bench.json'))
  args = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    raise SystemExit('bench_edge_collate: needs the MI355X (no CPU fallback)')
  from lanczosnet_amd.dataset import collate_graph_adjacency, collate_graph_edges
  dev = 'cuda:0'
  result = dict(device=torch.cuda.get_device_name(0), windows=args.windows, shapes={})
  warnings.simplefilter('ignore')
  for name in args.shapes.split(','):
    s = dict(SHAPES[name])
    if args.batch:
      s['B'] = args.batch
    rs = np.random.RandomState(5)
    graphs = [gnp_edges(s['N'], s['p'], rs) for _ in range(s['B'])]
    feats = [rs.randn(s['N'], 10).astype(np.float32) for _ in range(s['B'])]
    rec = dict(s, edges_per_graph=int(np.mean([g.shape[0] for g in graphs])),
               longest_row=int(max(np.bincount(g.reshape(-1)).max() for g in graphs) + 1))
    net = net_for(s['K'], dev)
    items = [dict(edges=g, node_feat=x, label=np.zeros((1, 2))) for g, x in zip(graphs, feats)]
    rec['edges'] = route(collate_graph_edges, items, s['K'], s['M'], net, dev, args.windows)
    try:
      dense = []
      for g, x in zip(graphs, feats):
        a = np.zeros((s['N'], s['N'], 1), np.float32)
        a[g[:, 0], g[:, 1], 0] = 1.0
        a[g[:, 1], g[:, 0], 0] = 1.0
        dense.append(dict(adjs=a, node_feat=x, label=np.zeros((1, 2))))
      rec['dense'] = route(collate_graph_adjacency, dense, s['K'], s['M'], net, dev, args.windows)
    except Exception as e:   # noqa: BLE001  (recorded: the dense collate does not reach every shape)
      rec['dense'] = dict(error='%s: %s' % (type(e).__name__, str(e).splitlines()[0][:300]))
    dense = None
    rec['build'] = build_times(graphs, s, dev, args.windows)
    result['shapes'][name] = rec
    print(json.dumps({name: rec}))
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print('wrote', args.out)


if __name__ == '__main__':
  main()
