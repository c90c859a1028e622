#!/usr/bin/env python
"""The full eigendecomposition (ops.sym_eigh_topk -> lnz_sym_eigh_topk) on BASELINE config 5's
graphs — G(n, 0.01), N = 2048, K = 64 — at B = 256 and at a small batch (B = 4), beside the two
other ways this project has to the same pairs: the vendor eigensolver branch
(utils/data_helper._full_decomposition_library, torch.linalg.eigh in fp64) and the K-step Lanczos
product path (ops.lanczos_ritz_collated, a different function for the trailing pairs).

Prints one JSON object (also written to --out): wall times per call, and the algorithmic bytes of
the tridiagonalisation — one read of the trailing lower triangle per column (sum_j m_j^2 / 2 * 8 B,
about N^3 / 6 * 8 B = 11.5 GB per graph at N = 2048) plus a read and a write of it per panel update
— with the fraction of HBM peak that count implies at the measured time.

    python tools/bench_full_eigh.py [--batches 256 4] [--reps 3] [--no-vendor] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lanczosnet_amd import ops  # noqa: E402
from lanczosnet_amd.utils.data_helper import _full_decomposition_library  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes / s
NB = 32             # the kernel's panel width (csrc/sym_eigh.hip)


def tridiag_bytes(n):
  symv = sum((n - 1 - j) ** 2 / 2.0 * 8 for j in range(n - 1))
  upd = sum((n - s) ** 2 / 2.0 * 8 * 2 for s in range(NB, n, NB))
  return symv, upd


def collated(B, N, p, seed):
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  L = torch.empty((B, N, N, 2), dtype=torch.float32, device='cuda')
  for b in range(B):
    adj = (torch.rand((N, N), generator=g, device='cuda') < p).float().triu(1)
    adj = adj + adj.t() + torch.eye(N, device='cuda')
    d = adj.sum(1).rsqrt()
    A = d[:, None] * adj * d[None, :]
    L[b, :, :, 0] = A
    L[b, :, :, 1] = A
  return L


def timed(fn, reps):
  fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t)
  return min(ts), ts


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batches', type=int, nargs='+', default=[256, 4])
  ap.add_argument('--nodes', type=int, default=2048)
  ap.add_argument('--k', type=int, default=64)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--no-vendor', action='store_true')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  N, K = args.nodes, args.k
  symv, upd = tridiag_bytes(N)
  out = dict(N=N, K=K, p_edge=0.01, device=torch.cuda.get_device_name(0),
             tridiag_bytes_per_graph=dict(symv=symv, panel_update=upd, total=symv + upd),
             hbm_peak_bytes_per_s=HBM_PEAK, runs=[])
  for B in args.batches:
    L = collated(B, N, 0.01, 7)
    n = torch.full((B,), N, dtype=torch.int32, device='cuda')
    A = L[:, :, :, 0]
    run = dict(B=B)
    t, ts = timed(lambda: ops.sym_eigh_topk(A, n, K), args.reps)
    byt = B * (symv + upd)
    run['sym_eigh_topk_s'] = t
    run['sym_eigh_topk_all_s'] = ts
    run['tridiag_bytes'] = byt
    run['hbm_fraction_at_total_time'] = byt / t / HBM_PEAK
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      t, _ = timed(lambda: ops.lanczos_ritz_collated(L, n, K), args.reps)
      run['kstep_collated_s'] = t
      if not args.no_vendor:
        t, _ = timed(lambda: _full_decomposition_library(A, n, K), 1)
        run['vendor_eigh_s'] = t
    out['runs'].append(run)
    print(json.dumps(run), flush=True)
    del L, A
    torch.cuda.empty_cache()
  line = json.dumps(out)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
