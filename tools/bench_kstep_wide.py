#!/usr/bin/env python
"""The wide K-step Lanczos path (ops.lanczos_ritz_kstep -> lnz_lanczos_ritz_kstep_wide: graphs beyond
2048 nodes or 64 Lanczos steps) on seeded G(N, p) graphs (the adjacency generator of
tests/large_fixture.py, L4 on the device): wall time per call from device events, warm, in several
windows (min / median / max), beside
  * the existing one-workgroup entry at (B 256, N 2048, M = K = 64), and the new path forced onto
    the same shape (a direct call of the C entry);
  * the vendor eigensolver the project uses as its yardstick (torch.linalg.eigh, fp64, on the
    device) where --vendor-max-n allows.
No time here is asserted anywhere.

The byte counts of a step are computed from the shapes: the image, 6 B per stored entry (slab padding
included: 64 rows x the slab's longest row rounded up to 8) plus an 8 B gather of q per entry; the
basis, (j + 1) N 8 B per kernel and pass (dots, update), i.e. M (M + 1) / 2 N 8 B x 2 per call
for one pass.  With --kernel-stats (the CSV of a separate `rocprofv3 --kernel-trace --stats` run of
this script with --shapes restricted to one shape) the per-kernel totals are set against them.

    python tools/bench_kstep_wide.py [--windows 5] [--reps 3] [--out profiles/kstep_wide_bench.json]
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lanczosnet_amd import _lib, ops  # noqa: E402

HBM_PEAK = 8.0e12   # MI355X HBM3E, bytes / s
SHAPES = [(4, 4096, 64, 64, 8.0 / 4096), (4, 8192, 128, 64, 8.0 / 8192), (2, 16384, 256, 64, 8.0 / 16384),
          (256, 2048, 128, 64, 0.01)]


def graphs(B, N, p, seed):
  """tests/large_fixture.adjacency's draws (numpy RandomState(seed), upper triangle mirrored), L4 =
  D^-1/2 (I + A) D^-1/2 in fp64 on the device, stored fp32."""
  rs = np.random.RandomState(seed)
  A = torch.empty((B, N, N), dtype=torch.float32, device='cuda')
  for b in range(B):
    a = torch.from_numpy(np.triu(rs.rand(N, N) < p, 1)).to('cuda').double()
    a = a + a.t() + torch.eye(N, dtype=torch.float64, device='cuda')
    d = a.sum(1).rsqrt()
    A[b] = (d[:, None] * a * d[None, :]).float()
  return A


def image_bytes(A):
  """(stored entries with slab padding, real nonzeros) of the sliced-ELL image of the batch."""
  B, N, _ = A.shape
  cnt = (A != 0).sum(dim=2)                                   # [B, N]
  pad = (-N) % 64
  if pad:
    cnt = torch.nn.functional.pad(cnt, (0, pad))
  width = (cnt.view(B, -1, 64).max(dim=2).values + 7) // 8 * 8
  return int(width.sum()) * 64, int(cnt.sum())


def windows(fn, n_windows, reps):
  fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(n_windows):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
      fn()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1) / reps * 1e-3)
  return dict(min_s=min(ts), median_s=float(np.median(ts)), max_s=max(ts), windows=n_windows, calls_per_window=reps)


def direct_wide(A, M, K):
  """lnz_lanczos_ritz_kstep_wide itself, whatever the routing of ops would choose."""
  lib = _lib.load()
  B, N, _ = A.shape
  cap = ops.kstep_row_cap(N)
  need = lib.lnz_lanczos_ritz_kstep_wide_workspace_bytes(B, N, M, cap)
  ws = torch.empty((need,), dtype=torch.uint8, device='cuda')
  D = torch.empty((B, K), dtype=torch.float32, device='cuda')
  V = torch.empty((B, N, K), dtype=torch.float32, device='cuda')
  p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

  def run():
    _lib.check(lib.lnz_lanczos_ritz_kstep_wide(p(A), A.stride(0), A.stride(1), 1, None, B, N, M, K, cap, p(ws), need,
                                               p(D), p(V), None, None,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
  return run


def kernel_stats(path):
  out = {}
  with open(path) as f:
    for row in csv.DictReader(f):
      name = row.get('Name') or row.get('KernelName') or ''
      for key in ('wide_spmv_kernel', 'wide_dots_kernel', 'wide_update_kernel', 'wide_vectors_kernel',
                  'wide_invit_kernel', 'wide_bisect_kernel', 'wide_init_kernel', 'ell_compact_rows_kernel',
                  'ell_pad_kernel'):
        if key in name:
          out[key] = dict(calls=int(row['Calls']), total_ns=float(row['TotalDurationNs']))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--windows', type=int, default=5)
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--shapes', type=int, nargs='+', default=list(range(len(SHAPES))), help='indices into SHAPES')
  ap.add_argument('--vendor-max-n', type=int, default=4096, help='torch.linalg.eigh (fp64) up to this N; 0: never')
  ap.add_argument('--no-seam', action='store_true')
  ap.add_argument('--kernel-stats', default=None)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  out = dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, runs=[])
  for i in args.shapes:
    B, N, M, K, p = SHAPES[i]
    A = graphs(B, N, p, seed=N)
    stored, nnz = image_bytes(A)
    run = dict(B=B, N=N, M=M, K=K, p_edge=p, launches=5 * M + 8, nnz=nnz, image_entries_with_padding=stored,
               spmv_bytes_per_step=stored * 6 + stored * 8 + B * N * 24,
               basis_bytes_one_pass=M * (M + 1) // 2 * N * 8 * 2 * B)
    run['wide'] = windows(lambda: ops.lanczos_ritz_kstep(A, None, M, K), args.windows, args.reps)
    run['kernel'] = ops.last_kernel()
    if N <= args.vendor_max_n and B <= 8:
      A64 = A.double()
      run['vendor_eigh_fp64'] = windows(lambda: torch.linalg.eigh(A64), 1, 1)
      del A64
    if args.kernel_stats:
      st = kernel_stats(args.kernel_stats)
      run['kernel_stats'] = st
      n_calls = st.get('wide_spmv_kernel', {}).get('calls', 0) // M
      if n_calls:
        t_spmv = st['wide_spmv_kernel']['total_ns'] * 1e-9 / n_calls
        t_gs = (st['wide_dots_kernel']['total_ns'] + st['wide_update_kernel']['total_ns']) * 1e-9 / n_calls
        run['spmv_hbm_fraction'] = run['spmv_bytes_per_step'] * M / t_spmv / HBM_PEAK
        run['gram_schmidt_hbm_fraction'] = run['basis_bytes_one_pass'] / t_gs / HBM_PEAK
        run['bound'] = 'launch latency and L2 (a step of a few graphs moves far less than HBM can in a launch)'
    out['runs'].append(run)
    print(json.dumps(run), flush=True)
    del A
    torch.cuda.empty_cache()
  if not args.no_seam:
    B, N, M = 256, 2048, 64
    A = graphs(B, N, 0.01, seed=N)
    seam = dict(B=B, N=N, M=M, K=M)
    seam['existing_entry'] = windows(lambda: ops.lanczos_ritz_kstep(A, None, M, M), args.windows, args.reps)
    seam['existing_kernel'] = ops.last_kernel()
    seam['wide_entry_direct'] = windows(direct_wide(A, M, M), args.windows, args.reps)
    out['seam'] = seam
    print(json.dumps(seam), flush=True)
  line = json.dumps(out)
  print(line)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
