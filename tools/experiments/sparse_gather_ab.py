#!/usr/bin/env python
"""A / B of two builds of the C-ABI library on the sparse-image kernels (csrc/conv_sparse.hip): the same
bits, the same time.  The library under test is the in-tree one, or the one LANCZOSNET_HIP_LIB names (a
variant from tools/experiments/build_variant.sh); tools/experiments/sparse_gather_ab.sh runs the steps,
each in a fresh process under its own time limit.

  bits  --out F.pt       the gather cases of tests/test_gpu_large_edges.py (B = 10, N = 133, row capacity 128
                         and 32): the images (one operator: expanded pair, one channel, strided slices; R = 2,
                         3, 8 channels), both one-operator gathers and both channel gathers, ReLU on and off
  same  A.pt B.pt        every saved tensor torch.equal, or exit 1
  time  --out F.json     per-launch time (device events, warm, the median of `--windows` windows of `--reps`
                         launches) and a SHA-256 of one launch's output: the one-operator gathers at config
                         5's shape (B 256, N 2048, G(n, 0.01)), the channel gathers at the two-type shape of
                         tools/bench_typed_edges.py (R = 3), the channel / strided image kernels at B = 32
  report --parent P1 P2 P3 --new N1 N2 N3 --out F.json
                         medians, the parent's own max - min spread as the margin, equal hashes; exit 1 when a
                         new median exceeds the parent's by more than the margin or a hash differs
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

DEV = 'cuda:0'
SHAPE = dict(B=256, N=2048, p=0.01, E=2, image_B=32)
GATHERS = ('sparse_conv_kernel', 'sparse_conv_f32_kernel', 'sparse_conv_channels_kernel',
           'sparse_conv_channels_f32_kernel')


def gather(ops, img, Z, X, relu, f32):
  """one launch of the entry that serves (img, f32), X accumulated in place"""
  abi = ops._abi()
  B, N = img.B, img.N
  if hasattr(img, 'R'):
    if f32:
      abi.large_sparse_conv_channels_f32(img.entries, img.values, img.counts, img.cap, Z, B, N, img.R, relu, X)
    else:
      abi.large_sparse_conv_channels(img.entries, img.counts, img.cap, Z, B, N, img.R, relu, X)
  elif f32:
    abi.large_sparse_conv_f32(img.entries, img.values, img.counts, img.cap, Z, B, N, relu, X)
  else:
    abi.large_sparse_conv(img.entries, img.counts, img.cap, Z, B, N, relu, X)
  return X


def live(img):
  """(entries, values) with everything behind a row's padded count cleared (never written: any bits)"""
  import torch
  keep = torch.arange(img.cap, device=img.counts.device) < ((img.counts + 7) // 8 * 8).unsqueeze(-1)
  return (torch.where(keep, img.entries, 0).cpu(), torch.where(keep, img.values, 0.0).cpu(), img.counts.cpu(),
          img.flags.cpu())


def bits(out):
  import torch
  import large_edges_fixture as fx
  from lanczosnet_amd import ops
  dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
  saved = {}
  for cap in (128, 32):
    case = fx.gather_case(cap, False)
    L = dev(case['L'])
    B, N = L.shape[:2]
    one = ops.large_sparse_image(L.unsqueeze(3), cap, values=True)
    saved['image/cap%d/rows' % cap] = live(one)
    saved['image/cap%d/pair' % cap] = live(ops.large_sparse_image(L.unsqueeze(3).expand(B, N, N, 2).contiguous(), cap,
                                                                  values=True))
    saved['image/cap%d/expanded' % cap] = live(ops.large_sparse_image(L.unsqueeze(3).expand(B, N, N, 2), cap, values=True))
    Zf = dev(case['Z'])
    for f32 in (False, True):
      for relu in (0, 1):
        saved['gather/cap%d/f32=%d/relu=%d' % (cap, f32, relu)] = gather(
            ops, one, Zf if f32 else Zf.to(torch.bfloat16), dev(case['X0']).clone(), relu, f32).cpu()
        assert ops.last_kernel() == GATHERS[int(f32)]
    for R in (2, 3, 8):
      ch = fx.gather_channels_case(cap, R)
      Lc = dev(ch['L'])
      imgs = ops.large_sparse_image_channels(Lc, cap, values=True)
      saved['images/cap%d/R%d' % (cap, R)] = live(imgs)
      saved['image/cap%d/R%d/strided' % (cap, R)] = live(ops.large_sparse_image(Lc[..., R - 1:R], cap, values=True))
      Zf = dev(ch['Z'])
      for f32 in (False, True):
        for relu in (0, 1):
          saved['gather/cap%d/R%d/f32=%d/relu=%d' % (cap, R, f32, relu)] = gather(
              ops, imgs, Zf if f32 else Zf.to(torch.bfloat16), dev(ch['X0']).clone(), relu, f32).cpu()
          assert ops.last_kernel() == GATHERS[2 + int(f32)]
  torch.cuda.synchronize()
  torch.save(saved, out)
  print('bits: %d results -> %s (%s)' % (len(saved), out, os.environ.get('LANCZOSNET_HIP_LIB', 'the in-tree library')))


def same(a, b):
  import torch
  A, Bd = torch.load(a), torch.load(b)
  assert sorted(A) == sorted(Bd)
  bad = []
  for k in sorted(A):
    xs, ys = (A[k], Bd[k]) if isinstance(A[k], tuple) else ((A[k],), (Bd[k],))
    # (bit patterns: a NaN equals itself)
    if not all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
               for x, y in zip(xs, ys)):
      bad.append(k)
  print('same: %d results compared, %d differ %s' % (len(A), len(bad), bad))
  return 1 if bad else 0


def timed(fn, windows, reps):
  import torch
  ms = []
  for w in range(windows + 1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
      fn()
    e1.record()
    torch.cuda.synchronize()
    if w:   # (window 0 warms the code object and the caches)
      ms.append(e0.elapsed_time(e1) / reps)
  ms.sort()
  return dict(min=ms[0], median=ms[len(ms) // 2], max=ms[-1])


def sha(t):
  return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def time_kernels(out, windows, reps):
  import torch
  from lanczosnet_amd import ops
  from tools.bench_edge_collate import gnp_edges
  s = SHAPE
  B, N, E, R = s['B'], s['N'], s['E'], s['E'] + 1
  rs = np.random.RandomState(5)
  graphs = [gnp_edges(N, s['p'], rs) for _ in range(B)]
  types = [rs.randint(0, E, size=g.shape[0]).astype(np.int32) for g in graphs]
  off = np.concatenate([[0], np.cumsum([g.shape[0] for g in graphs])]).astype(np.int64)
  edges, ety = torch.from_numpy(np.concatenate(graphs)).to(DEV), torch.from_numpy(np.concatenate(types)).to(DEV)
  n_nodes = torch.full((B,), N, dtype=torch.int32, device=DEV)
  img = ops.sparse_laplacian_from_edges(edges, torch.from_numpy(off).to(DEV), n_nodes, N).image
  typed = ops.sparse_laplacian_from_edges(edges, torch.from_numpy(off).to(DEV), n_nodes, N, edge_type=ety, num_edge_type=E)
  imgs = typed.images
  assert int(img.flags.item()) == 0 and int(imgs.flags.item()) == 0 and imgs.R == R
  g = torch.Generator(device=DEV).manual_seed(1)
  Zf = torch.randn((R, B, N, 128), device=DEV, generator=g)
  Zb = Zf.to(torch.bfloat16)
  X0 = torch.randn((B, N, 128), device=DEV, generator=g)
  rec = dict(library=os.environ.get('LANCZOSNET_HIP_LIB', 'in-tree'), windows=windows, reps=reps, shape=s,
             entries_per_row=[float(img.counts.float().mean())] + [float(imgs.counts[c].float().mean()) for c in range(R)],
             kernels={})
  for name, im, Z, f32 in ((GATHERS[0], img, Zb[0], False), (GATHERS[1], img, Zf[0], True),
                           (GATHERS[2], imgs, Zb, False), (GATHERS[3], imgs, Zf, True)):
    digest = sha(gather(ops, im, Z, X0.clone(), 1, f32))
    assert ops.last_kernel() == name
    X = X0.clone()
    rec['kernels'][name] = dict(timed(lambda: gather(ops, im, Z, X, 1, f32), windows, reps), sha256=digest)
    print(name, rec['kernels'][name], flush=True)
  # the image kernels that share the strided row scan (their register allocation moved with it)
  del Zf, Zb, X, X0
  Bi = s['image_B']
  few = ops.sparse_laplacian_from_edges(edges[:int(off[Bi])], torch.from_numpy(off[:Bi + 1]).to(DEV), n_nodes[:Bi], N,
                                        edge_type=ety[:int(off[Bi])], num_edge_type=E)
  L = few.to_dense()
  for name, fn in (('sparse_image_channels_kernel', lambda: ops.large_sparse_image_channels(L)),
                   ('sparse_image_kernel<strided>', lambda: ops.large_sparse_image(L[..., 1:2], values=True))):
    got = live(fn())
    assert ops.last_kernel() == name
    rec['kernels'][name] = dict(timed(fn, windows, max(1, reps // 10)), B=Bi,
                                sha256=hashlib.sha256(b''.join(t.numpy().tobytes() for t in got)).hexdigest())
    print(name, rec['kernels'][name], flush=True)
  with open(out, 'w') as f:
    json.dump(rec, f, indent=1, sort_keys=True)


def report(parent, new, out, registers):
  P, Nw = [json.load(open(f)) for f in parent], [json.load(open(f)) for f in new]
  med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
  result = dict(shape=P[0]['shape'], windows=P[0]['windows'], reps=P[0]['reps'], entries_per_row=P[0]['entries_per_row'],
                unit='ms per launch: each run is the median of its windows', kernels={}, ok=True)
  for k in P[0]['kernels']:
    p, n = [r['kernels'][k]['median'] for r in P], [r['kernels'][k]['median'] for r in Nw]
    margin = max(p) - min(p)
    row = dict(parent_runs=p, new_runs=n, parent_median=med(p), new_median=med(n), margin=margin,
               same_bits=len({r['kernels'][k]['sha256'] for r in P + Nw}) == 1)
    row['within_margin'] = row['new_median'] <= row['parent_median'] + margin
    result['kernels'][k] = row
    result['ok'] = result['ok'] and row['same_bits'] and (row['within_margin'] or k not in GATHERS)
    print('%-34s parent %.4f new %.4f margin %.4f %s %s' % (k, row['parent_median'], row['new_median'], margin,
                                                          'ok' if row['within_margin'] else 'SLOWER',
                                                          'same bits' if row['same_bits'] else 'OTHER BITS'))
  if registers:
    result['registers'] = json.load(open(registers))
  with open(out, 'w') as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write('\n')
  print('wrote', out)
  return 0 if result['ok'] else 1


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('step', choices=['bits', 'same', 'time', 'report'])
  ap.add_argument('files', nargs='*')
  ap.add_argument('--out')
  ap.add_argument('--windows', type=int, default=7)
  ap.add_argument('--reps', type=int, default=200)
  ap.add_argument('--parent', nargs='+')
  ap.add_argument('--new', nargs='+')
  ap.add_argument('--registers', help='a JSON file with the register table (tools/kernel_resources.py), copied in')
  a = ap.parse_args()
  if a.step in ('bits', 'time'):
    import torch
    if not torch.cuda.is_available():
      raise SystemExit('sparse_gather_ab: needs the MI355X (no CPU fallback)')
  if a.step == 'bits':
    bits(a.out)
  elif a.step == 'same':
    sys.exit(same(*a.files))
  elif a.step == 'time':
    time_kernels(a.out, a.windows, a.reps)
  else:
    sys.exit(report(a.parent, a.new, a.out, a.registers))


if __name__ == '__main__':
  main()
