#!/usr/bin/env python
"""Random shapes through the wide K-step path (ops.lanczos_ritz_kstep -> lnz_lanczos_ritz_kstep_wide)
against the fp64 restatement (oracle.lanczos_kstep_fp64) on the CPU: widths in 2049..6000 that are
not multiples of 4 / 64 / 256, ragged and empty graphs, image capacities 8..256 (graphs beyond them
take the dense rows in the same call), M and K in 1..256.  Recorded, not a test: counts and worst
deviations go to --out.  A graph whose restatement stops early, or fails to, with its last norm
within 1e-7 of the 1e-8 threshold is a nearly invariant Krylov space: the two sides may
stop a step apart; such graphs are counted and listed, not compared.

usage: kstep_wide_fuzz.py [cases] [seed] [--seconds S] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import oracle  # noqa: E402
from lanczosnet_amd import ops  # noqa: E402


def graph(n, p, rs):
  a = np.triu((rs.rand(n, n) < p).astype(np.float64), 1)
  return oracle.laplacian_l4(a + a.T).astype(np.float32)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('cases', type=int, nargs='?', default=40)
  ap.add_argument('seed', type=int, nargs='?', default=1)
  ap.add_argument('--seconds', type=float, default=420.0, help='stop drawing new cases after this long')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kstep_wide_fuzz.json'))
  args = ap.parse_args()
  rs = np.random.RandomState(args.seed)
  st = dict(seed=args.seed, cases=0, graphs=0, empty=0, flagged=0, compared=0, nearly_invariant=[], failures=[],
            worst_D=0.0, worst_projector=0.0, worst_orthogonality=0.0, worst_residual_gap=0.0, early_stops=0)
  t0 = time.time()
  for case in range(args.cases):
    if time.time() - t0 > args.seconds:
      break
    N = int(rs.randint(2049, 6001))
    while N % 4 == 0:
      N = int(rs.randint(2049, 6001))
    B = int(rs.randint(1, 4))
    M = int(rs.randint(1, 257))
    K = int(rs.randint(1, M + 1))
    cap = int(rs.randint(1, 33)) * 8
    p = float(rs.choice([1.0, 3.0, 8.0, 20.0])) / N
    sizes = []
    A = np.zeros((B, N, N), np.float32)
    for b in range(B):
      kind = rs.randint(0, 6)
      n = N if kind < 2 else (0 if kind == 2 else int(rs.randint(1, N + 1)))
      if kind == 5:
        n = int(rs.randint(1, 40))         # fewer nodes than steps: the recurrence stops by itself
      sizes.append(n)
      if n:
        A[b, :n, :n] = graph(n, p * N / n if n > 64 else 0.3, rs)
    if M > N:
      M = N
      K = min(K, M)
    nn = torch.tensor(sizes, dtype=torch.int32, device='cuda')
    D, V, info, fb = ops.lanczos_ritz_kstep(torch.from_numpy(A).to('cuda'), nn, M, K, row_cap=cap, return_info=True,
                                            return_fallback=True)
    assert 'wide' in ops.last_kernel()
    D, V, info, fb = D.cpu().numpy(), V.cpu().numpy().astype(np.float64), info.cpu().numpy(), fb.cpu().numpy()
    st['cases'] += 1
    for b, n in enumerate(sizes):
      st['graphs'] += 1
      st['flagged'] += int(fb[b])
      tag = dict(case=case, graph=b, N=N, n=n, M=M, K=K, cap=cap)
      if n == 0:
        st['empty'] += 1
        if info[b] != 0 or D[b].any() or V[b].any():
          st['failures'].append(dict(tag, what='empty graph not zero'))
        continue
      Dr, Vr, (_, _, steps, last) = oracle.lanczos_kstep_fp64(A[b, :n, :n], M, K)
      if steps < min(M, n):
        st['early_stops'] += 1
      if abs(last - 1e-8) < 1e-7 and steps < n and int(info[b]) != steps:
        st['nearly_invariant'].append(dict(tag, restatement_steps=int(steps), device_steps=int(info[b]), last_norm=float(last)))
        continue
      kk = min(K, steps)
      Vg = V[b, :n]
      eD = float(np.abs(D[b] - Dr).max())
      eP = float(np.abs(Vg @ Vg.T - Vr @ Vr.T).max())
      eO = float(np.abs(Vg[:, :kk].T @ Vg[:, :kk] - np.eye(kk)).max())
      A64 = A[b, :n, :n].astype(np.float64)
      eR = float(np.abs(np.linalg.norm(A64 @ Vg - Vg * D[b], axis=0) - np.linalg.norm(A64 @ Vr - Vr * Dr, axis=0)).max())
      st['compared'] += 1
      st['worst_D'] = max(st['worst_D'], eD)
      st['worst_projector'] = max(st['worst_projector'], eP)
      st['worst_orthogonality'] = max(st['worst_orthogonality'], eO)
      st['worst_residual_gap'] = max(st['worst_residual_gap'], eR)
      ok = int(info[b]) == steps and eD < 1e-6 and eP < 1e-5 and eO < 1e-5 and eR < 1e-4 and \
          not V[b, n:].any() and not V[b, :, kk:].any() and not D[b, kk:].any()
      if not ok:
        st['failures'].append(dict(tag, D=eD, projector=eP, orthogonality=eO, residual_gap=eR, steps=int(steps),
                                   device_steps=int(info[b])))
    print('case %d: N %d sizes %s M %d K %d cap %d -> worst D %.1e P %.1e, failures %d' %
          (case, N, sizes, M, K, cap, st['worst_D'], st['worst_projector'], len(st['failures'])), flush=True)
  st['seconds'] = time.time() - t0
  line = json.dumps(st)
  print(line)
  with open(args.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
