"""Worker of tests/test_gpu_gains_compact.py: the library reads LNZ_GAINS_COMPACT once per process,
so the test starts this file as a fresh child per form (0 = the padded first and last Linear, unset
= the compact ones) and compares what the children write.  One float32 file: G of every case of
`cases()`, first without and then with the live-row list, flattened and concatenated."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402  (parameter draw only)
from gains_tiles_worker import DIST16, gains_cfg, mlp_layers, planted_eigenvalues  # noqa: E402
from lanczosnet_amd import ops  # noqa: E402

# (B, K, L): the first two reach the one-tile kernel by the launcher's own rule, the other two the
# two-tile kernel with a ragged second tile (tests/test_gpu_gains.py: SHAPES)
SHAPES = [(3, 5, 1), (37, 27, 2), (205, 20, 16), (293, 27, 16)]
# odd S: a half-empty last k-step of the first Linear; S % 4 != 0: a part-filled feature group of
# the last; 8 | 9: the switch of the first Linear's form; 16: four groups
SCALES = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16]


# the pack layout of csrc/gains_body.hpp, restated: the padded form's pack ends at OFF_W0C
# (W0 image, four bias images of 128 rows and one of 32, W2 | W4 | W6 streams, 8 slots of slack)
OFF_W0C = 4 * 8 * 64 + 3 * 4 * 1024 + 1024 + 2 * 4 * 16 * 256 + 16 * 256 + 8 * 256
OFF_W6C = OFF_W0C + 4 * 4 * 64
PACK_SIZE = OFF_W6C + 4 * 8 * 64


def rev3(j):
  return ((j & 1) << 2) | (j & 2) | (j >> 2)


def compact_images(W0, W6, S):
  """numpy restatement of the two images behind the slack, W0 [128,S], W6 [S,128] -> float32
  [PACK_SIZE - OFF_W0C]:
    W0c[ot][u][lane]       = W0[32 ot + (lane & 31)][2 u + (lane >> 5)]
    W6c[grp][v][4 blk + i] = W6[4 grp + i][8 (2 v + (blk >> 3)) + rev3(blk & 7)]
  zero where the feature (W0c) or the row (W6c) is >= S."""
  W0c = np.zeros((4, 4, 64), np.float32)
  for ot in range(4):
    for u in range(4):
      for lane in range(64):
        f = 2 * u + (lane >> 5)
        if f < S:
          W0c[ot, u, lane] = W0[32 * ot + (lane & 31), f]
  W6c = np.zeros((4, 8, 64), np.float32)
  for grp in range(4):
    for v in range(8):
      for blk in range(16):
        for i in range(4):
          if 4 * grp + i < S:
            W6c[grp, v, 4 * blk + i] = W6[4 * grp + i, 8 * (2 * v + (blk >> 3)) + rev3(blk & 7)]
  return np.concatenate([W0c.reshape(-1), W6c.reshape(-1)])


def cases():
  return [(S, B, K, L) for (B, K, L) in SHAPES for S in SCALES]


def case_inputs(S, B, K, L):
  """-> (P, D [B,K] float32, n [B] int32): the parameters, eigenvalues and node counts of a case"""
  P = oracle.make_lanczosnet_params(gains_cfg(S, L), 2000 + 31 * S + B)
  D = planted_eigenvalues(B, K, 11 * S + B)
  rs = np.random.RandomState(S + B)
  n = rs.randint(1, 33, size=B).astype(np.int32)
  n[:3] = [1, K, 32]
  return P, D, n


def compute(dev):
  out = []
  for (S, B, K, L) in cases():
    P, D, n = case_inputs(S, B, K, L)
    pack = ops.pack_spectral_mlp_layers(mlp_layers(P, L, dev), S)
    Dd = torch.from_numpy(D).to(dev)
    mask = torch.from_numpy((np.arange(32)[None, :] < n[:, None]).astype(np.uint8)).to(dev)
    _, rows = ops.plan_batch(mask, True, K)
    out.append(ops.spectral_gains(Dd, DIST16[:S], L, pack).cpu().numpy().reshape(-1))
    out.append(ops.spectral_gains(Dd, DIST16[:S], L, pack, rows=rows, zero_fill=True).cpu().numpy().reshape(-1))
  return np.concatenate(out)


def main():
  form = os.environ.get('LNZ_GAINS_COMPACT')
  assert form in (None, '0')
  compute(torch.device('cuda', 0)).tofile(sys.argv[1])
  print('GAINS_COMPACT_OK form=%s' % form)


if __name__ == '__main__':
  main()
