"""Worker of tests/test_gpu_gains.py::test_one_tile_and_two_tile_kernels_give_the_same_bits: the
library reads LNZ_GAINS_TILES once per process, so the test starts this file as a fresh child per
setting (1 = spectral_gains_mlp_kernel, 2 = spectral_gains_mlp2_kernel) and compares the bytes each
child writes.  The test itself calls `compute()` too, for the launcher's own choice."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402  (parameter draw only)
from lanczosnet_amd import ops  # noqa: E402

DIST16 = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15, 20, 25, 30, 40, 50]
# (S, B, K, L): ragged row counts.  R = 999: R % 32 = 7, R % 64 = 39; R = 205: R % 64 = 13, the
# two-tile kernel's last wave has a wholly invalid second tile; R = 7911 x 16 layers is two-tile by
# the launcher's own rule (the first two are one-tile)
CASES = [(16, 37, 27, 2), (8, 37, 27, 2), (16, 41, 5, 3), (8, 41, 5, 3), (16, 293, 27, 16)]


def gains_cfg(S, L):
  return dict(num_atom=3, num_bond_type=1, short_diffusion_dist=[], long_diffusion_dist=DIST16[:S],
              num_eig_vec=4, spectral_filter_kind='MLP', input_dim=4, hidden_dim=[4] * L,
              output_dim=1, num_layer=L)


def mlp_layers(P, L, dev):
  """per conv layer the 4 (weight, bias) pairs of its filter MLP, as device tensors"""
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
  return [[(t(P['spectral_filter.%d.%d.weight' % (l, i)]), t(P['spectral_filter.%d.%d.bias' % (l, i)]))
           for i in (0, 2, 4, 6)] for l in range(L)]


def planted_eigenvalues(B, K, seed):
  """uniform in [-1, 1] with the values a power / MLP kernel gets wrong first planted in"""
  rs = np.random.RandomState(seed)
  D = rs.uniform(-1.0, 1.0, size=(B, K)).astype(np.float32)
  one = np.float32(1.0)
  lo, hi = np.nextafter(one, np.float32(0.0)), np.nextafter(one, np.float32(2.0))
  plant = np.array([0.0, -0.0, 1.0, -1.0, lo, hi, -lo, -hi, 1e-30], np.float32)
  D.reshape(-1)[rs.choice(B * K, size=len(plant), replace=False)] = plant
  return D


def compute(dev):
  """-> one float32 array: G of every case, flattened and concatenated"""
  out = []
  for i, (S, B, K, L) in enumerate(CASES):
    P = oracle.make_lanczosnet_params(gains_cfg(S, L), 300 + i)
    pack = ops.pack_spectral_mlp_layers(mlp_layers(P, L, dev), S)
    D = torch.from_numpy(planted_eigenvalues(B, K, 40 + i)).to(dev)
    out.append(ops.spectral_gains(D, DIST16[:S], L, pack).cpu().numpy().reshape(-1))
  return np.concatenate(out)


def main():
  assert os.environ.get('LNZ_GAINS_TILES') in ('1', '2')
  compute(torch.device('cuda', 0)).tofile(sys.argv[1])
  print('GAINS_TILES_OK tiles=%s' % os.environ['LNZ_GAINS_TILES'])


if __name__ == '__main__':
  main()
