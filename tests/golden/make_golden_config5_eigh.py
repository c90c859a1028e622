#!/usr/bin/env python
"""BASELINE config 5 at its FULL size pinned on the reference's OWN Ritz pairs: the same inputs as
config5_full.npz (tests/large_fixture.general_inputs, seed 11, B = 2, N = 2048, K = 64), but (D, V)
taken from the unmodified `utils/data_helper.py` get_graph_laplacian_eigs(adj_b, k=64,
graph_laplacian_type='L4', use_eigen_decomp=True) — `np.linalg.eigh` of the float64 L4 and the
top-64 |lambda| cut — and the unmodified LanczosNetGeneral scores on them.

Stored (basis-invariant where V is involved):
  score           the reference scores [B, 2]
  D               [B, K] eigenvalues in the reference order
  V_abs_colsum    sum_r |V[r, k]| per column [B, K]
  probe           V V^T R for the seeded probe R [N, 4] (numpy seed 5), float32 [B, N, 4]
  cut_gap         |lambda_64| - |lambda_65| per graph
  fp32_floor_D / fp32_floor_probe   how far (D, probe) move when the reference is fed its own
                  Laplacian rounded to fp32 (what the device sees): the floor a device result can
                  reach, reported by the GPU test next to its own error.

    python tests/golden/make_golden_config5_eigh.py       # needs the reference tree, ~1 min
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import AttrDict, import_reference, params_checksum  # noqa: E402
from large_fixture import adjacency, general_inputs  # noqa: E402

B, N, K, LAYERS, SEED, P_EDGE, PROBE_SEED = 2, 2048, 64, 7, 11, 0.01, 5


def probe_matrix():
  return np.random.RandomState(PROBE_SEED).randn(N, 4)


def ref_pairs(ref_dh, adj):
  D = np.zeros((B, K), np.float64)
  V = np.zeros((B, N, K), np.float64)
  gap = np.zeros((B,), np.float64)
  for b in range(B):
    eigs, v, _ = ref_dh.get_graph_laplacian_eigs(adj[b], k=K, graph_laplacian_type='L4',
                                                 use_eigen_decomp=True)
    D[b], V[b] = eigs, v
    # the cut gap needs the 65th modulus: one more pair from the same call
    e65, _, _ = ref_dh.get_graph_laplacian_eigs(adj[b], k=K + 1, graph_laplacian_type='L4',
                                                use_eigen_decomp=True)
    gap[b] = abs(e65[K - 1]) - abs(e65[K])
  return D, V, gap


def main():
  ref_model, ref_dh, _ = import_reference()
  torch.set_num_threads(os.cpu_count() or 4)
  cfg, P, X, L, mask = general_inputs(B, N, K, LAYERS, SEED, P_EDGE)
  adj = adjacency(B, N, P_EDGE, SEED)
  D, V, gap = ref_pairs(ref_dh, adj)
  # the same function fed its own Laplacian rounded to fp32 (the device's input precision)
  orig = ref_dh.get_laplacian
  ref_dh.get_laplacian = lambda *a, **k: orig(*a, **k).astype(np.float32).astype(np.float64)
  try:
    D32, V32, _ = ref_pairs(ref_dh, adj)
  finally:
    ref_dh.get_laplacian = orig
  R = probe_matrix()
  probe = np.einsum('bnk,bmk,mj->bnj', V, V, R)
  probe32 = np.einsum('bnk,bmk,mj->bnj', V32, V32, R)
  floor_probe = np.abs(probe32 - probe).max(axis=(1, 2)) / np.abs(probe).max(axis=(1, 2))
  floor_D = np.abs(D32 - D).max(axis=1)
  model = dict(name='LanczosNetGeneral', short_diffusion_dist=[],
               long_diffusion_dist=cfg['long_diffusion_dist'], num_eig_vec=K,
               spectral_filter_kind='MLP', input_dim=10, hidden_dim=[128] * LAYERS, output_dim=2,
               num_layer=LAYERS, loss='MSE')
  config = AttrDict(dict(seed=1234, model=model,
                         dataset=dict(node_emb_dim=10, graph_emb_dim=2, num_edge_type=1)))
  net = ref_model.LanczosNetGeneral(config).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  with torch.no_grad():
    score = net(torch.from_numpy(X), torch.from_numpy(L), torch.from_numpy(D.astype(np.float32)),
                torch.from_numpy(V.astype(np.float32)), mask=torch.from_numpy(mask).bool())
  path = os.path.join(HERE, 'config5_eigh.npz')
  np.savez_compressed(path, B=B, N=N, K=K, num_layer=LAYERS, seed=SEED, p_edge=P_EDGE,
                      probe_seed=PROBE_SEED, score=score.numpy(), D=D,
                      V_abs_colsum=np.abs(V).sum(axis=1), probe=probe.astype(np.float32),
                      cut_gap=gap, fp32_floor_D=floor_D, fp32_floor_probe=floor_probe,
                      param_checksum=params_checksum(P))
  print('score', score.numpy())
  print('cut gaps', gap, 'fp32 floor: D', floor_D, 'probe', floor_probe)
  print('wrote', path, os.path.getsize(path), 'B')


if __name__ == '__main__':
  main()
