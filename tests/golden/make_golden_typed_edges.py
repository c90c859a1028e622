#!/usr/bin/env python
"""Golden fixture for several edge types on the large-graph sparse path, produced by running the
UNMODIFIED reference on CPU in the build container:

    utils/data_helper.py          get_laplacian('L4') per operator channel (the simple graph, then every
                                  edge type alone: dataset/get_graph_data.py:60-72) and
                                  get_graph_laplacian_eigs(k = 20) of the simple graph (eigsh + |lambda| sort)
    model/lanczos_net_general.py  LanczosNetGeneral(config).eval()(...)   (two layers, width 128)

on two typed graphs padded to 301 nodes, E = 2 (tests/typed_edge_graphs.py: case('n301', 2), graphs 0 and
1, with their engineered rows).  Stored, DATA only: the edges and their types, node features, mask, the
collated L (compressed: 99 % zeros), D, V, the parameter seed (oracle.make_lanczosnet_params, loaded into
the reference with load_state_dict) and checksum, the configuration values and the reference scores.

    python tests/golden/make_golden_typed_edges.py    # needs the reference tree; writes typed_edges.npz
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

from make_golden import import_reference, make_config, params_checksum  # noqa: E402

E, K, PARAM_SEED = 2, 20, 2024
CFG = dict(num_bond_type=E, short_diffusion_dist=[], long_diffusion_dist=[1, 2, 3], num_eig_vec=K,
           spectral_filter_kind='MLP', input_dim=10, hidden_dim=[128, 128], output_dim=2, num_layer=2, num_atom=0)


def main():
  import typed_edge_graphs as tg
  from oracle import make_lanczosnet_params
  ref_model, ref_dh, _ = import_reference()
  torch.set_num_threads(4)
  graphs, N = tg.case('n301', E)
  graphs = graphs[:2]
  B = len(graphs)
  rs = np.random.RandomState(77)
  L = np.zeros((B, N, N, E + 1), np.float32)
  D = np.zeros((B, K), np.float32)
  V = np.zeros((B, N, K), np.float32)
  X = np.zeros((B, N, CFG['input_dim']), np.float32)
  mask = np.zeros((B, N), np.uint8)
  for b, g in enumerate(graphs):
    n = g['n']
    adjs = tg.dense_adjs([g], n, E)[0].astype(np.float64)                    # [n,n,E]
    d, v, l4 = ref_dh.get_graph_laplacian_eigs(adjs.sum(axis=2), k=K, graph_laplacian_type='L4',
                                               use_eigen_decomp=False, is_sym=True)
    assert d is not None
    L[b, :n, :n, 0] = l4
    for e in range(E):
      L[b, :n, :n, 1 + e] = ref_dh.get_laplacian(adjs[:, :, e], graph_laplacian_type='L4')
    D[b], V[b, :n] = d, v
    X[b, :n] = rs.randn(n, CFG['input_dim'])
    mask[b, :n] = 1
  P = make_lanczosnet_params(CFG, seed=PARAM_SEED, general=True)
  net = ref_model.LanczosNetGeneral(make_config(CFG, name='LanczosNetGeneral', general=True)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  with torch.no_grad():
    score = net(torch.from_numpy(X), torch.from_numpy(L), torch.from_numpy(D), torch.from_numpy(V),
                mask=torch.from_numpy(mask).bool())
  edges, off, n_nodes, types = tg.pack(graphs)
  out = dict(edges=edges, edge_off=off, n_nodes=n_nodes, edge_type=types, node_feat=X, node_mask=mask, L=L, D=D, V=V,
             score=score.numpy(), param_seed=PARAM_SEED, param_checksum=params_checksum(P), num_edge_type=E, N=N, K=K,
             num_layer=CFG['num_layer'], long_diffusion_dist=np.array(CFG['long_diffusion_dist'], np.int64),
             hidden_dim=np.array(CFG['hidden_dim'], np.int64))
  path = os.path.join(HERE, 'typed_edges.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, os.path.getsize(path), 'B; score', score.numpy().ravel())


if __name__ == '__main__':
  main()
