"""lnz_collate_qm8 (csrc/collate.hip) through ops.collate_qm8 on hand-built shards, at the shapes on both
sides of its LDS bound and on the molecules a shard can hold: no bonds, a bond listed twice, a self bond, a
bond of a type >= E or touching an atom >= n (dropped), more than 256 bonds, a molecule larger than the tile
(cut), ids outside [0, n_mol) and a repeated id, P = 1 and P = 300 labels.

L against oracle.dense_from_edges + oracle.laplacian_multi_l4 in float64 under the bar of builder_cases.py,
and bit for bit against ops.laplacian_l4 on the dense adjacency of the same molecules — a comparison worth
something since test_gpu_laplacian_edges.py holds that kernel itself; node_feat, node_mask, label and n_nodes
exactly.  test_builder_cases_cpu.py shows the shapes on the bound and the molecules holding their cases."""
import numpy as np
import pytest
import torch

import builder_cases as bc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(x):
  return torch.from_numpy(np.array(x)).to(DEV)   # (a copy: the shared cases are read-only)


def _shard(mols):
  mol_off, edge_off, atoms, edges, labels = bc.shard_arrays(mols)
  return dict(mol_off=_t(mol_off), edge_off=_t(edge_off), atoms=_t(atoms), edges=_t(edges), labels=_t(labels))


def _collate(mols, ids, N, E, P):
  from lanczosnet_amd import ops
  out = ops.collate_qm8(_shard(mols), _t(ids), N, E, P)
  assert ops.last_kernel() == 'collate_qm8_kernel', ops.last_kernel()
  return out


@pytest.mark.parametrize('N,E,P', bc.COLLATE_SHAPES)
def test_collate_of_a_hand_built_shard(N, E, P):
  from lanczosnet_amd import ops
  mols = bc.collate_molecules(N, E, P)
  ids = bc.collate_ids(len(mols))
  feat, mask, label, n_nodes, adjs = bc.collate_expected(mols, ids, N, E)
  out = _collate(mols, ids, N, E, P)
  assert out['L'].shape == (len(ids), N, N, E + 1) and out['label'].shape == (len(ids), P)
  assert np.array_equal(out['n_nodes'].cpu().numpy(), n_nodes)
  assert np.array_equal(out['node_feat'].cpu().numpy(), feat)
  assert np.array_equal(out['node_mask'].cpu().numpy(), mask)
  assert np.array_equal(out['label'].cpu().numpy().view(np.int32), label.view(np.int32))
  L = out['L'].cpu().numpy()
  worst, differ = bc.check_bar(L, bc.collate_reference(adjs, n_nodes), n_nodes, (N, E))
  print('collate_qm8_kernel N=%d E=%d P=%d: worst achieved/bar %.3f, %d elements differ from float32(ref)'
        % (N, E, P, worst, differ))
  assert torch.equal(out['L'], ops.laplacian_l4(_t(adjs), _t(n_nodes)))
  names = [m.name for m in mols]
  eye = np.zeros((N, N, E + 1), np.float32)
  k = names.index('no_bonds')
  eye[np.arange(n_nodes[k]), np.arange(n_nodes[k])] = 1
  assert np.array_equal(L[k], eye)                       # no bonds: the identity on n in every channel
  # a molecule larger than the tile equals the collate of the molecule cut to the tile
  cut = tuple(bc.truncated(m, N) for m in mols)
  again = _collate(cut, ids, N, E, P)
  for key in ('L', 'node_feat', 'node_mask', 'label', 'n_nodes'):
    assert torch.equal(again[key], out[key]), key
  # a molecule's result does not depend on its place in the batch (B = 1: the cut molecule, an unknown id)
  for b in (names.index('oversized'), len(mols) + 1):
    one = _collate(mols, ids[b:b + 1], N, E, P)
    assert torch.equal(one['L'][0], out['L'][b]) and torch.equal(one['label'][0], out['label'][b])


@pytest.mark.parametrize('N,E', bc.COLLATE_REFUSED)
def test_collate_refuses_the_first_shapes_beyond_its_lds_bound(N, E):
  from lanczosnet_amd import ops, _lib
  mols = bc.collate_molecules(2, 1, 1)
  with pytest.raises(_lib.NotSupported):
    ops.collate_qm8(_shard(mols), _t(np.zeros(1, np.int64)), N, E, 1)
