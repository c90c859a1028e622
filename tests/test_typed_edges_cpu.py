"""Host-side checks of the typed edge-list route: the graphs of tests/typed_edge_graphs.py stay inside
both row capacities in every operator channel (so none of the GPU cases passes through a densifying
fallback), the engineered rows are what the GPU tests count on, collate_graph_edges refuses malformed
edge types before anything is uploaded, and the reference fixture's Laplacian channels are the fp64
formula's."""
import os

import numpy as np
import pytest

import edge_graphs as eg
import typed_edge_graphs as tg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'typed_edges.npz')
CASES = [('n301', 2), ('n301', 3), ('n256', 2), ('n256', 3), ('n256', 7), ('n2100', 2)]


@pytest.mark.parametrize('name,E', CASES)
def test_typed_cases_stay_inside_both_capacities_and_the_dense_yardstick(name, E):
  from lanczosnet_amd import ops
  graphs, N = tg.case(name, E)
  Np = (N + 3) // 4 * 4
  assert eg.conv_cap(N) == ops.large_sparse_row_cap(N)
  assert (E + 1) * N <= ops.LAPLACIAN_MAX_CHANNEL_NODES                      # lnz_laplacian_l4 serves the yardstick
  for g in graphs:
    assert g['types'].shape == (g['edges'].shape[0],) and g['types'].dtype == np.int32
    assert not g['types'].size or (g['types'].min() >= 0 and g['types'].max() < E)
  assert tg.max_row_entries(graphs, E) == eg.conv_cap(N) <= ops.kstep_row_cap(Np)
  for b, g in enumerate(graphs):
    if not g['n']:
      continue
    n = g['n']
    rows = [eg.row_entries(tg.channel_graph(g, c)) for c in range(E + 1)]
    assert list(rows[0][n - 4:]) == [eg.conv_cap(N), 8, 9, 1]
    assert list(rows[1][n - 4:]) == [eg.conv_cap(N), 1, 2, 1]                # all of n - 4's edges are type 0
    assert list(rows[2][n - 4:]) == [1, 8, 8, 1]                             # exactly 8 with the diagonal, twice
    assert all((r == 1).any() for r in rows[1:])                             # identity rows in every type channel
    if E == 3 and b == 1:
      assert (rows[3] == 1).all() and (g['types'] != 2).all()                # a type that is entirely absent
    elif g['edges'].shape[0] > 100:
      assert all((g['types'] == t).any() for t in range(E))


def test_layer_case_and_shuffle_keep_the_typed_edge_set():
  graphs, N = tg.layer_case(2)
  assert len(graphs) == 9 and N == 130 and tg.max_row_entries(graphs, 2) <= eg.conv_cap(N)
  mixed = tg.shuffled(graphs, 41)
  for g, m in zip(graphs, mixed):
    key = lambda x: sorted((min(u, v), max(u, v), t) for (u, v), t in zip(x['edges'].tolist(), x['types'].tolist()))  # noqa: E731
    assert key(g) == key(m) and not np.array_equal(g['edges'], m['edges'])
  A = tg.dense_adjs(graphs, N, 2)
  assert A.shape == (9, N, N, 2) and (A.sum(3) <= 1).all() and (A == A.transpose(0, 2, 1, 3)).all()


def test_collate_graph_edges_refuses_malformed_edge_types_on_the_host():
  from lanczosnet_amd.dataset import collate_graph_edges
  graphs, N = tg.case('n301', 2)
  its = tg.items(graphs, 2)

  def broken(**change):
    out = [dict(it) for it in its]
    out[1].update(change)
    return out
  m = its[1]['edge_type'].shape[0]
  missing = [dict(it) for it in its]
  del missing[1]['edge_type']
  cases = [(missing, 'item 1 has no .edge_type'), (broken(edge_type=its[1]['edge_type'][:-1]), 'item 1: edge_type of shape'),
           (broken(edge_type=its[1]['edge_type'].astype(np.float32)), 'item 1: edge_type of dtype'),
           (broken(edge_type=np.full(m, 2, np.int32)), r'item 1: an edge type outside \[0, 2\)'),
           (broken(edge_type=np.full(m, -1, np.int32)), r'item 1: an edge type outside \[0, 2\)')]
  for bad, match in cases:
    with pytest.raises(ValueError, match=match):
      collate_graph_edges(bad, 20, device='cpu', num_edge_type=2)            # (raised before any upload)
  with pytest.raises(ValueError, match='num_edge_type=8'):
    collate_graph_edges(its, 20, device='cpu', num_edge_type=8)
  with pytest.raises(ValueError, match=r'item 0: an edge type outside \[0, 1\)'):
    collate_graph_edges(its, 20, device='cpu', num_edge_type=1)              # one type: every type must be 0


def test_fixture_channels_are_the_fp64_formula():
  """tests/golden/typed_edges.npz: the reference's get_laplacian('L4') per channel, rebuilt here from the
  stored edges and types by the helper's fp64 formula: 1e-7 (the project's L4 bar)."""
  z = np.load(GOLDEN)
  E, N = int(z['num_edge_type']), int(z['N'])
  off, n = z['edge_off'], z['n_nodes']
  assert z['L'].shape == (len(n), N, N, E + 1) and z['L'].dtype == np.float32
  for b in range(len(n)):
    g = dict(n=int(n[b]), edges=z['edges'][off[b]:off[b + 1]], types=z['edge_type'][off[b]:off[b + 1]])
    want = tg.dense_l4_fp64(g, N, E)
    err = np.abs(z['L'][b].astype(np.float64) - want).max()
    assert err <= 1e-7, err


def test_typed_sparse_laplacian_answers_like_the_dense_tensor_and_names_the_dense_limit():
  import torch
  from lanczosnet_amd import ops
  B, N, E = 1, 4096, 2
  z = torch.zeros((B,), dtype=torch.int32)
  imgs = ops.LargeSparseImages(torch.zeros((E + 1, B, N, 128), dtype=torch.int32),
                               torch.zeros((E + 1, B, N), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32), 128)
  sl = ops.SparseLaplacian(B, N, z, imgs.channel(0), torch.zeros((0, 2), dtype=torch.int32),
                           torch.zeros((B + 1,), dtype=torch.int64), E + 1, torch.zeros((0,), dtype=torch.int32), imgs)
  assert tuple(sl.shape) == (B, N, N, E + 1) and sl.to('cpu') is sl and sl.images.R == E + 1
  assert sl.image.entries.data_ptr() == imgs.entries.data_ptr() and sl.image.flags is imgs.flags
  with pytest.raises(ops.NotSupported, match='8192'):                        # (E + 1) N = 12288: no dense form
    sl.to_dense()
  assert [bit for bit, _ in ops.EDGE_TYPED_STATUS_REASONS] == [1, 2, 4, 8, 16, 32]
