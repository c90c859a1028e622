"""Typed versions of the seeded graphs of tests/edge_graphs.py (tests/test_typed_edges_cpu.py,
tests/test_gpu_typed_edges.py): the same graphs, every edge with a type in [0, E) drawn from a seeded
RandomState.  A typed graph is dict(n, edges [m,2] int32, types [m] int32).  In every non-empty graph
the engineered rows of edge_graphs.with_special_rows (the last four nodes: conv_cap, 8, 9, 1 entries)
are typed so that
  * the conv_cap-entry node (n - 4) has ALL its edges of type 0: channels 0 and 1 are both at the capacity;
  * the 9-entry node (n - 2) has seven neighbours of type 1 and one of type 0: channel 2's row holds
    exactly 8 entries with the diagonal;
  * the 8-entry node (n - 3) has all its edges of type 1 (a node with a single type);
  * node n - 4 has no type-1 edge and the isolated node n - 1 no edge at all: identity rows;
and graph 1 of an E = 3 case has no edge of type 2 at all (they are moved to type 1)."""
import numpy as np

import edge_graphs as eg


def add_types(graphs, E, seed):
  rs = np.random.RandomState(seed)
  out = []
  for b, g in enumerate(graphs):
    n, e = g['n'], g['edges']
    ty = rs.randint(0, E, size=e.shape[0]).astype(np.int32)
    if n > 0:
      touches = lambda node: (e[:, 0] == node) | (e[:, 1] == node)   # noqa: E731
      ty[touches(n - 4)] = 0
      ty[touches(n - 3)] = 1
      nine = np.flatnonzero(touches(n - 2))
      assert nine.shape[0] == 8
      ty[nine] = 1
      ty[nine[0]] = 0
      if E == 3 and b == 1:
        ty[ty == 2] = 1
    out.append(dict(n=n, edges=e, types=ty))
  return out


def case(name, E, special=True):
  """-> (typed graphs, N): edge_graphs.case(name) with types of seed 100 + E."""
  graphs, N = eg.case(name, special=special)
  return add_types(graphs, E, 100 + E), N


def layer_case(E=2):
  """Nine graphs padded to 130 nodes (a batch over more than one XCD round of the gather), real edges, no
  engineered rows (130 nodes are fewer than with_special_rows needs)."""
  rs = np.random.RandomState(23)
  graphs = []
  for b in range(9):
    n = 130 - 3 * b
    e = eg.gnp_edges(n, 0.06, rs)
    graphs.append(dict(n=n, edges=e, types=rs.randint(0, E, size=e.shape[0]).astype(np.int32)))
  return graphs, 130


def pack(graphs):
  """-> edges [m,2] int32, edge_off [B+1] int64, n_nodes [B] int32, edge_type [m] int32 (numpy)."""
  edges, off, n = eg.pack(graphs)
  return edges, off, n, np.concatenate([g['types'] for g in graphs]).astype(np.int32)


def channel_graph(g, c):
  """The untyped graph of operator channel c: every edge (c = 0) or the edges of type c - 1."""
  e = g['edges'] if c == 0 else g['edges'][g['types'] == c - 1]
  return dict(n=g['n'], edges=e)


def channel_rows_fp64(g, c):
  """edge_graphs.l4_rows_fp64 of channel c: per row the ascending columns and the fp64 values s_i s_j with
  the degrees of THAT channel's graph (1 + the node's neighbours in the channel)."""
  return eg.l4_rows_fp64(channel_graph(g, c))


def max_row_entries(graphs, E):
  return max(eg.max_row_entries([channel_graph(g, c) for g in graphs]) for c in range(E + 1))


def dense_adjs(graphs, N, E):
  """[B,N,N,E] float32 0/1 typed adjacency (the dense route's input)."""
  A = np.zeros((len(graphs), N, N, E), np.float32)
  for b, g in enumerate(graphs):
    e, t = g['edges'], g['types']
    A[b, e[:, 0], e[:, 1], t] = 1.0
    A[b, e[:, 1], e[:, 0], t] = 1.0
  return A


def dense_l4_fp64(g, N, E):
  """[N,N,E+1] float64: the collated L of one graph from the fp64 formula."""
  L = np.zeros((N, N, E + 1), np.float64)
  for c in range(E + 1):
    for i, (cols, v) in enumerate(channel_rows_fp64(g, c)):
      L[i, cols, c] = v
  return L


def shuffled(graphs, seed):
  """The same typed edge SETS: every graph's edges permuted (types with them), about half with swapped endpoints."""
  rs = np.random.RandomState(seed)
  out = []
  for g in graphs:
    p = rs.permutation(g['edges'].shape[0])
    e, t = g['edges'][p].copy(), g['types'][p].copy()
    swap = rs.rand(e.shape[0]) < 0.5
    e[swap] = e[swap][:, ::-1]
    out.append(dict(n=g['n'], edges=np.ascontiguousarray(e), types=t))
  return out


def items(graphs, E, dim=10, seed=5, dense=False):
  """The collate items: edge_graphs.items plus edge_type, or (dense) the typed adjs [n,n,E]."""
  out = eg.items(graphs, dim=dim, seed=seed)
  for it, g in zip(out, graphs):
    if dense:
      del it['edges']
      it['adjs'] = dense_adjs([g], g['n'], E)[0]
    else:
      it['edge_type'] = g['types']
  return out
