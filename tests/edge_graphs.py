"""Seeded graphs of the edge-list tests (tests/test_edge_collate_cpu.py, tests/test_gpu_edge_collate.py):
both sides build the SAME graphs from numpy RandomState alone.  A graph is a dict(n=nodes, edges=[m,2]
int32, each undirected edge once); a case is a list of graphs and the padded N."""
import numpy as np


def gnp_edges(n, p, rs):
  """The edges of a G(n, p)-like graph without an n x n array: round(p n (n-1) / 2) distinct pairs."""
  m = int(round(p * n * (n - 1) / 2))
  if n < 2 or m == 0:
    return np.zeros((0, 2), np.int32)
  u = rs.randint(0, n, size=2 * m + 16)
  v = rs.randint(0, n, size=2 * m + 16)
  keep = u != v
  lo, hi = np.minimum(u, v)[keep], np.maximum(u, v)[keep]
  code = np.unique(lo.astype(np.int64) * n + hi)
  code = code[rs.permutation(code.shape[0])[:m]]
  return np.stack([code // n, code % n], axis=1).astype(np.int32)


def with_special_rows(n, edges, conv_cap):
  """The last four nodes of the graph get rows of exactly 1 (isolated), 8, 9 and conv_cap entries
  (the diagonal included): their random edges are dropped and they are wired to disjoint runs of
  the first nodes, every one of which gains one neighbour at most."""
  assert n >= conv_cap + 24
  special = np.arange(n - 4, n)
  keep = ~(np.isin(edges[:, 0], special) | np.isin(edges[:, 1], special))
  out, at = [edges[keep]], 0
  for node, entries in ((n - 3, 8), (n - 2, 9), (n - 4, conv_cap)):
    nb = np.arange(at, at + entries - 1, dtype=np.int32)
    at += entries - 1
    out.append(np.stack([nb, np.full_like(nb, node)], axis=1))
  return np.concatenate(out, axis=0).astype(np.int32)


def row_entries(g):
  """Entries per row of the graph's Laplacian image: 1 + neighbours."""
  deg = np.bincount(g['edges'].reshape(-1), minlength=g['n']) if g['edges'].size else np.zeros(g['n'], np.int64)
  return deg + 1


def max_row_entries(graphs):
  return max([int(row_entries(g).max()) for g in graphs if g['n'] > 0] + [0])


def conv_cap(N):   # (ops.large_sparse_row_cap restated: the CPU tests check the two agree)
  return int(min(256, max(32, (N // 32 + 7) // 8 * 8)))


# name -> (B, N, p, seed): the ragged batches of the image / Ritz / module checks.  Graph 0 has N nodes,
# the last graph is EMPTY (no node, no edge), the ones between lose 7 nodes each.
CASES = {
    'n301': (3, 301, 0.02, 11),
    'n256': (2, 256, 0.03, 12),
    'n200': (2, 200, 0.05, 13),
    'n2100': (2, 2100, 0.004, 14),     # wide by size
    'n300': (2, 300, 0.02, 15),        # (wide by steps: M = 72)
    'n4096': (2, 4096, 0.002, 16),     # the no-dense-tensor check
}


def case(name, special=True):
  """-> (graphs, N).  special: the engineered rows (1, 8, 9, conv_cap entries) in every non-empty graph."""
  B, N, p, seed = CASES[name]
  rs = np.random.RandomState(seed)
  graphs = []
  for b in range(B):
    n = N if b == 0 else (0 if b == B - 1 else N - 7 * b)
    if name == 'n4096' and b == B - 1:
      n = N - 9          # (two real graphs there: the peak is measured on a full batch)
    e = gnp_edges(n, p, rs)
    if special and n > 0:
      e = with_special_rows(n, e, conv_cap(N))
    graphs.append(dict(n=n, edges=e))
  return graphs, N


def star_case():
  """A star on 301 nodes (a row of 301 entries: beyond every capacity) next to an ordinary graph."""
  rs = np.random.RandomState(21)
  star = np.stack([np.zeros(300, np.int32), np.arange(1, 301, dtype=np.int32)], axis=1)
  return [dict(n=301, edges=star), dict(n=290, edges=gnp_edges(290, 0.02, rs))], 301


def small_case():
  """Graphs of 20 .. 100 nodes: below the K-step territory."""
  rs = np.random.RandomState(22)
  return [dict(n=n, edges=gnp_edges(n, 0.1, rs)) for n in (20, 57, 100, 64)], 100


def shuffled(graphs, seed):
  """The same edge SETS: every graph's edges permuted, about half of them with swapped endpoints."""
  rs = np.random.RandomState(seed)
  out = []
  for g in graphs:
    e = g['edges'][rs.permutation(g['edges'].shape[0])].copy()
    swap = rs.rand(e.shape[0]) < 0.5
    e[swap] = e[swap][:, ::-1]
    out.append(dict(n=g['n'], edges=np.ascontiguousarray(e)))
  return out


def pack(graphs):
  """-> edges [E,2] int32, edge_off [B+1] int64, n_nodes [B] int32 (numpy)."""
  edges = np.concatenate([g['edges'].reshape(-1, 2) for g in graphs], axis=0).astype(np.int32)
  off = np.zeros(len(graphs) + 1, np.int64)
  np.cumsum([g['edges'].shape[0] for g in graphs], out=off[1:])
  return edges, off, np.array([g['n'] for g in graphs], np.int32)


def dense_adjs(graphs, N):
  """[B,N,N,1] float32 0/1 adjacency (the dense route's input)."""
  A = np.zeros((len(graphs), N, N, 1), np.float32)
  for b, g in enumerate(graphs):
    e = g['edges']
    A[b, e[:, 0], e[:, 1], 0] = 1.0
    A[b, e[:, 1], e[:, 0], 0] = 1.0
  return A


def l4_rows_fp64(g):
  """Per row the ascending columns and fp64 values s_i s_j of L4 = D^-1/2 (I + A) D^-1/2."""
  n, e = g['n'], g['edges']
  s = 1.0 / np.sqrt(row_entries(g).astype(np.float64))
  nb = [[i] for i in range(n)]
  for u, v in e.tolist():
    nb[u].append(v)
    nb[v].append(u)
  rows = []
  for i in range(n):
    c = np.array(sorted(nb[i]), np.int64)
    rows.append((c, s[i] * s[c]))
  return rows


def items(graphs, dim=10, seed=5, dense=False):
  """The collate items of the graphs: node_feat [n, dim], label [1, 2]; edges, or (dense) adjs [n,n,1]."""
  rs = np.random.RandomState(seed)
  out = []
  for g in graphs:
    n = g['n']
    it = dict(node_feat=rs.randn(n, dim).astype(np.float32), label=rs.randn(1, 2))
    if dense:
      it['adjs'] = dense_adjs([g], n)[0]
    else:
      it['edges'] = g['edges']
    out.append(it)
  return out
