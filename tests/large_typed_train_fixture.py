"""Planted inputs of the typed-batch backward checks (tests/test_gpu_large_typed_train.py and the CPU check of
their preconditions in tests/test_large_typed_train_cpu.py): numpy only.

EXACT cases of lnz_large_grad_input_channels in the manner of tests/large_train_fixture.py's `input_case`:
every operand is a small integer, every product and every partial sum an integer below 2^24, so the fp32
result must EQUAL the float64 one whatever the summation order.  The builder asserts that precondition on its
own inputs (`_check_below` on the sums of ABSOLUTE products).

Typed graphs: the graphs of tests/edge_graphs.py with an edge type drawn per edge from a seeded RandomState."""
import functools

import numpy as np

import edge_graphs as eg
from large_edges_fixture import EXACT_LIMIT, _check_below, _ints, _sparse_signs

# (B, N, K, R, d)
INPUT_SHAPES = [
    (3, 193, 1, 3, 1),        # the smallest typed batch, one column, one row in the fourth 64-row tile
    (3, 257, 17, 8, 127),     # the channel limit, an odd width, K no multiple of 4, one row in the fifth tile
    (10, 300, 64, 3, 128),    # the K limit, the full width, B not a multiple of 8
    (3, 256, 20, 4, 10),      # the reference's configuration; N exactly four tiles
    (2, 65, 0, 3, 128),       # no long scales: V and dY None
]


@functools.lru_cache(maxsize=None)
def input_channels_case(B, N, K, R, d):
  """dZ [R,B,N,128] in -4..4, Wn [R,128,128] in -2..2 (columns >= d zero), V signs [B,N,K], dY [B,K,128] in
  -8..8 with junk integers in its columns >= d (the launch masks them) -> dX [B,N,128], columns >= d zero.
  K = 0: V and dY are None."""
  rs = np.random.RandomState(7 * N + K + d + B + 1000 * R)
  dZ = _ints(rs, (R, B, N, 128), -4, 4)
  Wn = _ints(rs, (R, 128, 128), -2, 2, density=0.6)
  Wn[:, :, d:] = 0
  full = np.einsum('cbno,coi->bni', dZ, Wn)
  bound = np.einsum('cbno,coi->bni', np.abs(dZ), np.abs(Wn))
  V = dY = None
  if K:
    V = _sparse_signs(rs, B, N, K, 40)
    dY = _ints(rs, (B, K, 128), -8, 8)
    full = full + V @ dY
    bound = bound + np.abs(V) @ np.abs(dY)
    assert d == 128 or np.abs(dY[..., d:]).max() > 0
  ref = np.zeros((B, N, 128))
  ref[..., :d] = full[..., :d]
  worst = _check_below('input_channels_case(%d, %d, %d, %d, %d)' % (B, N, K, R, d), bound)
  assert np.abs(ref).max() > 0
  # every channel matters: dropping one changes the result
  for c in range(R):
    assert np.abs(np.einsum('bno,oi->bni', dZ[c], Wn[c])).max() > 0
  assert B < 9 or not np.array_equal(dZ[0, 0], dZ[0, 8])
  f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
  return dict(dZ=f32(dZ), Wn=f32(Wn), V=f32(V), dY=f32(dY), dX=ref, worst=worst)


def all_exact_cases():
  """Build every case (each asserts its own precondition) -> the worst bound met."""
  worst = max(input_channels_case(*shape)['worst'] for shape in INPUT_SHAPES)
  assert worst < EXACT_LIMIT
  return worst


# ---- typed graphs ------------------------------------------------------------------------------------------
def with_types(graphs, E, seed):
  """The same graphs, every edge with a type in [0, E) drawn from RandomState(seed)."""
  rs = np.random.RandomState(seed)
  return [dict(g, edge_type=rs.randint(0, E, size=g['edges'].shape[0]).astype(np.int32)) for g in graphs]


def b10_graphs():
  """B 10, nodes [257] + [200 + 6 i]: seven edge types on ~6 neighbours per node, so many nodes have no edge
  of some type (that channel's row is its single diagonal entry)."""
  rs = np.random.RandomState(1000)
  ns = [257] + [200 + 6 * i for i in range(9)]
  return [dict(n=n, edges=eg.gnp_edges(n, 6.0 / n, rs)) for n in ns], 257


# name -> (graphs, N, E): the batches of the split-gather check
def gather_case(name):
  if name == 'n301 E2':
    graphs, N = eg.case('n301')
    return with_types(graphs, 2, 31), N, 2
  if name == 'B10 E7':
    graphs, N = b10_graphs()
    return with_types(graphs, 7, 32), N, 7
  if name == 'n2100 E2':
    graphs, N = eg.case('n2100')
    return with_types(graphs, 2, 33), N, 2
  raise KeyError(name)


GATHER_CASES = ('n301 E2', 'B10 E7', 'n2100 E2')


def pack_typed(graphs):
  """-> edges [m,2] int32, edge_off [B+1] int64, n_nodes [B] int32, edge_type [m] int32 (numpy)."""
  edges, off, n = eg.pack(graphs)
  et = np.concatenate([g['edge_type'].reshape(-1) for g in graphs]).astype(np.int32)
  return edges, off, n, et


def channel_row_entries(g, E):
  """[E + 1, n]: entries per row of every channel's image (1 + neighbours; channel 1 + e: of type e)."""
  n = g['n']
  out = np.ones((E + 1, n), np.int64)
  e, t = g['edges'], g['edge_type']
  if e.size:
    out[0] += np.bincount(e.reshape(-1), minlength=n)
    for k in range(E):
      out[1 + k] += np.bincount(e[t == k].reshape(-1), minlength=n)
  return out


def l4_channels_float64(g, E, N):
  """[E + 1, N, N] float64: L4 = D^-1/2 (I + A) D^-1/2 of the simple graph and of every edge type alone, each
  with its own degrees (rows at or beyond the graph's nodes zero)."""
  n = g['n']
  L = np.zeros((E + 1, N, N))
  cnt = channel_row_entries(g, E)
  e, t = g['edges'], g['edge_type']
  for c in range(E + 1):
    s = 1.0 / np.sqrt(cnt[c].astype(np.float64))
    sel = e if c == 0 else e[t == c - 1]
    u, v = sel[:, 0], sel[:, 1]
    L[c, u, v] = s[u] * s[v]
    L[c, v, u] = s[u] * s[v]
    i = np.arange(n)
    L[c, i, i] = s * s
  return L
