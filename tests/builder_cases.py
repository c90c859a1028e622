"""Case tables for the batch builders — lnz_laplacian_l4, lnz_laplacian, lnz_collate_qm8 (csrc/laplacian.hip,
csrc/collate.hip) — and for the segment-sum operator and lnz_embedding_grad of csrc/laplacian.hip, shared by
the CPU checks of the cases (test_builder_cases_cpu.py) and the GPU tests of the kernels
(test_gpu_laplacian_edges.py, test_gpu_collate_edges.py, test_segment_sum_reference.py).

Plain numpy, fixed seeds.  Beside the tables stand a plain restatement of each launcher's selection rule
(`l4_route`, `segsum_forward_route`, `segsum_backward_route`, `collate_lds_bytes`), so that the CPU module
can show that every row sits on the seam it claims, the float64 reference of a batch (`reference`,
oracle.get_laplacian per molecule and channel), the bar (`check_bar`) and a numpy emulation of the kernels'
arithmetic (`emulate`), which shows the bar reachable before a GPU is involved.

Nearly every other GPU test builds its operator with ops.laplacian_l4 and hands the same L to the kernel
under test and to its reference: a wrong Laplacian cancels out of them.  These are the cases that hold the
builders themselves."""
import collections
import functools

import numpy as np

import oracle

LDS_MAX = 64 * 1024

# ------------------------------------------------------------------------------------ launcher rules
def l4_degree_bytes(N, E):
  return (E + 1) * N * 8


def l4_staged_bytes(N, E):
  """degrees (rounded up to an even count of doubles: the stage starts 16-byte aligned) + the [N, N, E] block"""
  return (((E + 1) * N + 1) & ~1) * 8 + N * N * E * 4


def l4_route(N, E, aligned=True):
  """lnz_laplacian_l4's choice: 'refused' (LNZ_ENOTSUP, lnz_laplacian too), 'staged' or 'direct'."""
  if l4_degree_bytes(N, E) > LDS_MAX:
    return 'refused'
  if l4_staged_bytes(N, E) <= LDS_MAX and (N * N * E) % 4 == 0 and aligned:
    return 'staged'
  return 'direct'


def l4_kernel_name(route):
  return 'laplacian_l4_kernel<%s>' % route


def kind_kernel_name(kind):
  return 'laplacian_kind_kernel<%d>' % int(kind[1])


def collate_lds_bytes(N, E):
  return (E + 1) * N * 8 + N * N * E * 4


def segsum_forward_route(B, D1, D2, S, aligned=True):
  """lnz_unsorted_segment_sum_forward's choice -> dict(kernel, vec, nw, lds, blocks)"""
  vec4 = D2 % 4 == 0 and D2 >= 128 and aligned
  cw = 256 if vec4 else 64
  copy = S * cw * 4
  if copy > LDS_MAX:
    total = B * D1 * D2
    grid = min(2048, (total + 255) // 256)
    return dict(kernel='segsum_fwd_atomic_kernel', vec=0, nw=0, lds=0, blocks=grid,
                turns=-(-total // (grid * 256)))
  blocks = (D2 + cw - 1) // cw
  nw = 1
  while nw < 4 and B * blocks * nw < 512 and copy * (nw * 2) <= LDS_MAX and D1 >= 16 * nw * 2:
    nw *= 2
  vec = 4 if vec4 else 1
  return dict(kernel='segsum_fwd_lds_kernel<%d> x %d' % (vec, nw), vec=vec, nw=nw, lds=copy * nw, blocks=blocks,
              last_width=D2 - (blocks - 1) * cw, rows_per_wave=(D1 + nw - 1) // nw)


def segsum_backward_route(B, D1, D2, S, aligned=True):
  vec = 4 if D2 % 4 == 0 and aligned else 1
  rows = B * D1
  waves = 4 * max(1, min(4096, (rows + 3) // 4))
  return dict(kernel='segsum_bwd_kernel<%d>' % vec, rows=rows, waves=waves)


# ------------------------------------------------------------------------------------- the L4 table
# (N, E, route, the seam the row sits on)
L4_SHAPES = (
    (4, 1, 'staged', '4 float4s: 252 lanes of the first round clamp their load'),
    (5, 4, 'staged', '(E+1) N = 25 is odd: the stage offset is rounded up'),
    (26, 6, 'staged', 'QM8'),
    (27, 4, 'staged', 'odd product, 729 float4s'),
    (48, 4, 'staged', '2304 float4s: second turn of the 2048-float4 outer loop'),
    (100, 1, 'staged', '2500 float4s'),
    (126, 1, 'staged', '65520 B, the last shape that stages; 3969 float4s'),
    (5, 1, 'direct', 'N N E is odd'),
    (3, 2, 'direct', 'N N E % 4 = 2'),
    (127, 1, 'direct', 'odd'),
    (128, 1, 'direct', 'first shape too large to stage'),
    (64, 4, 'direct', 'too large to stage with four bond types (N = 62 is the last that does)'),
)
UNALIGNED_SHAPES = ((26, 6), (4, 1))    # staged when aligned, direct from a view one float into a buffer
REFUSED_SHAPE = (1025, 7)               # (E+1) N = 8200 > 8192
KIND_SHAPES = ((27, 4), (64, 4))        # one staged-size, one direct-size
KINDS = (('L1', 0.5), ('L2', 0.5), ('L3', 0.5), ('L4', 0.5), ('L5', 0.5), ('L6', 0.5), ('L7', 0.5),
         ('L6', 0.3), ('L6', 1.0))
SPECIAL_SHAPES = KIND_SHAPES            # the L4-only zero / negative row sums
CONTENTS = ('bonds', 'weighted')
SPECIALS = ('zero_sum', 'negative_sum')

Batch = collections.namedtuple('Batch', 'label N E content adjs counts')


def counts_of(N):
  """n = 0, 1, N, one in between, N + 3 (clamped: the bits of n = N) and -2 (the same as 0)"""
  return np.array([0, 1, N, max(2, (N + 1) // 2) if N > 2 else 1, N + 3, -2], np.int32)


def clamp(n, N):
  return min(max(int(n), 0), N)


def _bond_graph(rs, n, E):
  """symmetric bond counts in {1, 2} (at least one 2 from three atoms on), the last atom without a bond and,
  with several bond types, the last type absent"""
  A = np.zeros((n, n, E), np.float32)
  m = n - 1 if n >= 3 else n               # atoms that may bond
  for i in range(m):
    for j in range(i + 1, m):
      if j == i + 1 or rs.rand() < 2.0 / m:   # a chain + a few rings
        A[i, j, rs.randint(0, max(1, E - 1))] = 1 + (rs.rand() < 0.3)
  if m >= 2:
    e = int(np.argmax(A[0, 1]))
    A[0, 1, e] = 2
  return A + A.transpose(1, 0, 2)


def _weighted_graph(rs, n, E):
  """non-negative, non-symmetric float weights, row n // 2 all zero, every other row positive"""
  A = (rs.rand(n, n, E) * (rs.rand(n, n, E) < 0.5)).astype(np.float32)
  for i in range(n):
    A[i, (i + 1) % n, :] += np.float32(0.25)
  A[n // 2] = 0
  return A


def _special_graph(rs, n, E, which):
  """a weighted graph whose row n // 2 holds a_ii alone, in bond type 0: -1 (the row sum of I + A is exactly
  0 in channels 0 and 1) or -3 (negative there)"""
  A = _weighted_graph(rs, n, E)
  r = n // 2
  A[r, r, 0] = -1.0 if which == 'zero_sum' else -3.0
  return A


@functools.lru_cache(maxsize=None)
def batch(N, E, content):
  """The six molecules of `counts_of(N)` in an [6, N, N, E] tile, padding zero.  Molecule 4 (count N + 3)
  carries molecule 2's adjacency, molecule 5 (count -2) a full tile that must not be read."""
  rs = np.random.RandomState(1000 * N + 10 * E + len(content))
  counts = counts_of(N)
  draw = {'bonds': _bond_graph, 'weighted': _weighted_graph}.get(content)
  adjs = np.zeros((len(counts), N, N, E), np.float32)
  for b, c in enumerate(counts):
    n = clamp(c, N)
    if b == 4:
      adjs[4] = adjs[2]
    elif b == 5:
      adjs[5] = adjs[2]
    elif n:
      adjs[b, :n, :n] = draw(rs, n, E) if draw else _special_graph(rs, n, E, content)
  adjs.setflags(write=False)
  return Batch('%s_%dx%d' % (content, N, E), N, E, content, adjs, counts)


def l4_batches():
  """every batch that test_gpu_laplacian_edges.py gives to lnz_laplacian_l4, with its route"""
  out = [(batch(N, E, c), route) for (N, E, route, _) in L4_SHAPES for c in CONTENTS]
  out += [(batch(N, E, c), l4_route(N, E)) for (N, E) in SPECIAL_SHAPES for c in SPECIALS]
  return out


def kind_batches():
  return [batch(N, E, c) for (N, E) in KIND_SHAPES for c in CONTENTS]


def with_padding(bt, fill):
  """bt.adjs with every entry of i >= n or j >= n replaced: 'junk' (finite) or 'nan'"""
  rs = np.random.RandomState(7)
  A = np.array(bt.adjs)
  junk = (100.0 * rs.randn(*A.shape)).astype(np.float32) if fill == 'junk' else np.full(A.shape, np.nan, np.float32)
  for b, c in enumerate(bt.counts):
    n = clamp(c, bt.N)
    pad = np.ones((bt.N, bt.N), bool)
    pad[:n, :n] = False
    A[b][pad] = junk[b][pad]
  return A


# --------------------------------------------------------------------------------- reference and bar
def _one_laplacian(A, kind, alpha):
  if kind == 'L1' and A.shape[0] == 1:
    # get_laplacian raises here as the reference does (np.diag of a 0-d array): D - A stated directly
    return np.array([[A.sum()]]) - A
  with np.errstate(divide='ignore', invalid='ignore'):
    return oracle.get_laplacian(A, kind, alpha)


@functools.lru_cache(maxsize=None)
def reference(N, E, content, kind='L4', alpha=0.5):
  """float64 [6, N, N, E + 1]: oracle.get_laplacian per molecule and channel on the clamped n x n block,
  channel 0 on adjs.sum(2) as oracle.laplacian_multi_l4 lays it out; zero padding.  Shared, never written."""
  bt = batch(N, E, content)
  ref = np.zeros(bt.adjs.shape[:3] + (E + 1,), np.float64)
  for b, c in enumerate(bt.counts):
    n = clamp(c, N)
    if n == 0:
      continue
    A = bt.adjs[b, :n, :n].astype(np.float64)
    ref[b, :n, :n, 0] = _one_laplacian(A.sum(axis=2), kind, alpha)
    for e in range(E):
      ref[b, :n, :n, 1 + e] = _one_laplacian(A[:, :, e], kind, alpha)
  ref.setflags(write=False)
  return ref


REL, ABS = 2.0 ** -23, 2.0 ** -40


def check_bar(got, ref, counts, tag, l4_rule=False):
  """|got - ref| <= 2^-23 |ref| + 2^-40 max |ref| per element, the maximum over the molecule and channel
  (one rounding to float32 costs half an ulp, the first term is twice that; the second absorbs the fp64
  row-sum order, pow against np.power and L1's cancellation on the diagonal — 2^16 below float32
  resolution).  Padding exactly zero.  NaN exactly where the reference has NaN — or, under l4_rule
  (lnz_laplacian_l4), a row and column of exact zeros where the reference's row sum of I + A is negative
  (its d^-1/2, hence its diagonal entry, is NaN).  -> (worst achieved / bar, elements != float32(ref))"""
  got = np.asarray(got)
  assert got.dtype == np.float32 and got.shape == ref.shape, (tag, got.dtype, got.shape)
  N = ref.shape[1]
  worst, differ = 0.0, 0
  for b, c in enumerate(counts):
    n = clamp(c, N)
    assert not got[b, n:].any() and not got[b, :, n:].any(), (tag, b, 'padding is not exact zeros')
    for ch in range(ref.shape[3]):
      r, g = ref[b, :n, :n, ch], got[b, :n, :n, ch].astype(np.float64)
      keep = np.ones((n, n), bool)
      if l4_rule:
        neg = np.isnan(np.diag(r))
        assert not g[neg].any() and not g[:, neg].any(), (tag, b, ch, 'negative row sum: zero row and column')
        keep[neg] = False
        keep[:, neg] = False
      r, g = r[keep], g[keep]
      nan = np.isnan(r)
      assert np.array_equal(np.isnan(g), nan), (tag, b, ch, 'NaN pattern')
      r, g = r[~nan], g[~nan]
      if r.size == 0:
        continue
      bar = REL * np.abs(r) + ABS * np.abs(r).max()
      err = np.abs(g - r)
      ok = err <= bar
      assert ok.all(), (tag, 'molecule %d channel %d' % (b, ch), float(err[~ok].max()), float(np.abs(r).max()))
      if bar.max() > 0:
        worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()))
      differ += int((g.astype(np.float32) != r.astype(np.float32)).sum())
  return worst, differ


def emulate(adjs, counts, kind='L4', alpha=0.5, l4_entry=False):
  """The kernels' arithmetic in numpy: the fp64 row sum in the kernel's order (j ascending, for channel 0 the
  bond types of a pair in turn), s = deg^-x with the inf -> 0 guard (l4_entry: 1 / sqrt and s = 0 unless
  deg > 0), (s_i m) s_j, one rounding to float32."""
  B, N, _, E = adjs.shape
  k = int(kind[1])
  plus_identity = k in (4, 5)
  expo = 0.5 if k in (2, 4) else (alpha if k == 6 else 1.0)
  out = np.zeros((B, N, N, E + 1), np.float32)
  for b, c in enumerate(counts):
    n = clamp(c, N)
    if n == 0:
      continue
    A = adjs[b, :n, :n].astype(np.float64)
    eye = np.eye(n)
    for ch in range(E + 1):
      deg = np.full(n, 1.0 if plus_identity else 0.0)
      for j in range(n):
        for e in (range(E) if ch == 0 else (ch - 1,)):
          deg = deg + A[:, j, e]
      if ch == 0:
        M = np.zeros((n, n))
        for e in range(E):
          M = M + A[:, :, e]
      else:
        M = A[:, :, ch - 1]
      with np.errstate(divide='ignore', invalid='ignore'):
        if l4_entry:
          s = np.where(deg > 0.0, 1.0 / np.sqrt(deg), 0.0)
        elif k == 1:
          s = deg
        else:
          s = np.power(deg, -expo)
          s[np.isinf(s)] = 0.0
        if k == 1:
          r = eye * s[:, None] - M
        else:
          m = eye + M if plus_identity else M
          r = (s[:, None] * m) * s[None, :] if k in (2, 4, 6) else s[:, None] * m
          if k in (2, 3):
            r = eye - r
      out[b, :n, :n, ch] = r.astype(np.float32)
  return out


# ------------------------------------------------------------------------------------------ collate
COLLATE_SHAPES = ((2, 1, 1), (30, 12, 300), (126, 1, 16), (51, 6, 16))    # (N, E, P): the last two are the last accepted
COLLATE_REFUSED = ((127, 1), (52, 6))

Molecule = collections.namedtuple('Molecule', 'name atoms bonds label')   # bonds: (u, v, type)


def _random_bonds(rs, n, E, count):
  return [(int(rs.randint(n)), int(rs.randint(n)), int(rs.randint(E))) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def collate_molecules(N, E, P):
  """The molecules of a hand-built shard for an [N, N, E] tile."""
  rs = np.random.RandomState(100 * N + E)
  lab = lambda: rs.randn(P).astype(np.float32)            # noqa: E731
  atoms = lambda n: rs.randint(1, 70, size=n).astype(np.uint8)   # noqa: E731
  n = N                      # the hand-made bonds below need two atoms
  mols = [Molecule('no_bonds', atoms(min(N, 5)), [], lab()),
          # a bond listed twice (count 2), a self bond (counted once), a type >= E and an atom >= n (both dropped)
          Molecule('twice_self_dropped', atoms(n),
                   [(0, 1, 0), (0, 1, 0), (1, 1, E - 1), (0, 1, E), (1, 0, 255), (0, n, 0), (n + 3, 1, 0)], lab()),
          # larger than the tile: cut to its first N atoms, bonds into the cut atoms dropped
          Molecule('oversized', atoms(N + 2),
                   [(0, 1, 0), (0, N, 0), (N + 1, 1, 0), (N, N + 1, 0)] + _random_bonds(rs, N + 2, E, 2 * N), lab()),
          Molecule('full', atoms(N), _random_bonds(rs, N, E, 3 * N), lab())]
  if N == 126:
    mols.append(Molecule('many_bonds', atoms(N), _random_bonds(rs, N, E, 300), lab()))   # the strided bond loop
  return tuple(mols)


def truncated(mol, N):
  """the molecule cut to its first N atoms (what the collate makes of a larger one)"""
  return Molecule(mol.name + '_cut', mol.atoms[:N], [(u, v, t) for (u, v, t) in mol.bonds if u < N and v < N],
                  mol.label)


def pack_bonds(bonds):
  return np.array([u | v << 8 | t << 16 for (u, v, t) in bonds], np.uint32)


def shard_arrays(mols):
  """(mol_off, edge_off, atoms, edges as int32, labels) of the packed shard of dataset/packed.py"""
  mol_off = np.concatenate([[0], np.cumsum([len(m.atoms) for m in mols])]).astype(np.int64)
  edge_off = np.concatenate([[0], np.cumsum([len(m.bonds) for m in mols])]).astype(np.int64)
  atoms = np.concatenate([m.atoms for m in mols]).astype(np.uint8)
  edges = np.concatenate([pack_bonds(m.bonds) for m in mols] + [np.zeros(1, np.uint32)]).view(np.int32)
  labels = np.stack([m.label for m in mols]).astype(np.float32)
  return mol_off, edge_off, atoms, edges, labels


def collate_ids(n_mol):
  """every molecule, ids outside [0, n_mol) — negative and too large —, and a repeated id"""
  return np.array(list(range(n_mol)) + [-1, n_mol, 2 ** 40, 1, -2 ** 40], np.int64)


def collate_expected(mols, ids, N, E):
  """-> node_feat, node_mask, label, n_nodes (exact) and the dense float32 adjacency [B, N, N, E] of the batch"""
  P = len(mols[0].label)
  B = len(ids)
  node_feat, mask = np.zeros((B, N), np.int64), np.zeros((B, N), np.uint8)
  label, n_nodes = np.zeros((B, P), np.float32), np.zeros(B, np.int32)
  adjs = np.zeros((B, N, N, E), np.float32)
  for b, i in enumerate(ids):
    if not 0 <= i < len(mols):
      continue                                   # an empty molecule with a zero label
    m = truncated(mols[int(i)], N)
    n = len(m.atoms)
    node_feat[b, :n], mask[b, :n], label[b], n_nodes[b] = m.atoms, 1, m.label, n
    adjs[b, :n, :n] = oracle.dense_from_edges(n, pack_bonds(m.bonds), E)
  return node_feat, mask, label, n_nodes, adjs


def collate_reference(adjs, n_nodes):
  """float64 oracle.laplacian_multi_l4 of every molecule's n x n block"""
  B, N, _, E = adjs.shape
  ref = np.zeros((B, N, N, E + 1), np.float64)
  for b, n in enumerate(n_nodes):
    if n:
      ref[b, :n, :n] = oracle.laplacian_multi_l4(adjs[b, :n, :n].astype(np.float64))
  return ref


# ------------------------------------------------------------------------- segment sum, embedding grad
# (B, D1, D2, S, aligned, kernel, what the row is for)
SEGSUM_FORWARD = (
    (2, 64, 40, 64, True, 'segsum_fwd_lds_kernel<1> x 4', '65536 B of LDS'),
    (3, 200, 36, 11, True, 'segsum_fwd_lds_kernel<1> x 4', '50 rows per wave: a ragged last group of the 4-row pipeline'),
    (2, 65, 36, 11, True, 'segsum_fwd_lds_kernel<1> x 4', 'the last wave gets 14 of 17 rows'),
    (3, 70, 132, 16, True, 'segsum_fwd_lds_kernel<4> x 4', '65536 B; one column block of width 132'),
    (2, 49, 260, 8, True, 'segsum_fwd_lds_kernel<4> x 2', 'two column blocks, the last of width 4'),
    (2, 33, 128, 64, True, 'segsum_fwd_lds_kernel<4> x 1', '65536 B'),
    (2, 33, 128, 65, True, 'segsum_fwd_atomic_kernel', 'one pass'),
    (8, 300, 220, 300, True, 'segsum_fwd_atomic_kernel', '528000 elements > 2048 x 256: the grid-stride loop turns'),
    (3, 70, 132, 16, False, 'segsum_fwd_lds_kernel<1> x 4', 'a view one float into a buffer: equals the aligned result'),
)
SEGSUM_FORWARD_OUT_OF_RANGE = 1       # the row that also runs with ids of -1, S and 2^31 planted
SEGSUM_BACKWARD = (
    (300, 64, 4, 7, 'segsum_bwd_kernel<4>', '19200 rows > 16384 waves: the wave-stride loop turns'),
    (5, 40, 37, 11, 'segsum_bwd_kernel<1>', 'scalar columns'),
)


def segsum_inputs(B, D1, D2, S, seed, out_of_range=False):
  """integer-valued data in [-8, 8] (every order of summation is exact), per-batch ids in [0, S); with
  out_of_range, ids of -1, S and 2^31 planted in every batch entry"""
  rs = np.random.RandomState(seed)
  data = rs.randint(-8, 9, size=(B, D1, D2)).astype(np.float32)
  ids = rs.randint(0, S, size=(B, D1)).astype(np.int64)
  if out_of_range:
    for b in range(B):
      where = rs.choice(D1, size=6, replace=False)
      ids[b, where] = [-1, S, 2 ** 31, -1, S, 2 ** 31]
  return data, ids


def segsum_forward_rule(data, ids, S):
  """out[b, ids[b, c]] += data[b, c], an id outside [0, S) adds nothing"""
  B, D1, D2 = data.shape
  out = np.zeros((B, S, D2), np.float64)
  for b in range(B):
    ok = (ids[b] >= 0) & (ids[b] < S)
    np.add.at(out[b], ids[b][ok], data[b][ok].astype(np.float64))
  return out


def segsum_backward_rule(gout, ids):
  """gdata[b, c] = gout[b, ids[b, c]], zeros for an id outside [0, S)"""
  B, S, D2 = gout.shape
  ok = (ids >= 0) & (ids < S)
  g = gout[np.arange(B)[:, None], np.where(ok, ids, 0)]
  return np.where(ok[:, :, None], g, np.float32(0))


# lnz_embedding_grad rows with integer-valued dx and equality: (B, N, width, atoms, chunks) -> (kernel, ids)
EMBEDDING_EXACT = {
    (20, 32, 64, 3, 2): ('embedding_grad_kernel<1>', 'equal'),    # 64 hits per 64-row step: the 8-deep batch turns 8 times
    (1, 1, 128, 5, 3): ('embedding_grad_kernel<2>', 'random'),    # more chunks than rows
}
