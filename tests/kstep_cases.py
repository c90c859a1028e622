"""Inputs for the K-step Lanczos kernels (csrc/lanczos_large.hip: dense stream, symmetric stream and
sliced-ELL image; csrc/lanczos_wide.hip) beyond L4 Laplacians of norm 1, shared by the CPU test of
the float64 restatement (test_kstep_cases_cpu.py) and the GPU test of the kernels
(test_gpu_kstep_edges.py).  Built on tests/ritz_cases.py; plain numpy, fixed seeds.

(a) `full_batches`: a tile of N = 64 run for M = 64 steps — a graph of n nodes stops by itself after
    n steps and the Ritz pairs ARE the eigenpairs: float64 eigh is the reference (ritz_cases.eigh_ref,
    check_bars).  Every case has a simple spectrum.
(b) `multiplicity_batch`: a Krylov method finds each distinct eigenvalue once — eigh is not the
    function; `distinct_eigenvalues` is.
(c) `seam_graphs`, `operator_cases`, `ragged_batch`, `row_cap_batch`: M < n, against the restatement
    (oracle.lanczos_kstep_fp64), one input per seam of the kernels.
(d) `scale_batches`: powers of two far beyond what an absolute 1e-8 survives."""
import functools

import numpy as np

import oracle
import ritz_cases as rc

N_FULL = 64
K_FULL = (1, 15, 16, 17, 64)
K_PAIRED = (2, 16, 18, 64)       # even: the cut never splits a +-lambda pair
BIG_SCALES = (2.0 ** -60, 2.0 ** -30, 2.0 ** 30, 2.0 ** 60)

# (c): every tile width at which the kernels take another path — the 16-row tiles of V = Q S, the
# 64-row slabs of the image and the diagonal quarters of the symmetric stream, its groups of 16 rows,
# the 256-column chunks, the 512-row Gram-Schmidt chunk of the wide kernel
SEAM_N = (4, 8, 60, 64, 68, 252, 256, 260, 516)
SEAM_M = (1, 2, 17, 64)
SEAM_K = (1, 16, 17, None)       # None: K = M
# the bars of tests/test_gpu_large.py against the restatement, relative to max |theta|
TOL_D, TOL_PROJ, TOL_ORTH = 1e-6, 1e-5, 1e-5


def gnp_adjacency(n, p, seed):
  a = np.triu((np.random.RandomState(seed).rand(n, n) < p).astype(np.float64), 1)
  return a + a.T


def connected(adj):
  """The graph with the path 0 - 1 - ... - n-1 added: connected, so the largest eigenvalue of its
  Laplacians is simple (a second component's copy of it would enter a Krylov space through rounding
  alone, differently in every implementation)."""
  adj = adj.copy()
  i = np.arange(adj.shape[0] - 1)
  adj[i, i + 1] = adj[i + 1, i] = 1.0
  return adj


def operators(tag, adj, kinds=('adj', 'L1', 'L2', 'L4')):
  out = []
  for k in kinds:
    A = adj if k == 'adj' else (oracle.laplacian_l4(adj) if k == 'L4' else oracle.get_laplacian(adj, k))
    out.append(('%s_%s' % (tag, k), np.asarray(A, np.float64).astype(np.float32)))
  return out


def _full_cases():
  cases, paired = [], []
  for n in (20, 63, 64):
    # (graded: the CPU test shows it inside a quarter of the bars; its smallest eigenvalues lie 2.4e-7 |A| apart)
    cases += rc.spread(n) + rc.graded(n) + [('sym%d' % n, rc.random_symmetric(n, 7000 + n))]
    paired += rc.paired(n)
  for c in rc.non_l4_operators():
    if c[0].startswith(('path13', 'gnp32')):
      # (a path is bipartite: its adjacency has every |lambda| twice, and goes with the even cuts)
      (paired if c[0] == 'path13_adj' else cases).append(c)
  cases += operators('gnp64', gnp_adjacency(64, 0.15, 64)) + operators('gnp60', gnp_adjacency(60, 0.2, 60))
  return cases, paired


def _passengers():
  """n = N, 0, N / 8 .. 3 N / 4, N - 1 (ritz_cases.shape_batch) and 3, 2, 1."""
  A, ns, names = rc.shape_batch(N_FULL)
  cases = [(names[b], A[b, :ns[b], :ns[b]]) for b in range(len(ns))]
  return cases + [('sym%d_tiny' % n, rc.random_symmetric(n, 7100 + n)) for n in (3, 2, 1)]


@functools.lru_cache(maxsize=None)
def full_batches():
  """-> [(tag, A [B, 64, 64], n_nodes, names, the K of the cut)]: the listed cases with the passengers
  in one batch, and the `paired` family with its even K."""
  cases, paired = _full_cases()
  out = []
  for tag, cs, ks in (('full', cases + _passengers(), K_FULL), ('paired', paired, K_PAIRED)):
    A, ns = rc.pad_batch(cs, N_FULL)
    out.append((tag, A, ns, [c[0] for c in cs], ks))
  return out


def min_relative_gap(A):
  e = np.linalg.eigvalsh(np.asarray(A, np.float64))
  return float(np.diff(e).min() / np.abs(e).max()) if len(e) > 1 else 1.0


# ---- (b) ---------------------------------------------------------------------------------------
def three_copies():
  blk = rc.spread(8)[0][1]
  A = np.zeros((24, 24), np.float32)
  for i in range(3):
    A[8 * i:8 * i + 8, 8 * i:8 * i + 8] = blk
  return A


@functools.lru_cache(maxsize=None)
def multiplicity_batch():
  """-> A [B, 24, 24], n_nodes, names."""
  cs = [('zero24', np.zeros((24, 24), np.float32)), ('0.75I_24', (0.75 * np.eye(24)).astype(np.float32)),
        ('3x_spread8', three_copies())]
  cs += [c for c in rc.non_l4_operators() if c[0].startswith(('ring24', 'star17'))]
  A, ns = rc.pad_batch(cs, 24)
  return A, ns, [c[0] for c in cs]


def distinct_eigenvalues(A):
  """The distinct eigenvalues of the float32 matrix (float64 eigh; values within 1e-9 |A| are one),
  in the kernels' order: descending |lambda|, -lambda before +lambda."""
  e = np.linalg.eigvalsh(np.asarray(A, np.float64))
  scale = max(float(np.abs(e).max()), 1e-300)
  groups = [[e[0]]]
  for x in e[1:]:
    if x - groups[-1][-1] <= 1e-9 * scale:
      groups[-1].append(x)
    else:
      groups.append([x])
  d = np.array([np.mean(g) for g in groups])
  d[np.abs(d) <= 1e-9 * scale] = 0.0
  return d[np.argsort(-np.abs(d), kind='mergesort')]


def check_distinct(tag, A, D, V, info, K):
  """(b) for one graph: info = the number of distinct eigenvalues, the leading slots of D are those
  within the D bar, V^T V = I on them (and A V = V D), exact zeros behind."""
  n = A.shape[0]
  want = distinct_eigenvalues(A)
  r = len(want)
  scale = float(np.abs(want).max()) or 1.0
  kk = min(K, r)
  assert int(info) == r, (tag, int(info), r)
  assert (D[kk:] == 0).all() and (V[:, kk:] == 0).all() and (V[n:] == 0).all(), tag
  # (-lambda and +lambda tie in |lambda|: their order is rounding's, so tied slots compare as sorted groups)
  pg, pw = rc.tie_order(D, want, kk, scale)[:kk], rc.tie_order(want, want, kk, scale)[:kk]
  Vd, Dd, want = V[:n, pg].astype(np.float64), D[pg].astype(np.float64), want[pw]
  fig = (np.abs(Dd - want[:kk]).max() / scale, np.abs(Vd.T @ Vd - np.eye(kk)).max(),
         np.abs(A.astype(np.float64) @ Vd - Vd * Dd).max() / scale)
  assert fig[0] < rc.TOL_D and fig[1] < rc.TOL_ORTH and fig[2] < rc.TOL_RES, (tag, fig)
  return fig


# ---- (c) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_graphs(N):
  """Two operators on one connected G(N, p) of about eight neighbours per node: its L4 and its L1.  [2, N, N]"""
  adj = connected(gnp_adjacency(N, min(0.6, 8.0 / N), 500 + N))
  return np.stack([oracle.laplacian_l4(adj), oracle.get_laplacian(adj, 'L1')]).astype(np.float32)


def seam_shapes(N):
  """The (M, K) of tile width N: M of SEAM_M within N, K of SEAM_K within M."""
  out = []
  for M in SEAM_M:
    if M <= N:
      out += [(M, K) for K in sorted({min(M, k if k else M) for k in SEAM_K})]
  return out


@functools.lru_cache(maxsize=None)
def operator_cases():
  """L2 and L1 of G(128, 0.1) and G(256, 0.05): where the fraction rule loses the basis."""
  out = []
  for n, p in ((128, 0.1), (256, 0.05)):
    out += operators('gnp%d' % n, gnp_adjacency(n, p, 900 + n), ('L2', 'L1'))
  return out


OPERATOR_M = (32, 48, 64)
RAGGED_N, RAGGED_SIZES = 260, (260, 259, 100, 3, 0)


@functools.lru_cache(maxsize=None)
def ragged_batch():
  cs = []
  for i, n in enumerate(RAGGED_SIZES):
    if n == 0:
      cs.append(('ragged0', np.zeros((0, 0), np.float32)))
      continue
    adj = connected(gnp_adjacency(n, 8.0 / n if n > 16 else 0.0, 1300 + i))   # (n = 3: the path, three distinct eigenvalues)
    cs.append(('ragged%d' % n, np.asarray(oracle.get_laplacian(adj, 'L2') if i % 2 else oracle.laplacian_l4(adj),
                                          np.float32)))
  A, ns = rc.pad_batch(cs, RAGGED_N)
  return A, ns, [c[0] for c in cs]


ROW_CAP = 8


@functools.lru_cache(maxsize=None)
def row_cap_batch():
  """A path of 40 nodes whose node 0 carries extra leaves: row 0 of its L4 (the diagonal included)
  has exactly ROW_CAP entries in graph 0 and ROW_CAP + 1 in graph 1.  -> A [2, 48, 48], n_nodes, longest rows"""
  cs = []
  for extra in (ROW_CAP - 2, ROW_CAP - 1):
    n = 40 + extra
    adj = np.zeros((n, n))
    i = np.arange(39)
    adj[i, i + 1] = adj[i + 1, i] = 1.0
    adj[0, 40:] = adj[40:, 0] = 1.0
    cs.append(('hub%d' % extra, oracle.laplacian_l4(adj).astype(np.float32)))
  A, ns = rc.pad_batch(cs, 48)
  return A, ns, [int((c[1] != 0).sum(axis=1).max()) for c in cs]


def check_restatement(tag, A, M, K, D, V, info, say=None):
  """One graph (A [n, n], D [K], V [>= n, K]) against the restatement at the bars of
  tests/test_gpu_large.py relative to max |theta|; info = its step count; exact zeros beyond
  min(K, info) and in rows >= n.  -> (|D - D_ref|, projector, |V^T V - I|)"""
  n = A.shape[0]
  Dr, Vr, (_, _, steps, _) = oracle.lanczos_kstep_fp64(A, M, K)
  kk = min(K, steps)
  assert int(info) == steps, (tag, int(info), steps)
  assert np.isfinite(D).all() and np.isfinite(V).all(), tag
  assert (D[kk:] == 0).all() and (V[:, kk:] == 0).all() and (V[n:] == 0).all(), tag
  if kk == 0:
    return (0.0, 0.0, 0.0)
  scale = float(np.abs(Dr).max())
  scale = scale if scale > 0 else 1.0
  Vd = V[:n].astype(np.float64)
  fig = (np.abs(D - Dr).max() / scale, np.abs(Vd @ Vd.T - Vr @ Vr.T).max(),
         np.abs(Vd[:, :kk].T @ Vd[:, :kk] - np.eye(kk)).max())
  if say is not None:
    say('%s M=%d K=%d: |D-Dref| %.2e  projector %.2e  |VtV-I| %.2e  steps %d' % ((tag, M, K) + fig + (steps,)))
  assert fig[0] < TOL_D and fig[1] < TOL_PROJ and fig[2] < TOL_ORTH, (tag, M, K, fig)
  return fig


def cut_gap(A, M, K):
  """Relative gap in |theta| at the cut of the restatement's Ritz values (1 where nothing is cut):
  the projector of K Ritz vectors is only defined where it is not tiny."""
  D, _, (_, _, steps, _) = oracle.lanczos_kstep_fp64(A, M, M)
  if K >= steps:
    return 1.0
  mags = np.abs(D[:steps])
  return float((mags[K - 1] - mags[K]) / mags[0])


# ---- (d) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scale_base():
  """The n = 64 cases of (a) in one batch, and the three-copies case.  -> [(tag, A, n_nodes)]"""
  cases, paired = _full_cases()
  cs = [c for c in cases + paired if c[1].shape[0] == N_FULL]
  A, ns = rc.pad_batch(cs, N_FULL)
  return [('full64', A, ns), ('3x_spread8', three_copies()[None], np.array([24], np.int32))]
