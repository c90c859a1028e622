"""Input families for the full-length Ritz kernels (csrc/lanczos_ritz.hip, csrc/lanczos_ritz_wg.hip)
beyond the L4 Laplacians of molecules, shared by the CPU tests of the kernel's mirror
(test_ritz_cases_cpu.py) and the GPU tests of the kernels (test_gpu_ritz_edges.py).

Plain numpy, fixed seeds.  Every builder returns a list of (name, float32 [n, n] symmetric matrix).
The reference of every test is np.linalg.eigh of the FLOAT32 matrix in float64 + the |lambda|
mergesort (`eigh_ref`), and the bars are the project's own taken relative to max |lambda| of the
case (`check_bars`)."""
import functools

import numpy as np

import oracle

WILKINSON_M = (8, 9, 10, 12, 13, 14)
WILKINSON_FORMS = ('plain', 'over16', 'minus3', 'negated', 'permuted')
SCALES = (2.0 ** -20, 2.0 ** -10, 2.0 ** 10, 2.0 ** 20)

# the project's bars (tests/test_gpu_parity.py), relative to max |lambda| of the case
TOL_D, TOL_ORTH, TOL_RES, TOL_PROJ = 1e-6, 2e-6, 2e-6, 1e-5


def _rotation(n, seed):
  q, _ = np.linalg.qr(np.random.RandomState(seed).randn(n, n))
  return q


def _sym32(Q, lam):
  A = (Q * lam) @ Q.T
  return (0.5 * (A + A.T)).astype(np.float32)


def spread(n):
  """Equispaced spectrum k / n, k = 1 .. n: rotated, and the plain diagonal."""
  lam = np.arange(1, n + 1) / n
  return [('spread%d_rot' % n, _sym32(_rotation(n, 100 + n), lam)),
          ('spread%d_diag' % n, np.diag(lam).astype(np.float32))]


def graded(n):
  """Six decades: Q diag(logspace(-6, 0, n)) Q^T."""
  return [('graded%d' % n, _sym32(_rotation(n, 200 + n), np.logspace(-6, 0, n)))]


def paired(n):
  """Q diag(+-linspace(.1, 1, n / 2)) Q^T (an odd n adds one eigenvalue 0.05): every |lambda| twice,
  once with either sign.  The float32 rounding of the matrix moves the two copies ~1e-8 apart, so
  their order in the |lambda| sort is decided — by eigenvalues that have to be right to 1e-9."""
  l = np.linspace(0.1, 1.0, n // 2)
  lam = np.concatenate([l, -l] + ([[0.05]] if n % 2 else []))
  return [('paired%d' % n, _sym32(_rotation(n, 300 + n), lam))]


def scaled(mats, s):
  """Every matrix times the power of two s: the float32 matrix is an exact multiple."""
  return [('%s_x2^%d' % (name, int(np.log2(s))), (A * np.float32(s)).astype(np.float32)) for name, A in mats]


def wilkinson_matrix(m):
  """W+_{2m+1}: diagonal |i - m|, off-diagonals 1.  Its largest eigenvalues agree pairwise to ~1e-14
  with no weak coupling between the two copies."""
  n = 2 * m + 1
  W = np.diag(np.abs(np.arange(n) - m).astype(np.float64))
  i = np.arange(n - 1)
  W[i, i + 1] = W[i + 1, i] = 1.0
  return W


def wilkinson(m, forms=WILKINSON_FORMS):
  W = wilkinson_matrix(m)
  n = W.shape[0]
  perm = np.random.RandomState(400 + m).permutation(n)
  made = {'plain': W, 'over16': W / 16.0, 'minus3': W - 3.0 * np.eye(n), 'negated': -W,
          'permuted': W[np.ix_(perm, perm)]}
  return [('wilkinson%d_%s' % (m, f), made[f].astype(np.float32)) for f in forms]


def wilkinson_family():
  return [c for m in WILKINSON_M for c in wilkinson(m)]


def small_graphs():
  """name -> adjacency of a path, a ring, a star and a G(n, 0.3)."""
  gs = {}
  n = 13
  a = np.zeros((n, n)); i = np.arange(n - 1); a[i, i + 1] = a[i + 1, i] = 1.0
  gs['path13'] = a
  n = 24
  r = np.zeros((n, n)); i = np.arange(n); r[i, (i + 1) % n] = r[(i + 1) % n, i] = 1.0
  gs['ring24'] = r
  n = 17
  s = np.zeros((n, n)); s[0, 1:] = s[1:, 0] = 1.0
  gs['star17'] = s
  n = 32
  g = np.triu((np.random.RandomState(11).rand(n, n) < 0.3).astype(np.float64), 1)
  gs['gnp32'] = g + g.T
  return gs


def non_l4_operators():
  """Raw adjacency, L1 = D - A (norm up to twice the largest degree) and L2 = I - D^-1/2 A D^-1/2
  of the small graphs."""
  out = []
  for name, adj in small_graphs().items():
    out.append((name + '_adj', adj.astype(np.float32)))
    out.append((name + '_L1', oracle.get_laplacian(adj, 'L1').astype(np.float32)))
    out.append((name + '_L2', oracle.get_laplacian(adj, 'L2').astype(np.float32)))
  return out


def random_symmetric(n, seed):
  """A dense symmetric matrix with a simple spectrum in about [-1, 1]."""
  g = np.random.RandomState(seed).randn(n, n)
  return ((g + g.T) / np.sqrt(8.0 * max(n, 1))).astype(np.float32)


# (N, K) of the one-wavefront kernel: every tile size x the store paths — K <= 64 with 64 / K = 64,
# 21, 3, 2, 1 node rows per pass, and the K > 64 loop
SHAPES = [(1, 1), (1, 3), (1, 65), (2, 1), (2, 20), (2, 100), (15, 3), (15, 33), (15, 64),
          (16, 1), (16, 32), (16, 65), (17, 20), (17, 64), (17, 100), (31, 3), (31, 32), (31, 65),
          (32, 1), (32, 3), (32, 20), (32, 32), (32, 33), (32, 64), (32, 65), (32, 100)]


@functools.lru_cache(maxsize=None)
def shape_batch(N):
  """Eight graphs in an N tile: n = N, 0 and sizes from 1 up to N - 1, dense symmetric matrices
  with a simple spectrum (a top-K cut never falls into a cluster).  -> A, n_nodes, names"""
  sizes = [N, 0] + [max(1, int(round(N * f))) for f in (0.125, 0.25, 0.375, 0.5, 0.75)] + [max(1, N - 1)]
  cases = [('sym%d_%d' % (n, i), random_symmetric(n, 1000 + 40 * N + i)) for i, n in enumerate(sizes)]
  A, ns = pad_batch(cases, N)
  return A, ns, [c[0] for c in cases]


def pad_batch(cases, N=None):
  """[(name, A)] -> A [B, N, N] float32 zero padded, n_nodes [B] int32."""
  ns = np.array([A.shape[0] for _, A in cases], np.int32)
  N = int(ns.max()) if N is None else N
  out = np.zeros((len(cases), N, N), np.float32)
  for b, (_, A) in enumerate(cases):
    out[b, :ns[b], :ns[b]] = A
  return out, ns


def eigh_ref(A, ns, K):
  """The reference: eigh of each float32 block in float64, descending |lambda| by a stable
  mergesort, collated like the dataset.  -> D [B, K], V [B, N, K] float32, the full spectra."""
  Dl, Vl = [], []
  for b in range(A.shape[0]):
    n = int(ns[b])
    e, v = np.linalg.eigh(A[b, :n, :n].astype(np.float64))
    idx = np.argsort(-np.abs(e), kind='mergesort')
    Dl.append(e[idx]); Vl.append(v[:, idx])
  D, V = oracle.collate_eigs(Dl, Vl, A.shape[1], K)
  return D, V, Dl


def tie_order(d, full, kk, scale):
  """Permutation of the first kk slots that puts every group of equal |lambda| into ascending
  order (-lambda before +lambda, the mergesort's order of an exact tie).  The groups are those of
  the reference spectrum `full`: slots whose |lambda| differ by less than 1e-7 of the largest (the
  project's cut gap: the float32 matrix does not resolve less).  Inside such a group — the +-lambda
  pairs of a bipartite graph's adjacency, of `paired` — the order is decided by the last bit of two
  numbers that are equal in exact arithmetic, in eigh as in the kernel; applied to both sides,
  slots compare one to one wherever the order is defined and as sorted groups where it is not."""
  perm = np.arange(len(d))
  mag = np.abs(np.asarray(full[:kk], np.float64))
  start = 0
  for i in range(1, kk + 1):
    if i == kk or mag[i - 1] - mag[i] >= oracle.CUT_GAP * scale:
      perm[start:i] = start + np.argsort(np.asarray(d[start:i], np.float64), kind='mergesort')
      start = i
  return perm


def check_bars(A, ns, K, D, V, ref, names=None, say=None):
  """Every graph of the batch against `ref` = eigh_ref(A, ns, K), each bar relative to the graph's
  max |lambda|: |D - D_ref| < 1e-6 (slot by slot, groups of tied |lambda| in the order of
  `tie_order`), |V^T V - I| < 2e-6, |A V - V D| < 2e-6, the spectral projectors of powers 1, 5, 30
  within 1e-5; D exactly zero beyond min(K, n), V exactly zero in rows >= n and columns >=
  min(K, n).  No graph may have its cut inside a cluster (nothing is skipped).
  -> the worst (D, orthogonality, residual, projector) figures."""
  from graph_fixture import check_ritz
  Dr, Vr, full = ref
  worst = np.zeros(4)
  for b in range(A.shape[0]):
    n, tag = int(ns[b]), (names[b] if names else b)
    kk = min(K, n)
    assert np.isfinite(D[b]).all() and np.isfinite(V[b]).all(), tag
    assert (D[b, kk:] == 0).all() and (V[b, n:] == 0).all() and (V[b, :, kk:] == 0).all(), tag
    if n == 0:
      continue
    Ab = A[b, :n, :n].astype(np.float64)
    scale = float(np.abs(full[b]).max())
    scale = scale if scale > 0 else 1.0
    assert not oracle.degenerate_cut(full[b] / scale, K), tag
    pg, pr = tie_order(D[b], full[b], kk, scale), tie_order(Dr[b], full[b], kk, scale)
    Dg, Vg, Dq, Vq = D[b][pg], V[b][:, pg], Dr[b][pr], Vr[b][:, pr]
    mags = np.abs(D[b, :kk].astype(np.float64))
    assert (mags[:-1] - mags[1:] > -TOL_D * scale).all(), tag   # descending |lambda|
    Vb, Db = Vg[:n, :kk].astype(np.float64), Dg[:kk].astype(np.float64)
    fig = np.array([np.abs(Dg.astype(np.float64) - Dq).max() / scale,
                    np.abs(Vb.T @ Vb - np.eye(kk)).max(),
                    np.abs(Ab @ Vb - Vb * Db).max() / scale, 0.0])
    if say is not None:
      say('%s n=%d K=%d: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e' % ((tag, n, K) + tuple(fig[:3])))
    assert fig[0] < TOL_D and fig[1] < TOL_ORTH and fig[2] < TOL_RES, (tag, n, K, fig.tolist())
    s32 = np.float32(scale)
    _, fig[3], c = check_ritz((Dg / s32)[None], Vg[None], (Dq / s32)[None], Vq[None], [n],
                              [full[b] / scale], K, tol_d=TOL_D, tol_p=TOL_PROJ)
    assert c == 1, tag
    worst = np.maximum(worst, fig)
  return worst
