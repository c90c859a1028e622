"""Input families for the hand-written full eigendecomposition (csrc/sym_eigh.hip and the bisection /
inverse-iteration bodies of csrc/tridiag_eig.hpp) at its kernel seams and beyond L4 Laplacians,
shared by the CPU checks of the inputs (test_eigh_cases_cpu.py) and the GPU tests of the kernels
(test_gpu_full_eigh_edges.py).

Plain numpy, fixed seeds.  The families that ritz_cases.py already has (spread, graded, paired,
scaled, wilkinson, random_symmetric, non_l4_operators) and its reference and checker (pad_batch,
eigh_ref, check_bars, tie_order) are used from there; this module adds the sizes at which the
kernels of the full decomposition change path, the matrices on which Householder meets a zero
column, exact multiplicities, and the checker of clustered spectra.

`bar_batches()` lists every (batch, K) that the GPU module holds to `check_bars`; the CPU module
walks the same list, so that the two cannot drift apart."""
import collections
import functools

import numpy as np

import ritz_cases as rc

# panel seams (NB = 32 columns), tile seams (TS = 64) and a last panel of one column
SEAM_N = (1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 193)
SEAM_K256 = (3, 129, 193)            # K = MAX_K = 256 > n
WILKINSON_M = (16, 32, 48)           # n = 33, 65, 97: beyond one panel
SPECTRA_N = (65, 129)
# 2^+-60 beside the 2^+-20 of ritz_cases.SCALES: the float32 matrix stays an exact multiple and
# squares stay far inside double range
SCALES = (2.0 ** -60, 2.0 ** -20, 2.0 ** 20, 2.0 ** 60)
assert SCALES[1] == rc.SCALES[0] and SCALES[2] == rc.SCALES[-1]

Batch = collections.namedtuple('Batch', 'label A ns names Ks')


def tridiagonal(n, seed):
  """A symmetric tridiagonal matrix with random entries: every Householder column below the
  sub-diagonal is zero (tau = 0, beta = alpha)."""
  rs = np.random.RandomState(seed)
  T = np.diag(rs.randn(n))
  i = np.arange(n - 1)
  T[i, i + 1] = T[i + 1, i] = 0.5 * rs.randn(n - 1)
  return T.astype(np.float32)


def seam_sizes(N):
  """n = N, N - 1, 3, 2, 1 and 0, those that fit an N tile, each once."""
  sizes = []
  for n in (N, N - 1, 3, 2, 1, 0):
    if 0 <= n <= N and n not in sizes:
      sizes.append(n)
  return sizes


def seam_K(N):
  """K = 1 and 15, 16, 17 around the KC = 16 columns of a back-transformation workgroup, min(N, 64)
  (n = 2K - 1, 2K, 2K + 1 of the candidate seam at N = 31 / 32 / 33 with K = 16 and at N = 128 /
  129 with K = 64, where the batch carries n = 127, 128 and 128, 129), and MAX_K = 256 > n."""
  Ks = {1, 15, 16, 17, min(N, 64)}
  if N in SEAM_K256:
    Ks.add(256)
  return tuple(sorted(Ks))


@functools.lru_cache(maxsize=None)
def seam_batch(N):
  """Graphs of n = N, N - 1, 3, 2, 1 and 0 nodes inside an N tile as dense symmetric matrices with
  a simple spectrum — the small ones ride column launches whose j >= n —, and from N = 31 on a
  diagonal and a tridiagonal matrix of n = N.  -> A, n_nodes, names"""
  cases = [('sym%d_in%d' % (n, N), rc.random_symmetric(n, 2000 + 40 * N + i))
           for i, n in enumerate(seam_sizes(N))]
  if N >= 31:
    cases.append(rc.spread(N)[1])
    cases.append(('tridiag%d' % N, tridiagonal(N, 3000 + N)))
  A, ns = rc.pad_batch(cases, N)
  return A, ns, [c[0] for c in cases]


def spectra(n):
  return rc.spread(n) + rc.graded(n) + rc.paired(n)


def _batch(label, cases, Ks, N=None):
  A, ns = rc.pad_batch(cases, N)
  return Batch(label, A, ns, [c[0] for c in cases], tuple(Ks))


@functools.lru_cache(maxsize=None)
def seam_batches():
  return tuple(Batch('seam%d' % N, *seam_batch(N), seam_K(N)) for N in SEAM_N)


@functools.lru_cache(maxsize=None)
def spectra_batches():
  """spread + graded + paired at n = 65 and 129; Wilkinson W+ at m = 16, 32, 48 in all five forms,
  K even (an odd K cuts a pair); the operators that are no L4 Laplacian at K = 32 >= n."""
  out = [_batch('spectra%d' % n, spectra(n), (16, 64)) for n in SPECTRA_N]
  out += [_batch('wilkinson%d' % m, rc.wilkinson(m), (16, 2 * m)) for m in WILKINSON_M]
  out.append(_batch('non_l4', rc.non_l4_operators(), (32,), 32))
  return tuple(out)


SCALED_K = (16, 64)


@functools.lru_cache(maxsize=None)
def scale_free_bases():
  """The two batches of the scale test, unscaled."""
  return (_batch('spectra65', spectra(65), SCALED_K), _batch('wilkinson32', rc.wilkinson(32), SCALED_K))


@functools.lru_cache(maxsize=None)
def scaled_batch(which, s):
  base = scale_free_bases()[which]
  cases = rc.scaled([(nm, base.A[b]) for b, nm in enumerate(base.names)], s)
  assert all(np.array_equal(A.astype(np.float64), base.A[b].astype(np.float64) * s)
             for b, (_, A) in enumerate(cases))          # an exact multiple
  return _batch('%s_x2^%d' % (base.label, int(np.log2(s))), cases, SCALED_K)


def scaled_batches():
  return tuple(scaled_batch(w, s) for s in SCALES for w in (0, 1))


def bar_batches():
  """Every batch that the GPU module holds to ritz_cases.check_bars, with the K it uses."""
  return seam_batches() + spectra_batches() + scaled_batches()


@functools.lru_cache(maxsize=None)
def reference(label, K):
  """eigh_ref of the batch `label` at K, computed once and shared (left unchanged by its users)."""
  b = {x.label: x for x in bar_batches()}[label]
  return rc.eigh_ref(b.A, b.ns, K)


# ------------------------------------------------------------------------------ exact multiplicities
@functools.lru_cache(maxsize=None)
def clustered():
  """(name, matrix): the zero matrix (tnorm = 0), c I (one cluster of K vectors), a diagonal with
  each of 20 values five times (in shuffled places), and three copies of one dense matrix whose
  blocks of 43 straddle columns 32, 64 and 96 — every eigenvalue exactly triple, T does not split."""
  vals = np.repeat(np.linspace(0.05, 1.0, 20), 5)
  vals = vals[np.random.RandomState(51).permutation(100)]
  S = rc.random_symmetric(43, 52)
  return (('zero40', np.zeros((40, 40), np.float32)),
          ('0.75I_70', (0.75 * np.eye(70)).astype(np.float32)),
          ('diag20x5', np.diag(vals).astype(np.float32)),
          ('3xsym43', np.kron(np.eye(3, dtype=np.float32), S).astype(np.float32)))


CLUSTER_K = (16, 64)
TOL_INSIDE = 1e-5


def check_clusters(A, ns, K, D, V, info, names=None, say=None):
  """The check of test_degenerate_spectra (test_gpu_full_eigh.py) with every figure relative to
  max |lambda| of the graph (1 for the zero matrix): info == 0, padding exactly zero, the sorted D
  within 1e-6 of the sorted reference, |V^T V - I| < 2e-6, |A V - V D| < 2e-6, every computed
  vector inside numpy's eigenspace of its eigenvalue to 1e-5, and numpy's projector to 1e-5 for
  the clusters that the cut keeps whole.  For the zero matrix D is exactly 0.
  -> the worst (D, orthogonality, residual, containment, projector) figures."""
  assert (np.asarray(info) == 0).all(), info
  Dr, _, full = rc.eigh_ref(A, ns, K)
  worst = np.zeros(5)
  for b in range(A.shape[0]):
    n, tag = int(ns[b]), (names[b] if names else b)
    kk = min(K, n)
    assert np.isfinite(D[b]).all() and np.isfinite(V[b]).all(), tag
    assert (D[b, kk:] == 0).all() and (V[b, n:] == 0).all() and (V[b, :, kk:] == 0).all(), tag
    if n == 0:
      continue
    Ab = A[b, :n, :n].astype(np.float64)
    e, U = np.linalg.eigh(Ab)
    scale = float(np.abs(e).max())
    if scale == 0.0:
      assert (D[b] == 0).all(), tag
      scale = 1.0
    Db, Vb = D[b, :kk].astype(np.float64), V[b, :n, :kk].astype(np.float64)
    fig = np.array([np.abs(np.sort(Db) - np.sort(Dr[b, :kk].astype(np.float64))).max() / scale,
                    np.abs(Vb.T @ Vb - np.eye(kk)).max(),
                    np.abs(Ab @ Vb - Vb * Db).max() / scale, 0.0, 0.0])
    assert fig[0] < rc.TOL_D and fig[1] < rc.TOL_ORTH and fig[2] < rc.TOL_RES, (tag, K, fig.tolist())
    whole = 0
    for val in np.unique(np.round(Db / scale, 6)) * scale:
      mine = np.where(np.abs(Db - val) < 1e-5 * scale)[0]
      theirs = np.where(np.abs(e - val) < 1e-5 * scale)[0]
      assert len(mine) and len(mine) <= len(theirs), (tag, val, len(mine), len(theirs))
      Uc, Vc = U[:, theirs], Vb[:, mine]
      fig[3] = max(fig[3], np.abs(Vc - Uc @ (Uc.T @ Vc)).max())
      if len(mine) == len(theirs):   # the cut keeps the cluster whole
        whole += 1
        fig[4] = max(fig[4], np.abs(Vc @ Vc.T - Uc @ Uc.T).max())
    assert fig[3] < TOL_INSIDE and fig[4] < rc.TOL_PROJ, (tag, K, fig.tolist())
    if say is not None:
      say('%s n=%d K=%d: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  containment %.2e  projector %.2e '
          '(%d whole clusters)' % ((tag, n, K) + tuple(fig) + (whole,)))
    worst = np.maximum(worst, fig)
  return worst
