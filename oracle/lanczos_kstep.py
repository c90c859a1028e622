"""Oracle (test infrastructure): K-step Lanczos Ritz pairs for LARGE graphs (BASELINE config 5).

The reference's Lanczos branch for large graphs is `scipy.sparse.linalg.eigsh(L, k, which='LM')`
(ARPACK implicitly restarted Lanczos, `utils/data_helper.py:205-208`, third-party, scipy 1.15.3
here).  The HIP kernel `lnz_lanczos_ritz_large` is a plain M-step Lanczos with full
re-orthogonalisation (no implicit restarts) — a different function from ARPACK for unconverged
pairs (SURVEY.md F8, §8d "Config 5").  Its parity is therefore pinned two ways:
  * `lanczos_kstep_fp64` below: fp64 restatement of the SAME M-step algorithm (same start vector,
    classical Gram-Schmidt with a second pass on cancellation or where the carried bound asks for it,
    early stop on a breakdown relative to the matrix' scale) — Ritz values / Ritz-vector subspace compared directly;
  * `eigsh` (the reference's call): the converged leading Ritz pairs must agree with it, and every
    Ritz pair must satisfy the Lanczos residual bound |A v - theta v| = beta_M |e_M^T s|.
"""
import numpy as np


def start_vector(n):
  lanes = np.arange(n, dtype=np.uint64)
  h = ((lanes + np.uint64(1)) * np.uint64(2654435761)) & np.uint64(0xffffffff)
  return 1.0 + ((h >> np.uint64(8)) & np.uint64(0xffff)).astype(np.float64) / 65536.0


def lanczos_kstep_fp64(A, M, K, tol=1e-8, reorth=1e-6, rule='bound', scale='relative', stats=None):
  """A [n,n] symmetric (float32 values, promoted), M Lanczos steps, top-K Ritz pairs by |theta|.
  Returns D [K], V [n,K], (alpha, beta, steps_done, last norm).
  The two data-dependent rules (oracle/cgs_bound.py, csrc/wave.hpp):
  rule — when the second classical Gram-Schmidt pass of a step runs.  'bound' (the kernels'): where
    the first pass removed more than 1 - `reorth` of |w|^2, or where the carried bound on the loss
    of orthogonality asks for it; 'fraction': the 1 - `reorth` test alone, on the norm that is left
    (the kernels' rule before the bound: it lets the loss of orthogonality compound on spectra
    that are not an L4 Laplacian's); 'always'.
  scale — what the early stop |w| <= tol * s is relative to.  'relative': s = 2^ceil(log2 max |a_ij|)
    (1 for an L4 Laplacian with an entry in (1/2, 1], 0 for the zero matrix); 'absolute': s = 1, the
    kernels' stop before — a matrix times 2^-30 stopped after one step.
  stats: a dict that receives the number of second passes and the largest accepted bound."""
  from .cgs_bound import OrthBound, cgs2, matrix_scale
  assert rule in ('bound', 'fraction', 'always') and scale in ('relative', 'absolute')
  A = np.asarray(A, dtype=np.float32).astype(np.float64)
  n = A.shape[0]
  M = min(M, n)
  Q = np.zeros((M, n))
  alpha = np.zeros(M)
  beta = np.zeros(M)
  stop = tol * (matrix_scale(A) if scale == 'relative' else 1.0)
  frac = float(np.float32(1.0 - reorth))   # (the kernels hold the fraction as a float)
  ob = OrthBound()
  w = start_vector(n)
  nrm = np.sqrt(w @ w)
  steps = 0
  for j in range(M):
    if j > 0 and nrm <= stop:
      break  # invariant subspace: stop, remaining slots stay zero
    if j > 0:
      beta[j - 1] = nrm
    q = w / nrm
    Q[j] = q
    w = A @ q
    if rule == 'fraction':
      coef = 0.0
      n0 = w @ w
      for p in range(2):
        if p == 1 and w @ w >= reorth * n0:
          break
        ob.second_passes += p
        c = Q[:j + 1] @ w
        w = w - Q[:j + 1].T @ c
        coef += c[j]
    else:
      w, coef = cgs2(Q, w, j, rule, ob, frac=frac)
      ob.accept()
    alpha[j] = coef
    nrm = np.sqrt(w @ w)
    steps = j + 1
  if stats is not None:
    stats.update(second_passes=ob.second_passes, bound=float(np.sqrt(ob.worst)))
  D = np.zeros(K)
  V = np.zeros((n, K))
  if steps == 0:   # (an empty graph takes no step at all)
    return D, V, (alpha, beta, 0, 0.0)
  T = np.diag(alpha[:steps]) + np.diag(beta[:steps - 1], 1) + np.diag(beta[:steps - 1], -1)
  th, S = np.linalg.eigh(T)
  idx = np.argsort(-np.abs(th), kind='mergesort')
  kk = min(K, steps)
  D[:kk] = th[idx[:kk]]
  V[:, :kk] = Q[:steps].T @ S[:, idx[:kk]]
  return D, V, (alpha, beta, steps, nrm)
