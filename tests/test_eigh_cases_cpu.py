"""CPU checks of the inputs of test_gpu_full_eigh_edges.py (eigh_cases.py), so that a failure on the
GPU is never the fault of the inputs: no (batch, K) that the GPU module holds to `check_bars` cuts a
graph's spectrum inside a cluster, and the float64 reference rounded to float32 — the best any
kernel could return — meets every bar with each figure at most a quarter of it; the clustered
matrices have the multiplicities they claim and the rounded reference passes `check_clusters`."""
import numpy as np
import pytest

import oracle
import eigh_cases as ec
import ritz_cases as rc

QUARTER = 0.25 * np.array([rc.TOL_D, rc.TOL_ORTH, rc.TOL_RES, rc.TOL_PROJ])


def _rounded_reference_meets_a_quarter(batch):
  worst = np.zeros(4)
  for K in batch.Ks:
    Dr, Vr, full = ref = ec.reference(batch.label, K)
    for b, n in enumerate(batch.ns):
      if n:
        assert not oracle.degenerate_cut(full[b] / max(np.abs(full[b]).max(), 1e-300), K), (batch.names[b], K)
    fig = rc.check_bars(batch.A, batch.ns, K, Dr, Vr, ref, batch.names)
    assert (fig <= QUARTER).all(), (batch.label, K, fig.tolist())
    worst = np.maximum(worst, fig)
  return worst


def test_the_seam_batches_hold_the_sizes_and_the_k_of_every_seam():
  assert ec.SEAM_N == (1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 193)
  assert ec.seam_sizes(1) == [1, 0] and ec.seam_sizes(2) == [2, 1, 0] and ec.seam_sizes(3) == [3, 2, 1, 0]
  assert ec.seam_sizes(129) == [129, 128, 3, 2, 1, 0]
  assert ec.seam_K(1) == (1, 15, 16, 17) and ec.seam_K(3) == (1, 3, 15, 16, 17, 256)
  assert ec.seam_K(64) == (1, 15, 16, 17, 64) and ec.seam_K(193) == (1, 15, 16, 17, 64, 256)
  pairs = {(int(n), K) for b in ec.seam_batches() for n in b.ns for K in b.Ks}
  # n = 2K - 1, 2K, 2K + 1: whether the K smallest and the K largest candidates overlap
  assert {(31, 16), (32, 16), (33, 16), (127, 64), (128, 64), (129, 64), (1, 1), (2, 1), (3, 1)} <= pairs
  for b in ec.seam_batches():
    N = b.A.shape[1]
    assert list(b.ns[:len(ec.seam_sizes(N))]) == ec.seam_sizes(N)
    assert len(b.ns) == len(ec.seam_sizes(N)) + (2 if N >= 31 else 0)
    for a, n in zip(b.A, b.ns):
      assert np.array_equal(a, a.T) and not a[n:].any() and not a[:, n:].any()
    if N >= 31:
      d, t = b.A[-2], b.A[-1]
      assert b.ns[-2] == b.ns[-1] == N
      assert not (d - np.diag(np.diag(d))).any()
      assert not np.tril(t, -2).any() and np.diag(t, -1).all()


@pytest.mark.parametrize('N', ec.SEAM_N)
def test_no_seam_cut_is_degenerate_and_the_rounded_reference_meets_a_quarter_of_the_bars(N):
  batch = [b for b in ec.seam_batches() if b.label == 'seam%d' % N][0]
  print(batch.label, _rounded_reference_meets_a_quarter(batch))


@pytest.mark.parametrize('label', [b.label for b in ec.spectra_batches() + ec.scaled_batches()])
def test_no_spectra_cut_is_degenerate_and_the_rounded_reference_meets_a_quarter_of_the_bars(label):
  batch = [b for b in ec.spectra_batches() + ec.scaled_batches() if b.label == label][0]
  print(batch.label, _rounded_reference_meets_a_quarter(batch))


def test_wilkinson_and_paired_cuts_are_clean_at_even_k_only():
  """Why the GPU module pairs these families with even K: every odd K cuts a pair."""
  for cases in (rc.wilkinson(16), rc.wilkinson(32), rc.wilkinson(48), rc.paired(65), rc.paired(129)):
    A, ns = rc.pad_batch(cases)
    full = rc.eigh_ref(A, ns, 1)[2]
    for b, (name, _) in enumerate(cases):
      lam = full[b] / np.abs(full[b]).max()
      assert not any(oracle.degenerate_cut(lam, K) for K in (16, 32, 64, 96)), name
    assert any(oracle.degenerate_cut(full[b] / np.abs(full[b]).max(), 15) for b in range(len(cases)))


def test_scaled_batches_are_exact_multiples_inside_float32_range():
  for w, base in enumerate(ec.scale_free_bases()):
    assert (base.ns == base.A.shape[1]).all()
    for s in ec.SCALES:
      sb = ec.scaled_batch(w, s)
      assert np.array_equal(sb.A.astype(np.float64), base.A.astype(np.float64) * s)
      live = np.abs(sb.A[sb.A != 0])
      assert np.isfinite(sb.A).all() and live.min() > 2.0 ** -120      # no float32 subnormal
      for K in sb.Ks:   # the reference eigenvalues scale into normal float32 numbers too
        Dr = ec.reference(sb.label, K)[0]
        assert (np.abs(Dr[Dr != 0]) > 2.0 ** -120).all()


def test_clustered_matrices_have_their_multiplicities_and_the_rounded_reference_passes():
  cases = ec.clustered()
  assert [m.shape[0] for _, m in cases] == [40, 70, 100, 129]
  mult = {}
  for name, M in cases:
    e = np.linalg.eigh(M.astype(np.float64))[0]
    s = max(np.abs(e).max(), 1e-300)
    groups = np.split(e, np.where(np.diff(e) > 1e-9 * s)[0] + 1)
    mult[name] = sorted({len(g) for g in groups})
  assert mult == {'zero40': [40], '0.75I_70': [70], 'diag20x5': [5], '3xsym43': [3]}
  blocks = cases[3][1]
  assert np.array_equal(blocks[:43, :43], blocks[43:86, 43:86]) and not blocks[:43, 43:].any()
  A, ns = rc.pad_batch(cases)
  names = [c[0] for c in cases]
  for K in ec.CLUSTER_K:
    Dr, Vr, _ = rc.eigh_ref(A, ns, K)
    fig = ec.check_clusters(A, ns, K, Dr, Vr, np.zeros(len(ns), np.int32), names, say=print)
    assert (fig <= 0.25 * np.array([rc.TOL_D, rc.TOL_ORTH, rc.TOL_RES, ec.TOL_INSIDE, rc.TOL_PROJ])).all(), fig


def test_check_clusters_rejects_a_vector_that_leaves_its_eigenspace():
  """The checker has teeth: a vector of the triple eigenvalue rotated by 1e-4 towards a
  neighbouring eigenspace, or two vectors of a cluster that are not orthogonal, fail it."""
  cases = ec.clustered()[3:]
  A, ns = rc.pad_batch(cases)
  Dr, Vr, _ = rc.eigh_ref(A, ns, 16)
  ok = np.zeros(1, np.int32)
  ec.check_clusters(A, ns, 16, Dr, Vr, ok)
  e, U = np.linalg.eigh(A[0].astype(np.float64))
  far = U[:, np.argmin(np.abs(e))]                # an eigenvector outside the top 16
  bad = Vr.copy()
  bad[0, :, 0] = (bad[0, :, 0] + 1e-4 * far).astype(np.float32)
  with pytest.raises(AssertionError):
    ec.check_clusters(A, ns, 16, Dr, bad, ok)
  bad = Vr.copy()
  bad[0, :, 1] = (bad[0, :, 1] + 1e-4 * bad[0, :, 0]).astype(np.float32)
  with pytest.raises(AssertionError):
    ec.check_clusters(A, ns, 16, Dr, bad, ok)
  with pytest.raises(AssertionError):
    ec.check_clusters(A, ns, 16, Dr, Vr, np.array([2], np.int32))
