"""CPU checks of the inputs of tests/kstep_cases.py against the float64 restatement of the K-step
Lanczos kernels (oracle.lanczos_kstep_fp64): with the kernels' rules (the carried bound of
lnz::CgsBound, the stop relative to the matrix' scale) the restatement, rounded to float32, meets every
bar the GPU test (test_gpu_kstep_edges.py) holds the kernels to, with a quarter of it; with the rules
the kernels had before (rule='fraction', scale='absolute') it fails them — on L1, L2 and evenly spread
spectra, and on matrices times 2^-30 — which is what gives the GPU test its teeth."""
import numpy as np
import pytest

import kstep_cases as kc
import oracle
import ritz_cases as rc

QUARTER = 0.25


def _restate_batch(A, ns, M, K, **kw):
  """The restatement on every graph of a padded batch, rounded to float32 like a kernel's output.
  -> D [B, K], V [B, N, K], steps [B]"""
  B, N = A.shape[0], A.shape[1]
  D = np.zeros((B, K), np.float32)
  V = np.zeros((B, N, K), np.float32)
  steps = np.zeros(B, np.int64)
  for b in range(B):
    n = int(ns[b])
    d, v, (_, _, steps[b], _) = oracle.lanczos_kstep_fp64(A[b, :n, :n], M, K, **kw)
    D[b], V[b, :n] = d, v
  return D, V, steps


@pytest.mark.parametrize('which', [0, 1])
def test_full_krylov_space_meets_the_bars_against_eigh(which):
  tag, A, ns, names, ks = kc.full_batches()[which]
  worst = np.zeros(4)
  for b, name in enumerate(names):   # every listed case: a simple spectrum, nothing skipped
    if ns[b] > 1:      # (beyond the 1e-7 the float32 matrix resolves; `graded` alone is below 1e-4)
      assert kc.min_relative_gap(A[b, :ns[b], :ns[b]]) > (oracle.CUT_GAP if name.startswith('graded') else 1e-4), name
  for K in ks:
    D, V, steps = _restate_batch(A, ns, kc.N_FULL, K)
    assert (steps == ns).all(), (tag, steps.tolist())          # a graph of n nodes stops after n steps
    worst = np.maximum(worst, rc.check_bars(A, ns, K, D, V, rc.eigh_ref(A, ns, K), names))
  print('%s: |D-Dref| %.2e  |VtV-I| %.2e  |AV-VD| %.2e  projector %.2e' % ((tag,) + tuple(worst)))
  assert (worst < QUARTER * np.array([rc.TOL_D, rc.TOL_ORTH, rc.TOL_RES, rc.TOL_PROJ])).all(), worst


def test_multiplicities_each_distinct_eigenvalue_once():
  A, ns, names = kc.multiplicity_batch()
  D, V, steps = _restate_batch(A, ns, 24, 24)
  want = {'zero24': 1, '0.75I_24': 1, '3x_spread8': 8, 'ring24_adj': 13, 'star17_adj': 3}
  for b, name in enumerate(names):
    n = int(ns[b])
    fig = kc.check_distinct(name, A[b, :n, :n], D[b], V[b], steps[b], 24)
    assert name not in want or steps[b] == want[name], (name, steps[b])
    assert fig[0] < QUARTER * rc.TOL_D and fig[1] < QUARTER * rc.TOL_ORTH and fig[2] < QUARTER * rc.TOL_RES, (name, fig)


def _orth(V, kk):
  return float(np.abs(V[:, :kk].T @ V[:, :kk] - np.eye(kk)).max())


def test_kstep_proper_inputs_are_well_posed():
  """(c): the restatement keeps its basis orthonormal to a quarter of the GPU bar on every input, takes
  all M steps where M < n, and no cut of the top K falls into a pair of Ritz values closer than 1e-5
  (the projector of K Ritz vectors would not be defined)."""
  for N in kc.SEAM_N:
    G = kc.seam_graphs(N)
    assert np.isfinite(G).all()
    for M, K in kc.seam_shapes(N):
      for g in range(G.shape[0]):
        _, V, (_, _, steps, _) = oracle.lanczos_kstep_fp64(G[g], M, K)
        assert steps == M and _orth(V, K) < QUARTER * kc.TOL_ORTH, (N, M, K, g)
        assert kc.cut_gap(G[g], M, K) > 1e-5, (N, M, K, g)
  for name, A in kc.operator_cases():
    for M in kc.OPERATOR_M:
      _, V, (_, _, steps, _) = oracle.lanczos_kstep_fp64(A, M, M)
      assert steps == M and _orth(V, M) < QUARTER * kc.TOL_ORTH, (name, M)
  A, ns, names = kc.ragged_batch()
  assert np.isfinite(A).all() and ns.tolist() == list(kc.RAGGED_SIZES)
  _, V, steps = _restate_batch(A, ns, 64, 64)
  assert steps.tolist() == [min(64, n) for n in kc.RAGGED_SIZES]
  A, ns, longest = kc.row_cap_batch()
  assert longest == [kc.ROW_CAP, kc.ROW_CAP + 1]
  _, V, steps = _restate_batch(A, ns, 16, 16)
  assert (steps == 16).all()


def test_the_fraction_rule_fails_L1_L2_and_spread():
  """What the kernels did before lnz::CgsBound: a second pass only beyond 1 - 1e-6 of |w|^2.  The
  basis is lost altogether on L1, L2 and the evenly spread spectrum, and kept on L4."""
  lost = {}
  for name, A in kc.operator_cases():
    for M in kc.OPERATOR_M:
      _, V, _ = oracle.lanczos_kstep_fp64(A, M, M, rule='fraction')
      lost[(name, M)] = _orth(V, M)
  print({k: '%.1e' % v for k, v in lost.items()})
  for name in ('gnp256_L2', 'gnp256_L1', 'gnp128_L2', 'gnp128_L1'):
    assert lost[(name, 64)] > 1.0, name                  # not a basis any more
  assert lost[('gnp128_L2', 32)] > kc.TOL_ORTH
  tag, A, ns, names, _ = kc.full_batches()[0]
  D, V, steps = _restate_batch(A, ns, kc.N_FULL, kc.N_FULL, rule='fraction')
  failed = []
  for b, name in enumerate(names):
    try:
      rc.check_bars(A[b:b + 1], ns[b:b + 1], kc.N_FULL, D[b:b + 1], V[b:b + 1],
                    rc.eigh_ref(A[b:b + 1], ns[b:b + 1], kc.N_FULL), [name])
    except AssertionError:
      failed.append(name)
  print('fraction rule fails:', failed)
  for name in ('spread63_rot', 'spread64_rot', 'spread64_diag', 'gnp32_L1', 'gnp32_L2', 'gnp64_L1', 'gnp64_L2',
               'gnp60_L1', 'gnp60_L2'):
    assert name in failed, name
  assert not [f for f in failed if f.startswith(('sym', 'gnp64_L4', 'gnp60_L4', 'gnp64_adj'))], failed


@pytest.mark.parametrize('s', kc.BIG_SCALES)
def test_power_of_two_scaling_changes_nothing_but_the_scale(s):
  for tag, A, ns in kc.scale_base():
    M = A.shape[1] if tag == 'full64' else 24
    D0, V0, steps0 = _restate_batch(A, ns, M, M)
    As = (A * np.float32(s)).astype(np.float32)
    assert (As.astype(np.float64) == A.astype(np.float64) * s).all()      # an exact multiple in float32
    D1, V1, steps1 = _restate_batch(As, ns, M, M)
    assert (steps1 == steps0).all(), (tag, s, steps0.tolist(), steps1.tolist())
    assert np.array_equal(V1, V0) and np.array_equal(D1, D0 * np.float32(s)), (tag, s)
    if tag != 'full64':
      assert steps0.tolist() == [8]


def test_the_absolute_stop_fails_small_scales():
  """`nrm <= 1e-8` as an absolute number: times 2^-30 and 2^-60 every matrix 'stops' after one step
  (one Ritz value, the rest zeros); times 2^30 the three copies of one block run past their 8
  distinct eigenvalues."""
  for tag, A, ns in kc.scale_base():
    M = A.shape[1] if tag == 'full64' else 24
    _, _, steps0 = _restate_batch(A, ns, M, M)
    for s in (2.0 ** -60, 2.0 ** -30):
      As = (A * np.float32(s)).astype(np.float32)
      _, _, steps = _restate_batch(As, ns, M, M, scale='absolute')
      assert (steps == 1).all() and (steps0 > 1).all(), (tag, s, steps.tolist())
  A = kc.three_copies() * np.float32(2.0 ** 30)
  _, _, (_, _, steps, _) = oracle.lanczos_kstep_fp64(A, 24, 24, scale='absolute')
  assert steps > 8, steps
