"""CPU checks of the input families of ritz_cases.py on the one-wavefront kernel's mirror
(algo_mirror.lanczos_ritz_mirror, n <= 32): every family meets the bars the GPU tests hold the
kernels to (test_gpu_ritz_edges.py), the Wilkinson matrices really reach the QL fallback, and the
99 % rule for the second Gram-Schmidt pass — the kernels' rule until these spectra — misses the
orthogonality bar on spread(32)."""
import numpy as np
import pytest

import oracle
import ritz_cases as rc
from algo_mirror import lanczos_ritz_mirror, matrix_scale


def _mirror(cases, K, N=None, **kw):
  """The mirror on every case, collated like the kernel's outputs.  -> A, ns, D, V, info"""
  A, ns = rc.pad_batch(cases, N)
  D = np.zeros((len(cases), K), np.float32)
  V = np.zeros((len(cases), A.shape[1], K), np.float32)
  info = np.zeros(len(cases), np.int64)
  for b, (_, M) in enumerate(cases):
    if ns[b]:
      D[b], V[b, :ns[b]], info[b] = lanczos_ritz_mirror(M, K, **kw)
  return A, ns, D, V, info


def _molecules():
  from lanczosnet_amd.synthetic import draw_batch
  b = draw_batch(8, seed=3, n_min=4, n_max=26)
  return [('mol%d' % i, oracle.laplacian_l4(b['adjs'][i, :n, :n].sum(axis=2)).astype(np.float32))
          for i, n in enumerate(int(x) for x in b['n_nodes'])]


FAMILIES = {
    'spread': lambda: [c for n in (24, 31, 32) for c in rc.spread(n)],
    'graded': lambda: [c for n in (24, 31, 32) for c in rc.graded(n)],
    'paired': lambda: [c for n in (24, 31, 32) for c in rc.paired(n)],
    'non_l4': rc.non_l4_operators,
    'wilkinson': rc.wilkinson_family,
    'scaled_molecules': lambda: [c for s in rc.SCALES for c in rc.scaled(_molecules(), s)],
    'scaled_spread': lambda: [c for s in rc.SCALES for c in rc.scaled(rc.spread(32), s)],
}


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_mirror_meets_the_bars_on_every_family(family):
  cases = FAMILIES[family]()
  A, ns, D, V, info = _mirror(cases, 32, 32)
  rc.check_bars(A, ns, 32, D, V, rc.eigh_ref(A, ns, 32), [c[0] for c in cases])


def test_mirror_meets_the_bars_at_every_tile_size_and_no_cut_is_degenerate():
  """The shape batches of the GPU test: no top-K cut of any (N, K) falls into a cluster (so nothing
  there is skipped), and the mirror meets the bars on each batch at its smallest K."""
  done = set()
  for N, K in rc.SHAPES:
    A, ns, names = rc.shape_batch(N)
    ref = rc.eigh_ref(A, ns, K)
    for b, n in enumerate(ns):
      if n:
        assert not oracle.degenerate_cut(ref[2][b] / np.abs(ref[2][b]).max(), K), (N, K, names[b])
    if N not in done:
      done.add(N)
      cases = [(nm, A[b, :n, :n]) for b, (nm, n) in enumerate(zip(names, ns))]
      _, _, D, V, _ = _mirror(cases, K, N)
      rc.check_bars(A, ns, K, D, V, ref, names)
  assert done == {1, 2, 15, 16, 17, 31, 32}


def test_wilkinson_matrices_reach_the_ql_fallback_in_the_mirror():
  """W+_{2m+1}, m = 8..10 and 12..14, plain, / 16, - 3 I and negated: the twist windows cannot
  separate the pairs of largest eigenvalues and the mirror takes the QL sweep (info >= 256) — the
  inputs that make the GPU test of the kernel's fallback meaningful."""
  for m in rc.WILKINSON_M:
    for name, W in rc.wilkinson(m, forms=rc.WILKINSON_FORMS[:4]):
      _, _, info = lanczos_ritz_mirror(W, W.shape[0])
      assert info >= 256, name


def test_the_99_percent_rule_alone_misses_the_orthogonality_bar_on_spread32():
  """Why the rule changed: with the second pass only where the first removed more than 99 % of
  |x|^2, the loss of orthogonality grows by |c| / |x'| ~ 2.2 per step on an evenly spread spectrum
  and passes the suite's 2e-6 at n = 32 (4.2e-6 on the diagonal member); the bound that the kernels
  carry now (lnz::CgsBound) takes the second pass every sixth step and stays at rounding level."""
  name, A = rc.spread(32)[1]
  n = A.shape[0]
  worst = {}
  for rule in ('fraction', 'bound', 'always'):
    stats = {}
    D, V, _ = lanczos_ritz_mirror(A, n, cgs_rule=rule, stats=stats)
    Vd = V.astype(np.float64)
    worst[rule] = (float(np.abs(Vd.T @ Vd - np.eye(n)).max()), stats['second_passes'])
  print(worst)
  assert worst['fraction'][0] > rc.TOL_ORTH
  assert worst['bound'][0] < 1e-7 and worst['always'][0] < 1e-7
  assert worst['fraction'][1] <= 2 and worst['bound'][1] < n // 2 and worst['always'][1] == n


def test_the_bound_leaves_molecules_on_the_single_pass():
  """On L4 Laplacians of molecules the bound adds second passes only at restarts (a restart vector
  always takes both): the steps of a molecule stay on the single pass."""
  from lanczosnet_amd.synthetic import draw_batch
  b = draw_batch(48, seed=1)
  extra = steps = restarts = 0
  for i in range(48):
    n = int(b['n_nodes'][i])
    A = oracle.laplacian_l4(b['adjs'][i, :n, :n].sum(axis=2)).astype(np.float32)
    old, new = {}, {}
    _, _, r = lanczos_ritz_mirror(A, 20, solver='ql', cgs_rule='fraction', stats=old)
    lanczos_ritz_mirror(A, 20, solver='ql', cgs_rule='bound', stats=new)
    extra += new['second_passes'] - old['second_passes']
    restarts += r
    steps += n
    assert new['bound'] <= 1.001e-9
  assert extra - restarts <= steps // 100, (extra, restarts, steps)


def test_breakdown_tolerance_follows_the_matrix_scale():
  assert matrix_scale(np.zeros((3, 3))) == 0.0
  for amax, want in ((1.0, 1.0), (0.75, 1.0), (0.5, 0.5), (0.50001, 1.0), (3.0, 4.0), (2.0 ** -20, 2.0 ** -20)):
    assert matrix_scale(np.array([[amax, 0.0], [0.0, -0.1 * amax]])) == want
  # a molecule times 2^-20 restarts at the same steps and returns the same vectors
  name, A = _molecules()[0]
  D1, V1, i1 = lanczos_ritz_mirror(A, 20)
  D2, V2, i2 = lanczos_ritz_mirror(A * np.float32(2.0 ** -20), 20)
  assert i1 == i2 and np.array_equal(V1, V2) and np.array_equal(D1 * np.float32(2.0 ** -20), D2)
