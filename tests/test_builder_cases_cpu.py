"""CPU checks of the cases of test_gpu_laplacian_edges.py, test_gpu_collate_edges.py and the new rows of
test_segment_sum_reference.py / test_gpu_mlp_grad.py (builder_cases.py), so that a failure on the GPU is never
the fault of the inputs: every row takes the route its table claims under a plain restatement of its
launcher's rule, the drawn graphs hold the contents they are meant to hold, and a numpy emulation of the
kernels' arithmetic — fp64 sequential row sum, s = deg^-x, (s_i m) s_j, one rounding to float32 — meets the
bar against oracle.get_laplacian on every Laplacian case, so the bar is shown reachable before a GPU is
involved."""
import numpy as np
import pytest

import oracle
import builder_cases as bc


def test_every_l4_shape_takes_the_route_its_row_claims():
  for (N, E, route, seam) in bc.L4_SHAPES:
    assert bc.l4_route(N, E) == route, (N, E, seam)
    assert bc.l4_route(N, E, aligned=False) == 'direct'
  float4s = {(N, E): N * N * E // 4 for (N, E, route, _) in bc.L4_SHAPES if route == 'staged'}
  assert float4s == {(4, 1): 4, (5, 4): 25, (26, 6): 1014, (27, 4): 729, (48, 4): 2304, (100, 1): 2500,
                     (126, 1): 3969}
  assert float4s[(48, 4)] > 8 * 256 and float4s[(4, 1)] < 256     # a second outer turn / lanes that clamp
  assert (5 * 5) % 2 == 1 and bc.l4_staged_bytes(5, 4) == 26 * 8 + 400   # the rounded stage offset
  assert bc.l4_staged_bytes(126, 1) == 65520
  # the three conditions, each alone: bytes, N N E % 4, alignment
  assert bc.l4_staged_bytes(128, 1) > bc.LDS_MAX and (128 * 128) % 4 == 0
  assert bc.l4_staged_bytes(64, 4) > bc.LDS_MAX and bc.l4_staged_bytes(62, 4) <= bc.LDS_MAX
  assert (127 * 127) % 4 == 1
  assert (3 * 3 * 2) % 4 == 2 and (5 * 5) % 4 == 1
  for (N, E) in bc.UNALIGNED_SHAPES:
    assert bc.l4_route(N, E) == 'staged' and bc.l4_route(N, E, aligned=False) == 'direct'
  N, E = bc.REFUSED_SHAPE
  assert bc.l4_route(N, E) == 'refused' and (E + 1) * N == 8200 and bc.l4_route(1024, 7) != 'refused'
  assert [bc.l4_route(N, E) for (N, E) in bc.KIND_SHAPES] == ['staged', 'direct']
  assert max(N for (N, _, _, _) in bc.L4_SHAPES) == 128


def test_every_batch_holds_the_counts_and_the_contents_it_is_meant_to():
  for bt, _ in bc.l4_batches():
    N, E = bt.N, bt.E
    assert bt.counts.tolist()[:3] == [0, 1, N] and bt.counts.tolist()[4:] == [N + 3, -2]
    assert 1 <= bt.counts[3] < N or N <= 2
    assert np.array_equal(bt.adjs[4], bt.adjs[2])
    for b, c in enumerate(bt.counts):
      n = bc.clamp(c, N)
      A = bt.adjs[b].astype(np.float64)
      if b < 4:
        assert not A[n:].any() and not A[:, n:].any()
    full, mid = bt.adjs[2].astype(np.float64), bt.adjs[3].astype(np.float64)
    if bt.content == 'bonds':
      assert np.array_equal(full, full.transpose(1, 0, 2)) and (full == 2).any()
      assert set(np.unique(full)) <= {0.0, 1.0, 2.0} and not np.einsum('iie->ie', full).any()
      assert not full[N - 1].any()                                   # an atom with no bond at all
      assert not bt.adjs[1].any()                                    # n = 1: every bond type absent
      if E > 1:
        assert not full[:, :, E - 1].any() and full[:, :, 0].any()   # a bond type absent from a molecule
    else:
      assert not np.array_equal(full, full.transpose(1, 0, 2))
      for A, n in ((full, N), (mid, int(bt.counts[3]))):
        r = n // 2
        rows = A[:n, :n].sum(axis=(1, 2))
        if bt.content == 'weighted':
          assert (A >= 0).all() and rows[r] == 0 and (np.delete(rows, r) > 0).all()
          assert (np.delete(A[:n, :n].sum(axis=1), r, axis=0) > 0).all()   # ... in every channel
        else:
          want = 0.0 if bt.content == 'zero_sum' else -2.0
          assert 1.0 + rows[r] == want and 1.0 + A[r, :n, 0].sum() == want
          assert not np.delete(A[r, :n], r, axis=0).any() and not A[r, r, 1:].any()
    for fill in ('junk', 'nan'):
      P = bc.with_padding(bt, fill)
      for b, c in enumerate(bt.counts):
        n = bc.clamp(c, N)
        assert np.array_equal(P[b, :n, :n], bt.adjs[b, :n, :n])
        pad = np.ones((N, N), bool)
        pad[:n, :n] = False
        assert (np.isfinite(P[b][pad]).all() and (P[b][pad] != 0).all()) if fill == 'junk' else np.isnan(P[b][pad]).all()


def test_the_reference_states_l1_directly_at_one_node_where_the_oracle_raises():
  with pytest.raises(ValueError):
    oracle.get_laplacian(np.array([[0.5]]), 'L1')
  assert bc._one_laplacian(np.array([[0.5]]), 'L1', 0.5).tolist() == [[0.0]]
  A = np.array([[0.0, 2.0], [1.0, 0.5]])
  assert np.array_equal(bc._one_laplacian(A, 'L1', 0.5), np.diag(A.sum(1)) - A)


@pytest.mark.parametrize('label', [bt.label for bt, _ in bc.l4_batches()])
def test_the_emulated_l4_arithmetic_meets_the_bar(label):
  bt = [b for b, _ in bc.l4_batches() if b.label == label][0]
  ref = bc.reference(bt.N, bt.E, bt.content)
  got = bc.emulate(bt.adjs, bt.counts, l4_entry=True)
  worst, differ = bc.check_bar(got, ref, bt.counts, label, l4_rule=True)
  print('%s: lnz_laplacian_l4 emulated, worst achieved/bar %.3f, %d elements differ from float32(ref)'
        % (label, worst, differ))
  # the clamped count gives the bits of n = N, the negative one those of n = 0
  assert np.array_equal(got[4], got[2]) and not got[5].any() and not got[0].any()
  kind4 = bc.emulate(bt.adjs, bt.counts, 'L4')
  if bt.content == 'negative_sum':
    # the two entry points' rules: NaN in the reference's row and column against zeros
    bc.check_bar(kind4, ref, bt.counts, label)
    assert np.isnan(kind4).any() and not np.isnan(got).any() and np.isnan(ref[2]).any()
    with pytest.raises(AssertionError):
      bc.check_bar(got, ref, bt.counts, label)
  else:
    assert np.array_equal(kind4.view(np.int32), got.view(np.int32))   # 1 / sqrt against pow(d, -0.5): the same bits here
    assert not np.isnan(ref).any()
  if bt.content == 'zero_sum':
    for b in (2, 3):
      r = bc.clamp(bt.counts[b], bt.N) // 2
      assert not got[b, r, :, :2].any() and not got[b, :, r, :2].any() and got[b, r, r, 2] == 1.0


@pytest.mark.parametrize('kind,alpha', bc.KINDS)
def test_the_emulated_arithmetic_of_every_kind_meets_the_bar(kind, alpha):
  for bt in bc.kind_batches():
    ref = bc.reference(bt.N, bt.E, bt.content, kind, alpha)
    got = bc.emulate(bt.adjs, bt.counts, kind, alpha)
    worst, differ = bc.check_bar(got, ref, bt.counts, (bt.label, kind, alpha))
    print('%s %s alpha %.1f emulated: worst achieved/bar %.3f, %d elements differ from float32(ref)'
          % (bt.label, kind, alpha, worst, differ))
    if bt.content == 'weighted':   # the all-zero row: degree 0 under kinds 1-3, 6, 7 (the inf -> 0 guard), 1 under 4, 5
      r = bt.N // 2
      row = ref[2, r, :, 1]
      want = np.zeros(bt.N)
      want[r] = {'L1': 0.0, 'L2': 1.0, 'L3': 1.0, 'L4': 1.0, 'L5': 1.0, 'L6': 0.0, 'L7': 0.0}[kind]
      assert np.array_equal(row, want), (kind, row)


def test_the_bar_has_teeth():
  """One float32 ulp on one element, a row sum taken in float32, a padding entry that is read, a count that
  is not clamped: each misses the bar."""
  bt = bc.batch(27, 4, 'weighted')
  ref = bc.reference(27, 4, 'weighted')
  good = bc.emulate(bt.adjs, bt.counts, l4_entry=True)
  bc.check_bar(good, ref, bt.counts, 'good')
  bad = good.copy()
  bad[2, 3, 4, 0] = np.nextafter(np.nextafter(bad[2, 3, 4, 0], np.float32(2)), np.float32(2))
  with pytest.raises(AssertionError):
    bc.check_bar(bad, ref, bt.counts, 'two ulps')
  deg32 = (1 + bt.adjs[2].sum(axis=2, dtype=np.float32).sum(axis=1, dtype=np.float32)).astype(np.float32)
  s32 = (1 / np.sqrt(deg32)).astype(np.float32)
  bad = good.copy()
  bad[2, :, :, 0] = (s32[:, None] * (np.eye(27, dtype=np.float32) + bt.adjs[2].sum(axis=2, dtype=np.float32))) * s32[None, :]
  with pytest.raises(AssertionError):
    bc.check_bar(bad, ref, bt.counts, 'float32 arithmetic')
  bad = good.copy()
  bad[3, 26, 26, 1] = 1.0
  with pytest.raises(AssertionError):
    bc.check_bar(bad, ref, bt.counts, 'padding written')
  junk = bc.emulate(bc.with_padding(bt, 'junk'), np.full(6, 27), l4_entry=True)   # counts not honoured
  with pytest.raises(AssertionError):
    bc.check_bar(junk, ref, bt.counts, 'padding read')


def test_collate_shapes_sit_on_the_lds_bound_and_the_molecules_hold_their_cases():
  assert [bc.collate_lds_bytes(N, E) for (N, E, _) in bc.COLLATE_SHAPES] == [48, 46320, 65520, 65280]
  assert all(bc.collate_lds_bytes(N, E) <= bc.LDS_MAX for (N, E, _) in bc.COLLATE_SHAPES)
  assert all(bc.collate_lds_bytes(N, E) > bc.LDS_MAX for (N, E) in bc.COLLATE_REFUSED)
  assert all(bc.collate_lds_bytes(N - 1, E) <= bc.LDS_MAX for (N, E) in bc.COLLATE_REFUSED)
  assert sorted(P for (_, _, P) in bc.COLLATE_SHAPES)[0] == 1 and max(P for (_, _, P) in bc.COLLATE_SHAPES) > 256
  for (N, E, P) in bc.COLLATE_SHAPES:
    mols = bc.collate_molecules(N, E, P)
    by = {m.name: m for m in mols}
    ids = bc.collate_ids(len(mols))
    assert (ids < 0).sum() == 2 and (ids >= len(mols)).sum() == 2 and len(set(ids.tolist())) < len(ids)
    feat, mask, label, n_nodes, adjs = bc.collate_expected(mols, ids, N, E)
    assert all(len(m.bonds) == 0 or max(max(u, v, t) for (u, v, t) in m.bonds) < 256 for m in mols)
    k = [m.name for m in mols]
    a = adjs[k.index('no_bonds')]
    assert not a.any() and n_nodes[k.index('no_bonds')] == len(by['no_bonds'].atoms)
    L = bc.collate_reference(adjs, n_nodes)
    n = int(n_nodes[k.index('no_bonds')])
    for ch in range(E + 1):          # no bonds: the identity on n in every channel
      assert np.array_equal(L[k.index('no_bonds'), :, :, ch], np.diag((np.arange(N) < n).astype(np.float64)))
    a = adjs[k.index('twice_self_dropped')]
    assert a[0, 1, 0] == 2 and a[1, 0, 0] == 2 and a[1, 1, E - 1] == 1 and a.sum() == 5   # twice; self once; the rest dropped
    big = by['oversized']
    assert len(big.atoms) == N + 2 and n_nodes[k.index('oversized')] == N
    cut = bc.truncated(big, N)
    assert 0 < len(cut.bonds) < len(big.bonds) and len(cut.atoms) == N
    assert np.array_equal(adjs[k.index('oversized')], oracle.dense_from_edges(N, bc.pack_bonds(cut.bonds), E))
    outside = [b for b, i in enumerate(ids) if not 0 <= i < len(mols)]
    assert len(outside) == 4 and not n_nodes[outside].any() and not label[outside].any() and not mask[outside].any()
    rep = [b for b, i in enumerate(ids) if i == 1]
    assert len(rep) == 2 and np.array_equal(adjs[rep[0]], adjs[rep[1]])
    if N == 126:
      assert len(by['many_bonds'].bonds) > 256
    assert np.isfinite(L).all()


def test_every_segment_sum_row_takes_the_route_its_row_claims():
  r = {}
  for i, (B, D1, D2, S, aligned, kernel, why) in enumerate(bc.SEGSUM_FORWARD):
    r[i] = bc.segsum_forward_route(B, D1, D2, S, aligned)
    assert r[i]['kernel'] == kernel, (i, r[i], why)
    assert B * D1 * D2 <= 8 * 300 * 220
  assert [r[i]['lds'] for i in (0, 3, 5)] == [65536] * 3                       # a dynamic LDS size of exactly 64 KiB
  assert r[1]['rows_per_wave'] == 50 and 50 % 4 == 2                            # a ragged last group of the pipeline
  assert r[2]['rows_per_wave'] == 17 and 65 - 3 * 17 == 14                      # the last wave's short range
  assert r[3]['blocks'] == 1 and r[3]['last_width'] == 132
  assert r[4]['blocks'] == 2 and r[4]['last_width'] == 4
  assert r[6]['turns'] == 1 and r[7]['turns'] == 2 and 8 * 300 * 220 == 528000 > 2048 * 256
  assert bc.SEGSUM_FORWARD[8][:4] == bc.SEGSUM_FORWARD[3][:4] and r[8]['vec'] == 1 and r[3]['vec'] == 4
  for i, (B, D1, D2, S, kernel, why) in enumerate(bc.SEGSUM_BACKWARD):
    r[i] = bc.segsum_backward_route(B, D1, D2, S)
    assert r[i]['kernel'] == kernel, (i, r[i], why)
  assert r[0]['rows'] == 19200 > r[0]['waves'] == 16384 and r[1]['rows'] <= r[1]['waves']


def test_the_segment_sum_rule_equals_the_oracle_in_range_and_drops_the_rest():
  B, D1, D2, S = bc.SEGSUM_FORWARD[bc.SEGSUM_FORWARD_OUT_OF_RANGE][:4]
  data, ids = bc.segsum_inputs(B, D1, D2, S, seed=3)
  assert np.array_equal(data, np.round(data)) and np.abs(data).max() == 8 and ids.min() == 0 and ids.max() == S - 1
  want = bc.segsum_forward_rule(data, ids, S)
  assert np.array_equal(want, oracle.unsorted_segment_sum_forward_gpu_semantics(data, ids, S))
  assert np.abs(want).max() < 2 ** 24                                          # exact in float32 in any order
  gout = np.random.RandomState(4).randint(-8, 9, size=(B, S, D2)).astype(np.float32)
  assert np.array_equal(bc.segsum_backward_rule(gout, ids),
                        oracle.unsorted_segment_sum_backward_gpu_semantics(gout, ids, D1))
  data, bad = bc.segsum_inputs(B, D1, D2, S, seed=3, out_of_range=True)
  out = (bad < 0) | (bad >= S)
  assert out.sum() == 6 * B and {-1, S, 2 ** 31} <= set(bad[out].tolist())
  dropped = np.where(out[:, :, None], np.float32(0), data)
  keep = np.where(out, 0, bad)
  assert np.array_equal(bc.segsum_forward_rule(data, bad, S), bc.segsum_forward_rule(dropped, keep, S))
  back = bc.segsum_backward_rule(gout, bad)
  assert not back[out].any() and np.array_equal(back[~out], bc.segsum_backward_rule(gout, keep)[~out])


def test_the_embedding_rows_are_the_two_the_kernel_has_not_run():
  (B, N, width, atoms, chunks), (B2, N2, width2, atoms2, chunks2) = sorted(bc.EMBEDDING_EXACT, reverse=True)
  assert (B * N) % 64 == 0 and B * N // chunks >= 64 and width == 64      # every 64-row step: 64 hits = 8 turns of 8
  assert chunks2 > B2 * N2 and width2 == 128
