"""The planted inputs of tests/test_gpu_large_edges.py hold what its exact cases rest on — checked
here in float64, on a machine without a GPU."""
import numpy as np

import large_edges_fixture as fx


def test_exact_cases_stay_integers_below_two_to_the_24():
  """Every exact case: integer operands that one bf16 / fp16 piece holds, and the sum of the
  absolute products of every dot product (x 2^10 where the two-plane mode scales its A operands)
  below 2^24 — so no partial sum, in any order, with or without atomics, is ever rounded."""
  worst = fx.all_exact_cases()
  print('largest partial-sum bound: %.0f of %.0f' % (worst, fx.EXACT_LIMIT))
  assert 0 < worst < fx.EXACT_LIMIT


def test_the_shapes_reach_the_seams_they_are_there_for():
  totals = [fx.conv_total(C, N) for C, N, _, _ in fx.CONV_SHAPES]
  assert totals == [1, 3, 7, 11, 10, 6, 17, 25, 4]
  assert {t % 4 for t in totals} == {0, 1, 2, 3} and {1, 3} <= set(totals)
  assert max(C for C, _, _, _ in fx.CONV_SHAPES) == 8
  assert all(B == 10 for C, _, B, _ in fx.CONV_SHAPES if C >= 1)
  # the k rotation kb0 = (7 b + (b >> 3)) % nkb takes every residue over b < 10 for nkb = 3 and 5
  for nkb in (3, 5):
    assert {(7 * b + (b >> 3)) % nkb for b in range(10)} == set(range(nkb))
  # both `rows` regimes of the projection, a ragged last chunk, and the two switch settings
  assert fx.project_rows(256, 140) == (192, 1) and fx.project_rows(128, 300) == (192, 2)
  assert all(fx.project_rows(B, N) == (128, (N + 127) // 128) for B, N, *_ in fx.SPECTRAL_SHAPES)
  assert fx.project_rows(3, 300, 1) == (320, 1) and fx.project_rows(3, 300, 4096) == (128, 3)


def test_gather_plan_holds_every_row_length_in_every_graph():
  for cap in (128, 32):
    plan = fx.gather_row_plan(cap)
    assert plan.shape == (fx.GATHER_B, fx.GATHER_N) and plan.max() == cap
    case = fx.gather_case(cap, False)
    assert np.array_equal((case['L'] != 0).sum(axis=2), plan)
  assert fx.GATHER_N % 32 == 5   # the last tile: one wave with five rows


def test_channel_gather_case_rotates_the_plan_and_stays_within_the_row_capacity():
  """(the case asserts its own preconditions) no row of any channel beyond cap: the images of
  test_channel_gathers_equal_chained_one_operator_gathers raise no flag because of their INPUTS"""
  for cap in (128, 32):
    for R in (2, 3, 8):
      case = fx.gather_channels_case(cap, R)
      assert case['L'].shape == (fx.GATHER_B, fx.GATHER_N, fx.GATHER_N, R) and case['plan'].max() == cap
      assert np.array_equal(case['plan'][1, 0], fx.gather_row_plan(cap)[1])
  assert fx.GATHER_B > 8   # the second dealing round


def test_bf16_round_is_round_to_nearest_even():
  x = np.array([1.0, 1.00390625, 1.01171875, 257.0, 259.0, -3.0, 0.0], np.float32)   # ties at 1 + 2^-8 k
  np.testing.assert_array_equal(fx.bf16_round(x), [1.0, 1.0, 1.015625, 256.0, 260.0, -3.0, 0.0])
  assert fx.is_bf16(np.array([64.0, -2.0, 0.5])) and not fx.is_bf16(np.array([257.0]))
