"""The instruction model of the strip forward's folded form of the rare bond-type channels
(utils/flop_model.py: strip_rare_mfma_issued, rare_cost, touch_masks, strip_touch_counts) against hand
counts, against the channel loop's model where nothing is folded, and against the recorded counter run
profiles/r07_strip_rare_pmc.json (rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_F32 alone, of the bench
command on an MI355X; the plan of that run is profiles/r06_strip_plan.npz)."""
import json
import os

import numpy as np

import oracle
from lanczosnet_amd.utils import flop_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QM8_CFG = dict(num_atom=70, num_bond_type=6, short_diffusion_dist=[],
               long_diffusion_dist=[1, 2, 3, 5, 7, 10, 20, 30], num_eig_vec=20,
               spectral_filter_kind='MLP', input_dim=64, hidden_dim=[128] * 7, output_dim=16,
               num_layer=7)


def _strip(S):
  return dict(sub=S, blk=[min(3, S)] * S, ident=[0] * S, rows_real=16 * S, mols=1)


def _hand_count(S, nv):
  """7 layers, 8 long + 7 edge channels, 64 -> 128, by hand: per wave and layer the long channels and
  edge types 0, 1 (10 GEMM1), the folded GEMM1, per virtual subtile a 16-row GEMM1 and 4 S scatter
  instructions, GEMM2 of two edge types, lift-back, projection (not in the last layer); then the
  first projection (4 waves) and the head (S waves)."""
  blocks = 3 * S - 2
  tot = 0
  for l in range(7):
    steps = 4 if l == 0 else 8                  # 16-k steps of the layer's input width
    per_wave = 11 * steps * 4 * S + nv * (steps * 4 + 4 * S) + 4 * 2 * blocks + 4 * blocks
    if l < 6:
      per_wave += 4 * blocks
    tot += 8 * per_wave
  return tot + 4 * 4 * blocks + 64 * S


def test_folded_form_against_hand_counts():
  for S in range(1, 6):
    for nv in range(0, 7):
      counts = [16] * nv + [0] * (5 - nv) if nv <= 5 else [32, 16, 16, 16, 16]
      folded, plain, got_nv = fm.rare_cost(S, counts, 5)
      assert got_nv == nv and folded == 32 * S + nv * (32 + 4 * S) and plain == 5 * (32 * S + 4 * (3 * S - 2))
      r = fm.strip_rare_mfma_issued([_strip(S)], [counts], QM8_CFG)
      old = fm.strip_mfma_issued([_strip(S)], QM8_CFG)
      if folded < plain:
        assert r['rare_strips'] == 1 and r['mfma_issued'] == _hand_count(S, nv), (S, nv)
        assert r['mfma_issued'] < old['mfma_issued']
      else:   # (S = 1 with five or six virtual subtiles: the channel loop is cheaper and is kept)
        assert S == 1 and nv >= 5 and r['rare_strips'] == 0 and r['mfma_issued'] == old['mfma_issued']
      assert r['mfma_channel_loop'] == old['mfma_issued']


def test_nothing_folded_is_the_channel_loop():
  strips = [_strip(S) for S in range(1, 7)]
  old = fm.strip_mfma_issued(strips, QM8_CFG)
  assert fm.strip_rare_mfma_issued(strips, None, QM8_CFG)['mfma_issued'] == old['mfma_issued']
  # six subtiles, more virtual subtiles than the kernel stages, every row of every channel touched
  assert not fm.strip_takes_rare(6, [0] * 5, 5)
  assert not fm.strip_takes_rare(5, [16 * 9, 0, 0, 0, 0], 5)
  assert not fm.strip_takes_rare(5, [80] * 5, 5) and fm.strip_takes_rare(5, [0] * 5, 5)
  full = [[16 * t['sub']] * 5 for t in strips]
  assert fm.strip_rare_mfma_issued(strips, full, QM8_CFG)['mfma_issued'] == old['mfma_issued']


def test_touch_masks_follow_the_row_or_column_rule():
  L = np.zeros((2, 6, 6, 3), np.float32)
  mask = np.array([[1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 1, 0]], np.uint8)
  for c in range(3):
    L[0, :4, :4, c] = np.eye(4)
    L[1, :5, :5, c] = np.eye(5)
  L[0, 1, 2, 1] = L[0, 2, 1, 1] = 0.5      # a bond: both atoms
  L[0, 0, 3, 2] = 0.25                     # one element: its row AND its column
  L[1, 2, 2, 1] = 0.5                      # a diagonal that is not one, on a real node
  L[1, 3, 3, 2] = 0.0                      # a masked node whose diagonal is 0: nothing to fold, nothing to scatter
  t = fm.touch_masks(L, mask)
  assert t.dtype == np.uint32 and t.shape == (2, 3)
  assert [int(x) for x in t[0]] == [0, 0b0110, 0b1001]
  # molecule 1: node 3 is a hole in the mask that channels 0 and 1 keep (diagonal 1): touched there
  assert [int(x) for x in t[1]] == [0b1000, 0b1100, 0]
  strips = np.zeros(2 * fm.STRIP_INTS + 1, np.int32)
  strips[:8] = [2, 1, 0, 0, 4, 1, 4, 5]    # one strip: molecule 0 at row 0, molecule 1 at row 4
  strips[-1] = 1
  assert fm.strip_touch_counts(strips, t, 3) == [[2]]


def test_model_on_the_bench_plan_and_the_recorded_counter():
  """Touched rows of the seed-0 bench batch on the recorded plan: the worst and the mean strip's
  count per wave and 128-wide layer, derived again from the cost rule, and the whole launch against
  the counter run (the model is pinned to it as strip_mfma_issued is to r04)."""
  from lanczosnet_amd.synthetic import draw_batch
  b = draw_batch(1024, seed=0)
  B, N = b['node_mask'].shape
  L = np.zeros((B, N, N, 7), np.float32)
  for i in range(B):
    n = int(b['n_nodes'][i])
    L[i, :n, :n] = oracle.laplacian_multi_l4(b['adjs'][i, :n, :n])
  touch = fm.touch_masks(L, b['node_mask'])
  rec = np.load(os.path.join(ROOT, 'profiles', 'r06_strip_plan.npz'))
  # the pack's identity bits of that run: bit c set exactly where no row of channel c is touched
  for m in range(B):
    for c in range(7):
      assert bool((int(rec['ident'][m]) >> c) & 1) == (int(touch[m][c]) == 0)
  strips = fm.strips_from_plan(rec['strips'], rec['ident'])
  counts = fm.strip_touch_counts(rec['strips'], touch, 7)
  share = np.array(counts).sum(axis=0) / float(b['n_nodes'].sum())
  assert np.allclose(share, [0.270, 0.094, 0.096, 0.059, 0.040], atol=6e-4)
  r = fm.strip_rare_mfma_issued(strips, counts, QM8_CFG)
  old = fm.strip_mfma_issued(strips, QM8_CFG)
  assert r['rare_strips'] == len(strips) == 244
  # per wave and 128-wide layer of a 5-subtile strip: the channel loop's 2868 less its five folded
  # channels, plus the folded form's cost
  five = [c for t, c in zip(strips, counts) if t['sub'] == 5]
  per = [15 * 160 + 4 * 13 * 2 + 4 * 7 * 13 - fm.rare_cost(5, c, 5)[1] + fm.rare_cost(5, c, 5)[0] for c in five]
  assert 15 * 160 + 4 * 13 * 2 + 4 * 7 * 13 == 2868 and len(five) == 243
  assert r['per_wave_layer_worst'] == max(per) == 2868 - 1060 + 160 + 7 * 52
  nv5 = sum(fm.rare_cost(5, c, 5)[2] for c in five)
  assert r['per_wave_layer_mean'] == np.mean(per) == (243 * 1968 + 52 * nv5) / 243.0
  assert round(r['per_wave_layer_mean'], 2) == 2242.34
  assert 0.77 < r['mfma_issued'] / old['mfma_issued'] < 0.79
  pmc = json.load(open(os.path.join(ROOT, 'profiles', 'r07_strip_rare_pmc.json')))
  assert pmc['kernel'].startswith('lanczosnet_strip_kernel<0, 0, 1,')
  assert pmc['touch_counts_per_strip'] == counts
  measured = pmc['SQ_INSTS_VALU_MFMA_MOPS_F32_per_launch']
  assert abs(r['mops_counts'] - measured) <= 0.002 * measured, (r['mops_counts'], measured)
