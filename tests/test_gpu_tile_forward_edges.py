"""lanczosnet_forward_kernel (csrc/conv_forward.hip: the inference forward on 32-row tiles, the fallback of the
strip kernels), all five instantiations, held to float64: models the strip launcher refuses (hidden width 64,
input width 32) and width-128 models launched without a strip plan; no plan (four molecules per workgroup in
batch order), single tiles, and pair tiles — an 8|24 pair whose first molecule has exactly 8 nodes, a 16|16 pair
and a lone 32-node molecule, each asserted from the plan words.  Cases, host-drawn operands, references and
bars: tests/forward_cases.py.  Pair tiles exist for diagonal gains AND for dense filters in eigen space
(ops.pairing_supported); both are held here.

Contracts of include/lanczosnet_hip.h pinned here: gains of slots k >= extent are not read (diagonal gains, NaN
included); dense filters there are read against zero rows (any finite value); which rows of state_out a tile
writes; batch position and padded width."""
import numpy as np
import pytest
import torch

import forward_cases as C

_poisoned = C.poisoned_gains

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(C.TILE_CASES))
def test_tile_case(name):
  from lanczosnet_amd import ops
  c = C.CASES[name]
  o = C.forward_operands(name)
  out = C.device_run(name)
  assert out['kernel'] == c['kernel'], out['kernel']
  assert ops.pairing_supported(C.device_model(name)._plan())
  if out['tile_plan'] is not None:
    words, n_wg = out['tile_plan']
    found = C.tile_seams(words, n_wg, o['ext'])
    assert set(c['seams']) <= found, (name, set(c['seams']) - found, words[:12 * n_wg])
    slots = words[:12 * n_wg].reshape(-1, 3)
    ids = sorted(int(x) for x in np.concatenate([slots[:, 0], slots[:, 1]]) if x >= 0)
    assert ids == list(range(len(c['mols'])))                     # every molecule exactly once
  C.hold_to_bars(name, C.device_tensors(o, out))


@pytest.mark.parametrize('name', ['w128_in64/auto', 'w128_in32/auto', 'w64/none_B5', 'w64/single', 'w128_in64/K32',
                                  'w128_in32/K32', 'w64/K32'])
def test_gains_of_dead_slots_are_never_read(name):
  base = C.device_run(name, G=_poisoned(name, 0.0))
  for value in (1e30, float('nan')):
    got = C.device_run(name, G=_poisoned(name, value))
    assert got['kernel'] == base['kernel'] == C.CASES[name]['kernel']
    assert torch.equal(got['score'], base['score']) and torch.equal(got['state'], base['state']), (name, value)
  assert torch.isfinite(base['score']).all()


@pytest.mark.parametrize('name', ['w128_dense/auto', 'w64_dense/none_B5', 'w64_dense/K32', 'w128_dense/K32'])
def test_dense_filters_of_dead_slots_meet_zero_rows(name):
  base = C.device_run(name, G=_poisoned(name, 0.0))
  got = C.device_run(name, G=_poisoned(name, 1e30))
  assert got['kernel'] == base['kernel'] == C.CASES[name]['kernel']
  assert torch.equal(got['score'], base['score']) and torch.equal(got['state'], base['state'])
  assert torch.isfinite(base['score']).all()


@pytest.mark.parametrize('name', ['w128_in64/auto', 'w128_in32/auto', 'w64/auto', 'w128_dense/auto', 'w64_dense/auto'])
def test_partners_in_a_pair_tile_do_not_meet(name):
  """The off-diagonal blocks of a pair tile are zero: with the features and gains of every other molecule
  redrawn, both molecules' partners aside, a molecule of the 8|24 pair keeps its scores and states bit for bit."""
  o = C.forward_operands(name)
  base = C.device_run(name)
  words, n_wg = base['tile_plan']
  pair = next((int(ta), int(tb)) for ta, tb, split in words[:12 * n_wg].reshape(-1, 3) if tb >= 0 and split == 8)
  rs = np.random.RandomState(6)
  for b in pair:
    feat, G = o['feat'].copy(), o['G'].copy()
    others = [i for i in range(feat.shape[0]) if i != b]
    feat[others] = (feat[others] + 1 + rs.randint(0, 60, size=feat[others].shape)) % 70
    G[:, others] = 3.0 * rs.randn(*G[:, others].shape).astype(np.float32)
    if C.CASES[name]['dense']:
      G = 0.5 * (G + np.swapaxes(G, 3, 4))
    got = C.device_run(name, o=dict(o, feat=feat, G=G))
    assert torch.equal(got['score'][b], base['score'][b]) and torch.equal(got['state'][b], base['state'][b]), b
    assert not torch.equal(got['score'][others], base['score'][others])


@pytest.mark.parametrize('name', ['w128_in64/auto', 'w64_dense/auto', 'w64/none_B5'])
def test_rows_a_tile_writes(name):
  """state_out (zeroed by the caller): a single tile writes all 32 rows of its molecule; a pair tile rows
  0 .. split - 1 of its first molecule and 0 .. 31 - split of its second, the rest stays exactly zero.  Rows
  at or beyond the extent hold finite bias-driven values."""
  c = C.CASES[name]
  out = C.device_run(name)
  x = out['state']
  assert torch.isfinite(x).all()
  rows = {b: 32 for b in range(len(c['mols']))}
  if out['tile_plan'] is not None:
    words, n_wg = out['tile_plan']
    for ta, tb, split in words[:12 * n_wg].reshape(-1, 3):
      if ta >= 0 and tb >= 0:
        rows[int(ta)], rows[int(tb)] = int(split), 32 - int(split)
    assert min(rows.values()) < 32
  for b, r in rows.items():
    assert (x[b, r:] == 0).all() and (x[b, :r].abs().sum(dim=1) > 0).all(), (name, b, r)


@pytest.mark.parametrize('name', ['w128_in64/none_B5', 'w64/none_B5', 'w64_dense/none_B5'])
def test_batch_position_and_padded_width(name):
  """The 32-node molecule's neighbour in batch order: the 17-node molecule first and last in the batch, at the
  batch's own N and with a batch cut to N = 17 (the 32-node molecule left out): four positions, the case's bars."""
  c = C.CASES[name]
  o = C.forward_operands(name)
  b = c['mols'].index(17)
  counts = o['mask'].sum(axis=1)
  lo = int(counts[:b].sum())
  small = [i for i in range(len(c['mols'])) if i != b and c['mols'][i] <= 17]
  for rest, N in ((small, 17), ([i for i in range(len(c['mols'])) if i != b], 32)):
    for order in ([b] + rest, rest + [b]):
      ov = C.reorder_operands(o, order, 32)
      if N == 17:
        ov = dict(ov, L=np.ascontiguousarray(ov['L'][:, :17, :17]), V=np.ascontiguousarray(ov['V'][:, :17]),
                  feat=np.ascontiguousarray(ov['feat'][:, :17]), mask=np.ascontiguousarray(ov['mask'][:, :17]))
      out = C.device_run(name, o=ov)
      pos = order.index(b)
      n = int(o['ext'][b])
      keep = torch.from_numpy(o['mask'][b, :n]).bool()
      got = dict(score=out['score'][pos:pos + 1].double(), state=out['state'][pos, :n][keep].double())
      C.hold_to_bars(name, got, rows=dict(score=slice(b, b + 1), state=slice(lo, lo + int(counts[b]))),
                     what=' pos %d N %d' % (pos, N))
