"""The cases of tests/forward_cases.py without a GPU: what tests/test_gpu_strip_forward_edges.py and
tests/test_gpu_tile_forward_edges.py rely on is true of the references alone.

  - every case's references run, the truth is finite and not all zero, the float32 reference (the operands as
    given) meets the bar the kernel is held to, and the spread of the eight evaluations is at most the case's k;
  - every bar, for every tensor, is at most 5e-6: half the 1e-5 the forward kernels are held to elsewhere;
  - the operands hold what a case claims: connected molecules, V zero at rows >= extent and slots >= extent, no
    empty mask, and in every batch of four or more an interior hole, a masked node 0 and a masked last node the
    operator keeps;
  - every strip seam a case claims is in strip_mirror.plan_strips_mirror's plan of its extents, and the case
    lists reach every seam and size the forward kernels' envelope names;
  - the two contracts that need no device hold in the truth: gains (or dense filters) in the slots k >= extent
    cannot matter because V is zero there, and the score is the mean over the nodes the mask keeps."""
import numpy as np
import pytest
import torch

import strip_mirror
import forward_cases as C


@pytest.mark.parametrize('name', list(C.CASES))
def test_case_reference_and_bars(name):
  c = C.CASES[name]
  o = C.forward_operands(name)
  truth, e, spread = C.forward_reference(name)
  k = C.forward_k(name)
  got = C.forward_eval(o, torch.float32, 0, split=c['gemm'] == 'f16x3')
  assert set(truth) == {'score', 'state'} | {'act/%d' % l for l in range(c['layers'])}
  for t, ref in truth.items():
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0, (name, t)
    err = float((got[t].double() - ref).abs().max()) / float(ref.abs().max())
    b = C.bar(e[t], k)
    assert err <= b, (name, t, err, b)
    assert spread[t] <= k, (name, t, spread[t])
    assert b <= C.BAR_CAP, (name, t, b)
  assert tuple(truth['score'].shape) == (len(c['mols']), c['dout'])
  assert truth['state'].shape[0] == int(o['mask'].sum())


@pytest.mark.parametrize('name', list(C.CASES))
def test_case_operands(name):
  c = C.CASES[name]
  o = C.forward_operands(name)
  mask, ext, L, V = o['mask'], o['ext'], o['L'], o['V']
  B, N = mask.shape
  assert B == len(c['mols']) <= 30 and N == max(c['mols']) <= 32 and L.shape[3] == c['n_edge']
  assert mask.any(axis=1).all()                                   # no empty mask
  for b, n in enumerate(c['mols']):
    reach = np.linalg.matrix_power((L[b, :n, :n, 0] != 0).astype(np.float64), n) > 0
    assert reach.all(), (name, b)                                 # connected
    assert (L[b, n:] == 0).all() and (L[b, :, n:] == 0).all()
    e = int(ext[b])
    assert (V[b, e:] == 0).all() and (V[b, :, min(e, c['K']):] == 0).all()
    if c['K'] > n:
      assert (o['G'][:, b, ..., n:] != 0).all()                   # drawn there, and must not matter
  if B >= 4:
    last, hole, zero = C._special_molecules(c)
    assert ext[last] == c['mols'][last] - 1 and L[last, ext[last], ext[last], 0] != 0   # masked, kept by L
    assert not mask[hole, c['mols'][hole] // 2] and mask[hole, 0] and ext[hole] == c['mols'][hole]
    assert not mask[zero, 0] and mask[zero, 1]
  if c['dense']:
    assert (o['G'] == np.swapaxes(o['G'], 3, 4)).all()
  elif c['S'] > 0:
    assert (o['G'] < 0).any() and (o['G'] > 0).any()
  if c['special'] == 'sparse_operator':
    rare = L[..., 2:]
    assert (rare != np.swapaxes(rare, 1, 2)).any(axis=(1, 2)).all()          # no mirror, in every rare channel
  if c['special'] == 'no_rare_bonds':
    assert all((L[b, :n, :n, 2] == np.eye(n)).all() for b, n in enumerate(c['mols']))
  if c['general']:
    assert (o['feat'][mask == 0] != 0).all()                                 # features on holes and padding too
  if c['special'] == 'any_operator':
    e1 = L[0, :c['mols'][0], :c['mols'][0], 1]
    assert (e1 != 0).all() and not np.allclose(e1, e1.T)


@pytest.mark.parametrize('name', list(C.STRIP_CASES))
def test_strip_case_seams_in_the_mirror_plan(name):
  c = C.STRIP_CASES[name]
  ext = C.case_extents(name)
  plan = strip_mirror.plan_strips_mirror(ext, c['n_cu'])
  strip_mirror.check_plan(plan, ext)
  found = C.strip_seams(plan)
  assert set(c['seams']) <= found, (name, set(c['seams']) - found, plan)
  if name in C.STRIP_ENVELOPE:
    assert len(plan) == 1
  # the strips that fold, by the kernel's cost rule on the host-drawn L: what the case claims, and every strip
  # of at most five subtiles of a geometry case
  assert C.expected_rare_strips(name, plan) == c['rare_strips'], (name, C.expected_rare_strips(name, plan))
  if name in C.STRIP_GEOMETRY:
    assert c['rare_strips'] == sum(1 for _, sub in plan if sub <= 5)


def test_strip_cases_reach_what_they_name():
  geo, env = C.STRIP_GEOMETRY.values(), C.STRIP_ENVELOPE.values()
  claimed = set().union(*[set(c['seams']) for c in geo])
  assert claimed >= {'h1', 'h2', 'h3', 'h4', 'h5', 'h6', 'start4', 'start8', 'start12', 'rows12_31',
                     'two_full_subtiles', 'mols_in_subtile_2', 'mols_in_subtile_3', 'skip_dead', 'tail_dead', 'mol24',
                     'n1', 'n2', 'n3', 'n4', 'pad5', 'B1', 'two_heights', 'straddle', 'two_rows_across'}
  assert all((c['layers'], c['K'], c['S'], c['n_edge'], c['din'], c['dhid']) == (7, 20, 8, 7, 64, 128) for c in geo)
  assert {c['K'] for c in env if not c['dense']} >= {1, 3, 20, 32}
  assert {c['K'] for c in env if c['dense']} >= {4, 20, 32}
  assert {c['S'] for c in env} >= {0, 1, 12}
  assert {len(c['short']) for c in env} >= {0, 1, 8} and any(max(c['short'], default=0) == 8 for c in env)
  assert {c['n_edge'] for c in env} >= {1, 2, 3, 7, 8} and any(c['S'] + c['n_edge'] == 32 for c in env)
  assert {(c['din'], c['general']) for c in env} >= {(64, False), (128, False), (1, True), (65, True)}
  assert {c['dout'] for c in env} >= {1, 31} and {c['layers'] for c in env} >= {1, 16}
  assert any(c['act'] for c in env) and any(c['gemm'] == 'f16x3' for c in env)
  assert {c['special'] for c in env} >= {'any_operator', 'any_V', 'sparse_operator', 'no_rare_bonds'}
  assert any(c['n_edge'] == 3 and c['rare_strips'] == 1 for c in env)      # the smallest that folds, folding
  assert C.STRIP_ENVELOPE['sparse_operator']['rare_strips'] == 1 and C.STRIP_ENVELOPE['edge7']['rare_strips'] == 1
  assert {c['kernel'] for c in env} == {C.RARE, C.PLAIN, C.SHORT, C.DENSE, C.DENSE_SHORT, C.SPLIT}


def test_tile_cases_reach_what_they_name():
  cs = C.TILE_CASES.values()
  assert {c['kernel'] for c in cs} == {C.TILE % a for a in ((4, 0, 1), (4, 0, -1), (2, 0, -1), (4, 2, 0), (2, 2, 0))}
  for kern in {c['kernel'] for c in cs}:
    mine = [c for c in cs if c['kernel'] == kern]
    assert {c['tiling'] for c in mine} == {'none', 'single', 'auto'}
    assert {len(c['mols']) for c in mine if c['tiling'] == 'none'} == {1, 4, 5}
    assert any({'pair8_exact', 'pair16', 'lone32'} <= set(c['seams']) for c in mine)
    assert {c['K'] for c in mine} == {1, 3, 20, 32}


@pytest.mark.parametrize('name', ['K20', 'K20_dense', 'w64_dense/auto', 'h6_mol24'])
def test_dead_slots_cannot_matter_in_the_truth(name):
  """V[:, :, k] = 0 for k >= extent, so whatever G (or DD) holds there meets a zero column: the float64 forward
  with those slots zeroed and with them at 1e30 is the same, bit for bit."""
  c = C.CASES[name]
  o = C.forward_operands(name)
  K = c['K']
  dead = np.arange(K)[None, :] >= np.minimum(o['ext'], K)[:, None]            # [B,K]
  assert dead.any()
  out = []
  for fill in (0.0, 1e30):
    G = o['G'].copy()
    if c['dense']:
      G[:, dead[:, None, :, None] | dead[:, None, None, :] | np.zeros_like(G[0], bool)] = fill
    else:
      G[:, dead[:, None, :] | np.zeros_like(G[0], bool)] = fill
    out.append(C.forward_eval(o, torch.float64, 0, G=G))
  base = C.forward_eval(o, torch.float64, 0)
  for t in base:
    assert torch.equal(out[0][t], out[1][t]), (name, t)
    assert float((out[0][t] - base[t]).abs().max()) <= 1e-12 * float(base[t].abs().max()), (name, t)


@pytest.mark.parametrize('name', ['K20', 'w128_in64/auto'])
def test_score_is_the_mean_over_the_kept_nodes(name):
  """The head's y of every node from the truth's final state; the score is its mean over the nodes the mask
  keeps — a hole and a masked last node are left out of the sum AND of the count."""
  o = C.forward_operands(name)
  truth, _, _ = C.forward_reference(name)
  P = {k: torch.from_numpy(v).double() for k, v in o['params'].items()}
  nl = o['cfg']['num_layer']
  x = truth['state']
  y = (x @ P['filter.%d.weight' % nl].t() + P['filter.%d.bias' % nl]) * \
      torch.sigmoid(x @ P['att_func.0.weight'].t() + P['att_func.0.bias'])
  counts = o['mask'].sum(axis=1)
  assert (counts < o['ext']).any()                                # some molecule keeps fewer nodes than its extent
  lo = 0
  for b, n in enumerate(counts):
    want = y[lo:lo + int(n)].mean(dim=0)
    assert float((truth['score'][b] - want).abs().max()) <= 1e-12 * float(truth['score'].abs().max())
    by_extent = y[lo:lo + int(n)].sum(dim=0) / float(o['ext'][b])
    if n < o['ext'][b]:
      assert float((truth['score'][b] - by_extent).abs().max()) > 1e-3 * float(truth['score'][b].abs().max())
    lo += int(n)
