"""The cases of tests/train_kernel_cases.py without a GPU: what the GPU files test_gpu_head_grad_edges.py,
test_gpu_mlp_grad_edges.py and test_gpu_gain_grad_edges.py rely on is true of the references alone.

  - every case's float32 reference (the operands as given) meets the bar the kernel is held to,
    max(k e32, 4 * 2^-23) of max|truth| per output tensor, and the truth is finite and not all zero;
  - the operands hold the edges a case claims (empty mask, masked node 0, interior hole, lone last node,
    finite non-zero rows outside the mask, +-100 gate pre-activations; exact 0 / +-1 / underflowing
    eigenvalues, a strict-subset row list whose unused tail points at a NaN row);
  - the share of (layer, row) pairs of the filter MLP on the ReLU kink is under its 5 % cap from the
    float64 reference alone, and nothing is zeroed at one live row;
  - strip_mirror.plan_strips_mirror(extents, 1) makes exactly the ONE strip a gain-gradient case claims
    (subtiles, molecules, a molecule astride two subtiles)."""
import numpy as np
import pytest
import torch

import strip_mirror
import train_kernel_cases as C


def _meets_its_bar(fn, truth, e32, k, what):
  got = fn(torch.float32, 0)
  for name, t in truth.items():
    assert torch.isfinite(t).all(), (what, name)
    s = float(t.abs().max())
    assert s > 0, (what, name)
    err = float((got[name].double() - t).abs().max()) / s
    assert err <= C.bar(e32[name], k), (what, name, err, e32[name])


@pytest.mark.parametrize('case', C.HEAD_CASES, ids=[C.head_id(c) for c in C.HEAD_CASES])
def test_head_case(case):
  B, N, P, n_wg, gate = case
  g100 = case[:4] == C.HEAD_GATE100
  o = C.head_operands(B, N, P, g100)
  truth, e32, _ = C.head_reference(B, N, P, g100)
  _meets_its_bar(lambda dt, d: C.head_eval(o, dt, d), truth, e32, C.K_HEAD, C.head_id(case))
  mask, X = o['mask'], o['X']
  real = torch.zeros((B, 32), dtype=torch.bool)
  real[:, :N] = mask
  assert torch.isfinite(X).all() and (~real).any() and (X[~real] != 0).all()   # finite non-zero outside the mask
  assert (X[real] == 0).any() and (X[real] >= 0).all()           # post-ReLU with exact zeros
  assert (truth['dY'][~mask] == 0).all()
  if B >= 3:
    assert not mask[0, 0] and mask[0].any()                      # a masked node 0
    n1 = int(mask[1].nonzero().max()) + 1
    assert not mask[1, :n1].all() and mask[1, 0]                 # an interior hole
    assert not mask[2].any()                                     # an empty mask
    assert (truth['dY'][2] == 0).all()
  if B > 3:
    assert mask[3].nonzero().flatten().tolist() == [N - 1]       # extent N, count 1
  if g100:
    a = C.head_gate_preactivations(o)
    assert float(a.abs().max()) > 99.0 and float(a.min()) < -50.0 and float(a.max()) > 50.0
  assert 1 <= n_wg and gate in ('stacked', 'split')


def test_head_cases_reach_what_they_name():
  cs = C.HEAD_CASES
  assert {c[2] for c in cs} >= {1, 15, 16, 17, 31}               # P: the exact instantiation, its neighbours, PMAX
  assert any(c[3] == 1 and c[0] > 1 for c in cs) and any(c[3] > c[0] for c in cs)
  assert any(c[0] % c[3] for c in cs if c[3] < c[0])
  assert {c[4] for c in cs} == {'stacked', 'split'}
  assert C.HEAD_GATE100 in [c[:4] for c in cs]


@pytest.mark.parametrize('case', C.MLP_CASES, ids=[C.mlp_id(c) for c in C.MLP_CASES])
def test_mlp_case(case):
  R, parts, L, S, live = case
  o = C.mlp_operands(*case)
  truth, e32, _ = C.mlp_reference(*case)
  _meets_its_bar(lambda dt, d: C.mlp_eval(o, dt, d), truth, e32, C.mlp_k(case), C.mlp_id(case))
  assert o['kink'] < C.KINK_CAP, o['kink']
  if R == 1:
    assert o['kink'] == 0.0                                      # the one row is off the kink
  assert len(o['dist']) == S and 30 in o['dist'] and len(o['layers']) == L
  D = o['D'].reshape(-1)
  idx = o['idx']
  assert idx.numel() == R == len(set(idx.tolist()))
  assert torch.isfinite(D[idx]).all() and torch.isfinite(o['dG'][:, idx]).all()
  if R >= 7:
    d = D[idx].tolist()
    assert 0.0 in d and 1.0 in d and -1.0 in d and any(x < 0 for x in d)
    assert any(x != 0 and np.float32(x) ** np.float32(30) == 0 for x in d)     # underflows at the power 30
  if live is None:
    assert o['rows'] is None and D.numel() == R
  else:
    buf, n = o['rows']
    assert n == R < buf.numel() and buf[:R].tolist() == idx.tolist()
    tail = set(buf[R:].tolist())
    assert len(tail) == 1 and not (tail & set(idx.tolist()))     # the unused entries: one row, not in the list,
    p = tail.pop()
    assert torch.isnan(D[p]) and torch.isnan(o['dG'][:, p]).all()   # whose D and dG are NaN
    asc = bool((idx[1:] > idx[:-1]).all())
    assert asc == (live == 'asc') or R == 1
  tiles = (R + 63) // 64
  if (R, parts) == (65, 5):
    assert parts - tiles == 3                                    # three workgroups own no tile
  if (R, parts) == (129, 1):
    assert tiles == 3 and R % 64 == 1                            # three tiles in one workgroup, ragged tail


def test_mlp_cases_reach_what_they_name():
  cs = C.MLP_CASES
  assert {(c[0], c[1]) for c in cs} >= {(1, 1), (63, 1), (64, 1), (65, 1), (129, 1), (129, 3), (65, 5)}
  assert {c[2] for c in cs} == {1, 2, 16}
  assert {c[3] for c in cs if c[0] == 65 and c[2] == 2} == set(range(1, 9))
  assert {c[4] for c in cs} == {None, 'asc', 'shuffled'}


@pytest.mark.parametrize('name', sorted(C.GAIN_CASES))
def test_gain_case(name):
  c = C.GAIN_CASES[name]
  o = C.gain_operands(name)
  truth, e32, _ = C.gain_reference(name)
  _meets_its_bar(lambda dt, d: C.gain_eval(o, name, dt, d), truth, e32, C.K_GAIN, name)
  ext = np.array(c['mols'])
  plan = strip_mirror.plan_strips_mirror(ext, 1)
  strip_mirror.check_plan(plan, ext)
  assert C.strip_shape(plan) == (1, c['sub'], len(c['mols']), c['straddle']), C.strip_shape(plan)
  B, N, K = o['V'].shape
  for b, n in enumerate(c['mols']):
    v = o['V'][b].double()
    m = min(n, K)
    assert (v[n:] == 0).all() and (v[:, m:] == 0).all()
    assert float((v[:n, :m].t() @ v[:n, :m] - torch.eye(m, dtype=torch.float64)).abs().max()) < 1e-6
    for l in range(c['layers']):
      assert (truth['dG/%d' % l][b, m:] == 0).all()              # dead slots: the truth is identically zero
  assert (o['act'][:, torch.arange(32)[None, :] >= o['n'][:, None]] == 0).all()
  assert tuple(o['x0'].shape) == (B, 32, C.gain_padded_width(c['din']))
  assert (c['form'] == 'strip') == (c['S'] <= 12)


def test_gain_cases_reach_what_they_name():
  cs = C.GAIN_CASES.values()
  assert {c['sub'] for c in cs if c['form'] == 'strip'} == {1, 2, 3, 4, 5, 6}
  assert {c['K'] for c in cs} == {1, 7, 20, 32}
  assert {c['S'] for c in cs} >= {1, 8, 12, 13, 16}
  assert {c['layers'] for c in cs} == {1, 2}
  assert {C.gain_padded_width(c['din']) for c in cs} == {64, 128}
  assert any(len(c['mols']) == 24 and max(c['mols']) <= 4 for c in cs)
  assert any(c['mols'] == [1] for c in cs) and any(c['mols'] == [32] and c['K'] == 32 for c in cs)
  assert {len(c['mols']) for c in cs} >= {1, 5}                  # the tile form's B = 1 and B = 5
