"""lanczosnet_strip_kernel (csrc/conv_strip.hip), every instantiation, held to float64 at its strip seams and
across the model envelope.  Cases, host-drawn operands, references and bars: tests/forward_cases.py (checked
without a GPU by tests/test_forward_cases_cpu.py).  Every case asserts the seams of the plan the device made, the
kernel ops.last_kernel() names, and every output tensor — scores, final node state, and for the training forward
every layer's activations — against the float64 truth at bar(e32, 4) of max|truth| (e_split for gemm_mode
'f16x3'); error, yardstick and bar are printed per tensor.

Contracts of include/lanczosnet_hip.h pinned here: the gains of the slots k >= extent never reach the result
(diagonal gains: not read, NaN included; dense filters: read against zero rows, so any FINITE value); rows no
molecule owns stay zero in state_out and act_out; a molecule's results do not depend on its batch position or on
the padded node count beyond re-association."""
import numpy as np
import pytest
import torch

import strip_mirror
import forward_cases as C

pytestmark = pytest.mark.gpu


def _check_strip_plan(name, out):
  c = C.CASES[name]
  plan, used, cap = out['strip_plan']
  ext = C.case_extents(name)
  strip_mirror.check_plan(plan, ext)
  found = C.strip_seams(plan)
  assert set(c['seams']) <= found, (name, set(c['seams']) - found, plan)
  mirror = strip_mirror.plan_strips_mirror(ext, c['n_cu'])
  assert [(sorted(m), int(s)) for m, s in plan] == [(sorted((int(b), int(st), int(n)) for b, st, n in m), int(s))
                                                   for m, s in mirror]
  return used, cap


@pytest.mark.parametrize('fold', [True, False], ids=['default', 'channel_loop'])
@pytest.mark.parametrize('name', list(C.STRIP_GEOMETRY))
def test_strip_geometry_at_the_qm8_shape(name, fold):
  c = C.CASES[name]
  o = C.forward_operands(name)
  out = C.device_run(name, fold=fold, fast=fold)
  used, cap = _check_strip_plan(name, out)
  assert out['kernel'] == (C.RARE if fold else C.PLAIN), out['kernel']
  # the strips that took the folded form (the decision is the strip's, the kernel name does not tell): what the
  # cost rule gives on the host-drawn L — every strip of at most five subtiles; a six-subtile strip runs the
  # channel loop inside the rare-capable launch
  want = C.expected_rare_strips(name, out['strip_plan'][0]) if fold else 0
  assert out['rare_strips'] == want == (c['rare_strips'] if fold else 0), (out['rare_strips'], want)
  if fold:
    assert want == sum(1 for _, sub in out['strip_plan'][0] if sub <= 5) and (want >= 1 or 'h6' in c['seams'])
  if name == 'two_heights':
    assert used == 2 and cap > used         # more plan entries than strips in use: the idle workgroups return
  C.hold_to_bars(name, C.device_tensors(o, out), what=' folded' if fold else ' loop')
  if fold:
    assert out['fast_kernel'] == C.RARE and torch.equal(out['fast'], out['score'])
    # without the packed folded weights (the in-register sum): the same bits
    reg = C.device_run(name, packed_fold=False)
    assert reg['kernel'] == C.RARE and reg['rare_strips'] == out['rare_strips']
    assert torch.equal(reg['score'], out['score']) and torch.equal(reg['state'], out['state'])
    if 'h6' in c['seams']:
      # six subtiles: the plain kernel's arithmetic inside the rare-capable launch, bit for bit
      loop = C.device_run(name, fold=False)
      assert torch.equal(loop['score'], out['score']) and torch.equal(loop['state'], out['state'])


@pytest.mark.parametrize('name', list(C.STRIP_ENVELOPE))
def test_strip_model_envelope(name):
  c = C.CASES[name]
  o = C.forward_operands(name)
  out = C.device_run(name, act=c['act'])
  used, _ = _check_strip_plan(name, out)
  assert used == 1
  assert out['kernel'] == c['kernel'], out['kernel']
  # folded or not is the strip's decision: the cost rule on the host-drawn L, and what the case claims
  assert out['rare_strips'] == C.expected_rare_strips(name, out['strip_plan'][0]) == c['rare_strips']
  got = C.device_tensors(o, out)
  if c['act']:
    assert set(got) == {'score', 'state'} | {'act/%d' % l for l in range(c['layers'])}
    assert torch.equal(got['state'], got['act/%d' % (c['layers'] - 1)])
  if c['gemm'] == 'f16x3':
    # the header's own parity bar of this mode first: whatever the yardstick below says, this holds
    truth, _, _ = C.forward_reference(name)
    for t in got:
      assert float((got[t] - truth[t]).abs().max()) <= C.SPLIT_HEADER_BAR * float(truth[t].abs().max()), (name, t)
  C.hold_to_bars(name, got)


_poisoned = C.poisoned_gains


# (case, fold, act): the folded and the channel-loop form, the training forward, short channels, split precision
DEAD_SLOT_RUNS = [('K20', True, False), ('K20', False, False), ('K20', True, True), ('K32', True, False),
                  ('short1', True, False), ('split', True, False), ('h6_mol24', True, False),
                  ('sparse_operator', True, False), ('edge3_fold', True, False)]


@pytest.mark.parametrize('name,fold,act', DEAD_SLOT_RUNS)
def test_gains_of_dead_slots_are_never_read(name, fold, act):
  """Diagonal gains: G[l, b, s, k] with k >= extent_b zeroed, at 1e30 and NaN: scores, states and activations
  bit for bit (spectral_gains(zero_fill=False) leaves those slots uninitialised)."""
  base = C.device_run(name, fold=fold, act=act, G=_poisoned(name, 0.0))
  for value in (1e30, float('nan')):
    got = C.device_run(name, fold=fold, act=act, G=_poisoned(name, value))
    assert got['kernel'] == base['kernel'] and got['rare_strips'] == base['rare_strips']
    assert torch.equal(got['score'], base['score']) and torch.equal(got['state'], base['state']), (name, value)
    if act:
      assert torch.equal(got['act'], base['act'])
  assert torch.isfinite(base['score']).all()
  assert base['rare_strips'] == (C.CASES[name]['rare_strips'] if fold and not act else 0)


@pytest.mark.parametrize('name,fold', [('h2_three', True), ('h2_three', False), ('h6_mol24', True), ('K20_dense', True),
                                       ('split', True)])
def test_neighbours_in_a_subtile_do_not_meet(name, fold):
  """The cross-molecule fragments of a block (I, I) are zero: with the features and gains of every OTHER
  molecule of the strip redrawn (L and the masks as they were, so the plan and the strip's form stay), a
  molecule that shares its subtile keeps its scores and node states bit for bit."""
  o = C.forward_operands(name)
  base = C.device_run(name, fold=fold)
  plan = base['strip_plan'][0]
  shared = [b for mols, _ in plan for b, st, n in mols
            if any(b2 != b and st2 // 16 == st // 16 for b2, st2, _ in mols)]
  assert shared
  b = shared[0]
  rs = np.random.RandomState(5)
  feat, G = o['feat'].copy(), o['G'].copy()
  others = [i for i in range(feat.shape[0]) if i != b]
  feat[others] = (feat[others] + 1 + rs.randint(0, 60, size=feat[others].shape)) % 70
  G[:, others] = 3.0 * rs.randn(*G[:, others].shape).astype(np.float32)
  if C.CASES[name]['dense']:
    G = 0.5 * (G + np.swapaxes(G, 3, 4))
  got = C.device_run(name, o=dict(o, feat=feat, G=G), fold=fold)
  assert got['rare_strips'] == base['rare_strips']
  assert torch.equal(got['score'][b], base['score'][b]) and torch.equal(got['state'][b], base['state'][b])
  assert not torch.equal(got['score'][others], base['score'][others])


@pytest.mark.parametrize('name', ['K20_dense', 'K4_dense', 'dense_short'])
def test_dense_filters_of_dead_slots_meet_zero_rows(name):
  """Dense filters: rows and columns k >= extent_b of DD inside the molecule's 4-row padding ARE read, against the
  zero rows of V^T X — any finite value there leaves the same bits (a non-finite one is not filtered)."""
  base = C.device_run(name, G=_poisoned(name, 0.0))
  got = C.device_run(name, G=_poisoned(name, 1e30))
  assert got['kernel'] == base['kernel'] == C.CASES[name]['kernel']
  assert torch.equal(got['score'], base['score']) and torch.equal(got['state'], base['state'])
  assert torch.isfinite(base['score']).all()


@pytest.mark.parametrize('name,fold,act', [('K20', True, False), ('K20', False, True), ('h5_skip', True, False),
                                           ('K20_dense', True, True)])
def test_rows_outside_a_molecule(name, fold, act):
  """state_out / act_out (zeroed by the caller): a molecule's rows 0 .. rows4 - 1 are written (rows4 = its extent
  rounded up to 4 rows, at least 4: real nodes, holes, and the padding rows, which hold finite bias-driven
  values); every row from rows4 on stays exactly zero."""
  o = C.forward_operands(name)
  out = C.device_run(name, fold=fold, act=act)
  tensors = [out['state']] + ([out['act'][l] for l in range(out['act'].shape[0])] if act else [])
  for x in tensors:
    assert torch.isfinite(x).all()
    for b, e in enumerate(o['ext']):
      r4 = C._rows4(int(e))
      assert (x[b, r4:] == 0).all(), (name, b)
      assert (x[b, :r4].abs().sum(dim=1) > 0).all(), (name, b)      # written: relu(bias) is not all zero
  # the hole's and the masked last node's own state is the operator's (they feed their neighbours): the truth
  # of ALL rows the operator keeps, not only the ones the mask keeps
  nodes = np.array(C.CASES[name]['mols'])
  full = dict(o, mask=(np.arange(o['mask'].shape[1])[None, :] < nodes[:, None]).astype(np.uint8))
  truth = C.forward_eval(full, torch.float64, 0)
  N = o['mask'].shape[1]
  got = out['state'][:, :N][torch.from_numpy(full['mask']).bool()].double()
  _, e, _ = C.forward_reference(name)
  err = float((got - truth['state']).abs().max()) / float(truth['state'].abs().max())
  b = C.bar(e['state'], C.forward_k(name))
  print('%s state of every node the operator keeps: err %.2e bar %.2e' % (name, err, b))
  assert err <= b


@pytest.mark.parametrize('name,fold', [('K20', True), ('K20', False), ('split', True), ('K20_dense', True)])
def test_batch_position_and_padded_width(name, fold):
  """The batch's largest molecule first and last in the batch, at N = its node count and at N = 32: its scores
  and node states meet the case's bars in all four positions."""
  c = C.CASES[name]
  o = C.forward_operands(name)
  truth, _, _ = C.forward_reference(name)
  b = int(np.argmax(c['mols']))
  assert o['mask'][b].all() and c['mols'][b] == o['mask'].shape[1] < 32
  counts = o['mask'].sum(axis=1)
  lo = int(counts[:b].sum())
  rest = [i for i in range(len(c['mols'])) if i != b]
  for order in ([b] + rest, rest + [b]):
    for N in (c['mols'][b], 32):
      ov = C.reorder_operands(o, order, N)
      out = C.device_run(name, o=ov, fold=fold)
      pos = order.index(b)
      got = dict(score=out['score'][pos:pos + 1].double(), state=out['state'][pos, :c['mols'][b]].double())
      C.hold_to_bars(name, got, rows=dict(score=slice(b, b + 1), state=slice(lo, lo + int(counts[b]))),
                     what=' pos %d N %d' % (pos, N))
