"""CPU-only: the backward formulas of csrc/mpnn_grad.hip (tests/mpnn_grad_mirror.py) against float64 autograd
through tests/mpnn_mirror.py, the kink condition of every kernel-level GPU case, the switch of route
'mpnn_hip_train' without a GPU, and the host-side validation of the new C entries."""
import ctypes as C
import os
import re

import pytest
import torch

import mpnn_grad_mirror as GM
import mpnn_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
  scale = float(b.abs().max())
  err = float((a - b).abs().max())
  return err / scale if scale > 0 else err


def _compare(S, L, W, dST, steps, agg):
  d = lambda x: x.double()  # noqa: E731
  W8 = [d(w) for w in W]
  mine = GM.propagate_backward(d(S), d(dST), d(L), W8, steps, agg)
  auto = GM.propagate_autograd(d(S), d(dST), d(L), W8, steps, agg)
  for name, a, b in zip(GM.STEP_NAMES, mine, auto):
    assert a.shape == b.shape, name
    assert _rel(a, b) <= 1e-12, (name, _rel(a, b))
  return auto


@pytest.mark.parametrize('steps,agg', [(1, 'avg'), (3, 'avg'), (1, 'sum'), (3, 'sum')])
def test_step_formulas_equal_float64_autograd(steps, agg):
  N, C, D, B = 7, 3, 32, 3
  S, L, W = GM.draw_operands(500 + steps, B, N, C, D)                 # an ASYMMETRIC L, a row of degree 0
  assert not torch.equal(L != 0, (L != 0).transpose(1, 2))
  assert bool(((L != 0).sum(dim=2) == 0).any())
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(7))
  auto = _compare(S, L, W, dST, steps, agg)
  assert all(float(g.abs().max()) > 0 for g in auto)
  if steps == 1:   # one step of step_backward is propagate_backward
    d = lambda x: x.double()  # noqa: E731
    one = GM.step_backward(d(S), d(dST), d(L), *[d(w) for w in W], agg=agg)
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(one, auto))


def test_the_ordered_mirror_is_the_factored_mirror():
  N, C, D, B = 6, 3, 32, 2
  S, L, W = GM.draw_operands(40, B, N, C, D)
  d = lambda x: x.double()  # noqa: E731
  ref = M.propagate_factored(d(S), d(L), *[d(w) for w in W], 3, agg='avg')
  traj = GM.propagate(d(S), d(L), *[d(w) for w in W], 3, agg='avg', trajectory=True)
  assert len(traj) == 4 and torch.equal(traj[0], d(S)) and _rel(traj[3], ref) <= 1e-14
  assert _rel(GM.propagate(d(S), d(L), *[d(w) for w in W], 3, agg='avg', order=[2, 0, 1]), ref) <= 1e-13


def test_swapped_halves_and_a_missing_transpose_show_on_an_asymmetric_L():
  """dP_c[b] sums over the edges INTO b, dQ_c[a] over the edges of a, and the neighbour half of W1 goes with dP:
  a backward that takes the halves the other way round, or sums dP over the row's own edges, is told apart from
  the right one on the asymmetric draw (in dS; the missing transpose in dW1 too)."""
  d = lambda x: x.double()  # noqa: E731
  N, C, D, B = 5, 2, 32, 3
  S, L, W = GM.draw_operands(41, B, N, C, D)
  assert not torch.equal(L != 0, (L != 0).transpose(1, 2))
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(8))
  W8 = [d(w) for w in W]
  auto = GM.propagate_autograd(d(S), d(dST), d(L), W8, 1, 'sum')
  good = GM.step_backward(d(S), d(dST), d(L), *W8, agg='sum')
  assert _rel(good[0], auto[0]) <= 1e-12 and _rel(good[1], auto[1]) <= 1e-12
  swapped = GM.step_backward(d(S), d(dST), d(L), *W8, agg='sum', swap_halves=True)
  assert _rel(swapped[0], auto[0]) > 1e-3
  untransposed = GM.step_backward(d(S), d(dST), d(L), *W8, agg='sum', transpose_dP=False)
  assert _rel(untransposed[0], auto[0]) > 1e-3 and _rel(untransposed[1], auto[1]) > 1e-3


def test_degree_zero_rows_and_an_empty_channel():
  N, C, D, B = 6, 3, 32, 3
  S, L, W = GM.draw_operands(43, B, N, C, D)
  L[0, 2] = 0.0                   # a row without an edge in every channel
  L[:, :, 4] = 0.0                # a column nobody reads: its dP is exactly zero
  L[1, :, :, 1] = 0.0             # a whole channel without an edge
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(9))
  for agg in ('avg', 'sum'):
    _compare(S, L, W, dST, 2, agg)
  L[:, :, :, 2] = 0.0             # a channel without an edge in the whole batch: its weights have zero gradients
  auto = _compare(S, L, W, dST, 2, 'avg')
  assert float(auto[1][2].abs().max()) == 0.0 and float(auto[3][2].abs().max()) == 0.0


def _kink_cases():
  for N, Cc, D, B, steps, agg, _, lkind in GM.STEP_CASES:
    yield 'step N %d C %d D %d B %d %s' % (N, Cc, D, B, agg), GM.step_case_inputs(N, Cc, D, B, steps, agg, lkind)[:3], \
        steps, agg
  S, _, ones, W, _ = GM.edge_case()
  for agg in ('avg', 'sum'):
    yield 'edge semantics %s' % agg, (S, ones, W), GM.EDGE_DRAW[5], agg
  seed, N, Cc, D, B, steps, density = GM.REPEAT_DRAW
  yield 'repeatability', GM.draw_operands(seed, B, N, Cc, D, density=density), steps, 'avg'
  yield 'saturated gates', GM.saturated_case()[:3], GM.SATURATED_DRAW[5], 'avg'


@pytest.mark.parametrize('tag,operands,steps,agg', list(_kink_cases()), ids=[c[0] for c in _kink_cases()])
def test_every_kernel_level_case_is_kink_free(tag, operands, steps, agg):
  S, L, W = operands
  smallest, widest, count = GM.kink_figures(S, L, W, steps, agg)
  print('%s: %d edge pre-activations, smallest %.2e, |pre32 - pre64| <= %.2e' % (tag, count, smallest, widest))
  assert count <= 135000
  assert smallest >= GM.KINK_RATIO * widest, (tag, smallest, widest)


def _module(name, **over):
  from lanczosnet_amd.model import MPNN
  cfg, batch, _ = M.case_inputs(name)
  if over:
    cfg = M.make_config(**dict(M.CASES[name][0], **over))
  return MPNN(cfg), torch.from_numpy(batch['L'])


def test_the_switch_routes_without_a_gpu():
  from lanczosnet_amd.model import MPNN
  net, L = _module('c')
  assert MPNN.mpnn_backward_impl == os.environ.get('LANCZOSNET_MPNN_BACKWARD', 'torch')
  net.mpnn_backward_impl = 'torch'
  why = net._why_not_hip(5, L, True, False)
  assert 'gradients' in why and 'LANCZOSNET_MPNN_BACKWARD=hip' in why
  assert net._why_not_hip(5, L, False, False) is None
  net.mpnn_backward_impl = 'hip'
  assert net._why_not_hip(5, L, True, False) is None
  assert net._why_not_hip(5, L, False, False) is None
  assert 'dropout' in net._why_not_hip(5, L, True, True)
  assert '33 nodes' in net._why_not_hip(33, L, True, False)
  wide, _ = _module('c', hidden=48)
  wide.mpnn_backward_impl = 'hip'
  assert 'D = 48' in wide._why_not_hip(5, L, True, False)
  emb, _ = _module('e')
  emb.mpnn_backward_impl = 'hip'
  assert 'edge embedding' in emb._why_not_hip(5, L, True, False)
  net._transpose_cache = ('stale', None)
  net.invalidate_plan()
  assert net._transpose_cache is None and net._pack_cache is None


NEW = ('lnz_mpnn_forward_states', 'lnz_mpnn_backward_step')


def test_the_new_entries_are_in_the_change_log_and_the_version_stays():
  from lanczosnet_amd import _lib
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  assert re.search(r'#define LNZ_ABI_VERSION 7\b', hdr) and _lib.ABI_VERSION == 7
  log = hdr.split('#define LNZ_ABI_VERSION')[0]
  for name in NEW:
    assert name in log, name
    assert name in _lib.SIGNATURES, name
  lib = _lib.load()
  assert lib.lnz_abi_version() == 7
  from lanczosnet_amd import _torch_ext
  _torch_ext.load()
  for name in NEW:
    assert hasattr(torch.ops.lanczosnet, 'raw_' + name[4:]), name


def test_the_new_entries_validate_on_the_host():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  null, one = C.c_void_p(0), C.c_void_p(64)   # never dereferenced: validation fails before any launch
  outs = [C.c_void_p((k + 1) << 30) for k in range(8)]

  def step(N=8, Cc=2, D=32, B=1, lds=None, S=one, dSn=None, L=one, w=one, wt=one, dS=None, sb=1, buf=None):
    dSn = C.c_void_p(1 << 29) if dSn is None else dSn
    o = list(outs)
    if dS is not None:
      o[0] = dS
    if buf is not None:
      o[3] = buf
    return lib.lnz_mpnn_backward_step(S, D if lds is None else lds, dSn, D, L, sb, 1, 1, 1, w, one, one, one, one, one,
                                      one, one, wt, one, one, one, B, N, Cc, D, 1, o[0], D, o[1], o[2], o[3], o[4],
                                      o[5], o[6], null)
  assert step(N=33) == _lib.LNZ_ENOTSUP and b'N = 33' in lib.lnz_last_error()
  assert step(Cc=9) == _lib.LNZ_ENOTSUP
  assert step(D=48) == _lib.LNZ_ENOTSUP
  assert step(D=160) == _lib.LNZ_ENOTSUP
  assert step(lds=34) == _lib.LNZ_ENOTSUP                               # rows not 16-byte aligned
  assert step(S=C.c_void_p(68)) == _lib.LNZ_ENOTSUP
  assert step(wt=C.c_void_p(68)) == _lib.LNZ_ENOTSUP
  assert step(N=0) == _lib.LNZ_EINVAL
  assert step(B=0) == _lib.LNZ_EINVAL
  assert step(S=null) == _lib.LNZ_EINVAL
  assert step(wt=null) == _lib.LNZ_EINVAL
  assert step(buf=null) == _lib.LNZ_EINVAL
  assert step(lds=28) == _lib.LNZ_EINVAL                                # below the width
  assert step(sb=-1) == _lib.LNZ_EINVAL
  assert step(dS=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
  assert step(buf=outs[1]) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()

  far = C.c_void_p(1 << 30)

  def states(N=8, D=32, steps=2, st=None, out=far, tile=0, S=one):
    st = C.c_void_p(1 << 32) if st is None else st
    return lib.lnz_mpnn_forward_states(S, D, one, 1, 1, 1, 1, one, one, one, one, one, one, one, one, 1, N, 2, D, steps,
                                       1, out, D, st, tile, null)
  assert states(N=33) == _lib.LNZ_ENOTSUP and b'lnz_mpnn_forward_states' in lib.lnz_last_error()
  assert states(D=48) == _lib.LNZ_ENOTSUP
  assert states(steps=-1) == _lib.LNZ_ENOTSUP
  assert states(st=null) == _lib.LNZ_EINVAL
  assert states(S=null) == _lib.LNZ_EINVAL
  assert states(st=C.c_void_p((1 << 32) + 4)) == _lib.LNZ_ENOTSUP        # not 16-byte aligned
  assert states(st=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
  assert states(st=far) == _lib.LNZ_EINVAL                                # the trajectory over state_out
  assert states(tile=48) == _lib.LNZ_EINVAL
  # the forward entry keeps its own checks: state_out is required there
  assert lib.lnz_mpnn_forward(one, 32, one, 1, 1, 1, 1, one, one, one, one, one, one, one, one, 1, 8, 2, 32, 2, 1,
                              null, 32, 0, null) == _lib.LNZ_EINVAL
  assert lib.lnz_mpnn_forward(one, 32, one, 1, 1, 1, 1, one, one, one, one, one, one, one, one, 1, 8, 2, 32, 2, 1,
                              one, 32, 0, null) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
