"""CPU-only: the backward formulas of csrc/ggnn_grad.hip (tests/ggnn_grad_mirror.py) against float64
autograd through tests/ggnn_mirror.py, the switch of route 'ggnn_hip_train' without a GPU, and the host-side
validation of the new C entries."""
import ctypes as C
import os
import re

import pytest
import torch

import ggnn_grad_mirror as GM
import ggnn_mirror as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
  scale = float(b.abs().max())
  err = float((a - b).abs().max())
  return err / scale if scale > 0 else err


def _compare(S, L, W, dST, steps, agg):
  d = lambda x: x.double()  # noqa: E731
  W8 = [d(w) for w in W[:8]]
  mine = GM.propagate_backward(d(S), d(dST), d(L), W8, steps, agg)
  auto = GM.propagate_autograd(d(S), d(dST), d(L), W8, steps, agg)
  for name, a, b in zip(GM.STEP_NAMES, mine, auto):
    assert a.shape == b.shape, name
    assert _rel(a, b) <= 1e-12, (name, _rel(a, b))
  return auto


@pytest.mark.parametrize('steps,agg', [(1, 'avg'), (3, 'avg'), (3, 'sum')])
def test_step_formulas_equal_float64_autograd(steps, agg):
  N, C, D, B = 7, 3, 32, 3
  S, L, W = GM.draw_operands(500 + steps, B, N, C, D)                 # an ASYMMETRIC L
  assert not torch.equal(L != 0, (L != 0).transpose(1, 2))
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(7))
  auto = _compare(S, L, W, dST, steps, agg)
  assert all(float(g.abs().max()) > 0 for g in auto)


def test_a_missing_transpose_in_dM_shows_on_an_asymmetric_L_only():
  """ggnn_mirror.draw_inputs is symmetric: with 'sum' Â_c^T = Â_c and a backward that forgets the transpose
  passes on it.  The asymmetric draw tells the two apart."""
  d = lambda x: x.double()  # noqa: E731
  N, C, D, B = 5, 2, 32, 3
  S, L, W = GM.draw_operands(41, B, N, C, D)
  Lsym = torch.from_numpy(G.draw_inputs(81, B, N, C)['L'])
  assert torch.equal(Lsym != 0, (Lsym != 0).transpose(1, 2)) and not torch.equal(L != 0, (L != 0).transpose(1, 2))
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(8))
  W8 = [d(w) for w in W[:8]]
  for Lx, caught in ((Lsym, False), (L, True)):
    auto = GM.propagate_autograd(d(S), d(dST), d(Lx), W8, 1, 'sum')
    good = GM.step_backward(d(S), d(dST), d(Lx), *W8, agg='sum')
    wrong = GM.step_backward(d(S), d(dST), d(Lx), *W8, agg='sum', transpose_dM=False)
    assert _rel(good[0], auto[0]) <= 1e-12
    assert (_rel(wrong[0], auto[0]) > 1e-3) == caught


def test_degree_zero_rows_and_an_empty_channel():
  N, C, D, B = 6, 3, 32, 3
  S, L, W = GM.draw_operands(43, B, N, C, D)
  L[0, 2] = 0.0                   # a row without an edge in every channel
  L[:, :, 4] = 0.0                # a column nobody reads: its dM is exactly zero
  L[1, :, :, 1] = 0.0             # a whole channel without an edge
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(9))
  for agg in ('avg', 'sum'):
    _compare(S, L, W, dST, 2, agg)


def test_readout_formulas_equal_float64_autograd():
  N, D, B, P = 6, 32, 3, 16
  S, L, W = GM.draw_operands(44, B, N, 1, D, P=P)
  dscore = torch.randn(B, P, generator=torch.Generator().manual_seed(10)).double()
  mask = (torch.arange(N).unsqueeze(0) < torch.tensor([6, 3, 1]).unsqueeze(1)).to(torch.uint8)
  head = [w.double() for w in W[8:]]
  for mk in (None, mask):
    mine = GM.readout_backward(S.double(), mk, *head, dscore)
    auto = GM.readout_autograd(S.double(), mk, *head, dscore)
    for name, a, b in zip(GM.RO_NAMES, mine, auto):
      assert _rel(a, b) <= 1e-12, name
    if mk is not None:
      assert float(mine[0][1, 3:].abs().max()) == 0.0 and float(mine[0][2, 1:].abs().max()) == 0.0


def _module(name, **over):
  from lanczosnet_amd.model import GGNN
  cfg, batch, _ = G.case_inputs(name)
  if over:
    cfg = G.make_config(**dict(G.CASES[name][0], **over))
  return GGNN(cfg), torch.from_numpy(batch['L'])


def test_the_switch_routes_without_a_gpu():
  from lanczosnet_amd.model import GGNN
  net, L = _module('c')
  assert GGNN.ggnn_backward_impl == os.environ.get('LANCZOSNET_GGNN_BACKWARD', 'torch')
  net.ggnn_backward_impl = 'torch'
  why = net._why_not_hip(5, L, True, False)
  assert 'gradients' in why and 'LANCZOSNET_GGNN_BACKWARD' in why
  net.ggnn_backward_impl = 'hip'
  assert net._why_not_hip(5, L, True, False) is None
  assert net._why_not_hip(5, L, False, False) is None
  assert 'dropout' in net._why_not_hip(5, L, True, True)
  assert '33 nodes' in net._why_not_hip(33, L, True, False)
  wide, _ = _module('c', hidden=48)
  wide.ggnn_backward_impl = 'hip'
  assert 'D = 48' in wide._why_not_hip(5, L, True, False)
  rnn, _ = _module('e')
  rnn.ggnn_backward_impl = 'hip'
  assert 'RNN update' in rnn._why_not_hip(5, L, True, False)


NEW = ('lnz_ggnn_forward_states', 'lnz_ggnn_backward_step', 'lnz_ggnn_readout_backward',
       'lnz_ggnn_readout_backward_workspace_floats')


def test_the_new_entries_are_in_the_change_log_and_the_version_stays():
  from lanczosnet_amd import _lib
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  assert re.search(r'#define LNZ_ABI_VERSION 7\b', hdr) and _lib.ABI_VERSION == 7
  log = hdr.split('#define LNZ_ABI_VERSION')[0]
  for name in NEW:
    assert name.replace('_workspace_floats', '') in log, name
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
    return lib.lnz_ggnn_backward_step(S, D if lds is None else lds, dSn, D, L, sb, 1, 1, 1, w, one, one, one, one, one,
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

  def readout(N=8, D=32, P=16, B=1, ld=None, S=one, ws=one, dS=None):
    dS = outs[0] if dS is None else dS
    return lib.lnz_ggnn_readout_backward(S, D if ld is None else ld, null, one, one, one, one, one, B, N, D, P, ws, dS,
                                         D, one, one, one, one, null)
  assert readout(N=33) == _lib.LNZ_ENOTSUP
  assert readout(D=48) == _lib.LNZ_ENOTSUP
  assert readout(D=160) == _lib.LNZ_ENOTSUP
  assert readout(P=17) == _lib.LNZ_ENOTSUP
  assert readout(B=0) == _lib.LNZ_EINVAL
  assert readout(S=null) == _lib.LNZ_EINVAL
  assert readout(ws=null) == _lib.LNZ_EINVAL
  assert readout(ld=28) == _lib.LNZ_EINVAL
  assert readout(dS=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
  assert lib.lnz_ggnn_readout_backward_workspace_floats(3, 128, 16) == 3 * (16 * 128 + 16 + 128 + 1)
  assert lib.lnz_ggnn_readout_backward_workspace_floats(0, 128, 16) == 0

  far, far2 = C.c_void_p(1 << 30), C.c_void_p(1 << 31)

  def states(N=8, D=32, steps=2, st=None):
    st = C.c_void_p(1 << 32) if st is None else st
    return lib.lnz_ggnn_forward_states(one, D, one, 1, 1, 1, 1, null, one, one, one, one, one, one, one, one, one, one,
                                       one, one, 1, N, 2, D, 16, steps, 1, far, far2, D, st, 0, null)
  assert states(N=33) == _lib.LNZ_ENOTSUP and b'lnz_ggnn_forward_states' in lib.lnz_last_error()
  assert states(D=48) == _lib.LNZ_ENOTSUP
  assert states(steps=-1) == _lib.LNZ_ENOTSUP
  assert states(st=null) == _lib.LNZ_EINVAL
  assert states(st=C.c_void_p((1 << 32) + 4)) == _lib.LNZ_ENOTSUP        # not 16-byte aligned
  assert states(st=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
  assert states(st=far2) == _lib.LNZ_EINVAL
