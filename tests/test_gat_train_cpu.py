"""CPU-only: the backward formulas of csrc/gat_grad.hip (tests/gat_grad_mirror.py) against float64 autograd
through tests/gat_mirror.py, the four C entries of the GAT backward on the host (known to the binding,
refusing bad arguments before any launch), their raw ops, and the routing of the opt-in switch
`LANCZOSNET_GAT_BACKWARD` / `GAT.gat_backward_impl`."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import gat_grad_mirror as M
import gat_mirror as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 4, 1), (5, 2, 3, 16, 3), (17, 2, 3, 32, 1)]   # (N, C, H, Dh, B)


def _close(got, ref, what):
  for name, a, b in zip(what, got, ref):
    assert a.shape == b.shape and a.dtype == b.dtype, name
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= 1e-12 * scale, (name, err, scale)


@pytest.mark.parametrize('elu', [True, False])
@pytest.mark.parametrize('N,Cc,H,Dh,B', SHAPES)
def test_attention_backward_formulas_match_float64_autograd(N, Cc, H, Dh, B, elu):
  g = torch.Generator().manual_seed(300 + N + Dh)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
  Wh, L = 0.5 * r(B, N, Cc * H * Dh), 0.5 * torch.rand(B, N, N, Cc, generator=g, dtype=torch.float64)
  a1, a2, b1, b2, bias = 0.3 * r(Cc * H, Dh), 0.3 * r(Cc * H, Dh), 0.1 * r(Cc * H), 0.1 * r(Cc * H), 0.1 * r(Cc * H, Dh)
  dOut = r(B, N, Cc * H * Dh)
  out = G.attention(Wh, L, a1, b1, a2, b2, bias, H, elu)
  got = M.attention_backward(Wh, L, a1, b1, a2, b2, out, dOut, H, elu)
  ref = M.attention_autograd(Wh, L, a1, b1, a2, b2, bias, dOut, H, elu)
  _close(got, ref, M.ATT_NAMES)
  if N == 1:   # a one-row softmax is exactly 1 and dP - t cancels exactly
    for k in (1, 2, 3, 4):
      assert float(got[k].abs().max()) == 0.0 and float(ref[k].abs().max()) == 0.0


@pytest.mark.parametrize('mkind', ['ragged', None])
@pytest.mark.parametrize('N,Cc,H,Dh,B', SHAPES)
def test_readout_backward_formulas_match_float64_autograd(N, Cc, H, Dh, B, mkind):
  g = torch.Generator().manual_seed(400 + N + Dh)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
  CH, P = Cc * H, 5
  Hl, Wo, bo, wg, bg, dscore = r(B, N, CH * Dh), 0.4 * r(P, Dh), 0.1 * r(P), 0.4 * r(1, Dh), 0.1 * r(1), r(B, P)
  mask = None
  if mkind == 'ragged':
    n = torch.randint(1, N + 1, (B,), generator=g)
    mask = (torch.arange(N).unsqueeze(0) < n.unsqueeze(1)).to(torch.uint8)
  got = M.readout_backward(Hl, mask, Wo, bo, wg, bg, CH, dscore)
  ref = M.readout_autograd(Hl, mask, Wo, bo, wg, bg, CH, dscore)
  _close(got, ref, M.RO_NAMES)
  if mask is not None:
    assert float(got[0][mask == 0].abs().max() if (mask == 0).any() else 0.0) == 0.0


def test_mirror_computes_in_the_dtype_of_its_operands():
  g = torch.Generator().manual_seed(9)
  r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
  Wh, L = r(2, 5, 2 * 3 * 4), torch.rand(2, 5, 5, 2, generator=g)
  a1, a2, b1, b2, bias = r(6, 4), r(6, 4), r(6), r(6), r(6, 4)
  out = G.attention(Wh, L, a1, b1, a2, b2, bias, 3, True)
  assert all(x.dtype == torch.float32 for x in M.attention_backward(Wh, L, a1, b1, a2, b2, out, r(2, 5, 24), 3))
  assert all(x.dtype == torch.float32
             for x in M.readout_backward(Wh, None, r(3, 4), r(3), r(1, 4), r(1), 6, r(2, 3)))


def test_binding_knows_the_backward_entries_and_they_validate_on_the_host():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  for name in ('lnz_gat_attention_backward', 'lnz_gat_attention_backward_workspace_floats',
               'lnz_gat_readout_backward', 'lnz_gat_readout_backward_workspace_floats'):
    assert name in _lib.SIGNATURES and hasattr(lib, name)
  assert _lib.ABI_VERSION == 7 and lib.lnz_abi_version() == 7          # additive: the version stays
  null, one = C.c_void_p(0), C.c_void_p(64)   # never dereferenced: validation fails before any launch
  far = lambda k: C.c_void_p(k << 24)  # noqa: E731  (16 MiB apart: no ranges overlap)

  def att(N=8, Cc=2, H=2, Dh=16, ldw=None, ldo=None, ldd=None, ldg=None, Wh=far(1), out=far(2), dOut=far(3),
          dWh=far(4), elu=1, sb=1, ws=one, da1=one):
    w = Cc * H * Dh
    ld = lambda x: w if x is None else x  # noqa: E731
    return lib.lnz_gat_attention_backward(Wh, ld(ldw), one, sb, 1, 1, 1, one, one, one, one, out, ld(ldo), dOut,
                                          ld(ldd), 1, N, Cc, H, Dh, elu, ws, dWh, ld(ldg), da1, one, one, one, one,
                                          null)
  assert att(N=33) == _lib.LNZ_ENOTSUP and b'N = 33' in lib.lnz_last_error()
  assert att(Dh=6) == _lib.LNZ_ENOTSUP
  assert att(Dh=36) == _lib.LNZ_ENOTSUP
  assert att(Cc=9) == _lib.LNZ_ENOTSUP
  assert att(H=17) == _lib.LNZ_ENOTSUP
  for k in ('ldw', 'ldo', 'ldd', 'ldg'):
    assert att(**{k: 66}) == _lib.LNZ_ENOTSUP, k                       # not a multiple of 4
    assert att(**{k: 60}) == _lib.LNZ_EINVAL, k                        # below the width
  for k in ('Wh', 'dOut', 'dWh', 'ws', 'da1'):
    assert att(**{k: null}) == _lib.LNZ_EINVAL, k
  assert att(out=null, elu=1) == _lib.LNZ_EINVAL and b'elu' in lib.lnz_last_error()
  assert att(N=0) == _lib.LNZ_EINVAL
  assert att(sb=-1) == _lib.LNZ_EINVAL
  assert att(Wh=C.c_void_p((1 << 24) + 4)) == _lib.LNZ_EINVAL          # not 16-byte aligned
  assert att(dWh=far(1)) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()      # dWh is Wh
  assert att(dWh=C.c_void_p((3 << 24) + 16)) == _lib.LNZ_EINVAL        # overlaps dOut
  assert att(dWh=far(2)) == _lib.LNZ_EINVAL                            # dWh is out

  def ro(N=8, CH=4, Dh=16, P=16, ld=None, ldg=None, Hl=far(1), dH=far(2), dscore=one, ws=one):
    w = CH * Dh
    return lib.lnz_gat_readout_backward(Hl, w if ld is None else ld, null, one, one, one, one, dscore, 1, N, CH,
                                        Dh, P, ws, dH, w if ldg is None else ldg, one, one, one, one, null)
  assert ro(P=17) == _lib.LNZ_ENOTSUP
  assert ro(N=33) == _lib.LNZ_ENOTSUP
  assert ro(Dh=33) == _lib.LNZ_ENOTSUP
  assert ro(ld=60) == _lib.LNZ_EINVAL
  assert ro(ldg=60) == _lib.LNZ_EINVAL
  assert ro(Hl=null) == _lib.LNZ_EINVAL and ro(dscore=null) == _lib.LNZ_EINVAL and ro(ws=null) == _lib.LNZ_EINVAL
  assert ro(P=0) == _lib.LNZ_EINVAL
  assert ro(dH=far(1)) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()

  wa = lib.lnz_gat_attention_backward_workspace_floats
  wr = lib.lnz_gat_readout_backward_workspace_floats
  assert 0 < wa(1, 7, 8, 16) < wa(2, 7, 8, 16) < wa(1024, 7, 8, 16)
  assert wa(3, 7, 8, 16) == 3 * 56 * (3 * 16 + 2)                      # [da1 | da2 | dbias | db1 | db2] per molecule
  assert 0 < wr(1, 16, 16) < wr(2, 16, 16) < wr(1024, 16, 16)
  assert wr(3, 16, 16) == 3 * (16 * 16 + 16 + 16 + 1)


def test_raw_backward_ops_exist():
  from lanczosnet_amd import _torch_ext
  _torch_ext.load()
  for name in ('raw_gat_attention_backward', 'raw_gat_attention_backward_workspace_floats',
               'raw_gat_readout_backward', 'raw_gat_readout_backward_workspace_floats'):
    assert hasattr(torch.ops.lanczosnet, name), name
  assert torch.ops.lanczosnet.raw_gat_readout_backward_workspace_floats(2, 16, 16) == 2 * 289
  from lanczosnet_amd import ops
  assert callable(ops.gat_attention_backward) and callable(ops.gat_readout_backward) and callable(ops.gat_layer_backward)


def _module(name):
  from lanczosnet_amd.model import GAT
  cfg, batch = G.case_inputs(name)
  return GAT(cfg), torch.from_numpy(batch['L'])


def test_switch_defaults_to_torch_and_is_read_from_the_environment():
  code = ('from lanczosnet_amd.model import GAT; print("impl=" + GAT.gat_backward_impl)')
  for value, expect in ((None, 'torch'), ('hip', 'hip')):
    env = {k: v for k, v in os.environ.items() if k != 'LANCZOSNET_GAT_BACKWARD'}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    if value is not None:
      env['LANCZOSNET_GAT_BACKWARD'] = value
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, check=True).stdout
    assert 'impl=' + expect in out


def test_switch_routes_without_a_gpu():
  net, L = _module('c')
  net.gat_backward_impl = 'torch'
  assert 'gradients' in net._why_not_hip(5, L, True, False)            # unchanged
  assert net._why_not_hip(5, L, False, False) is None
  net.gat_backward_impl = 'hip'
  assert net._why_not_hip(5, L, True, False) is None
  assert 'dropout' in net._why_not_hip(5, L, True, True)
  assert '33 nodes' in net._why_not_hip(33, L, True, False)
  assert 'float32' in net._why_not_hip(5, L.double(), True, False)
  assert net._why_not_hip(5, L, False, False) is None
  other, _ = _module('c')                                               # an instance attribute: the class keeps its own
  assert type(other).gat_backward_impl == os.environ.get('LANCZOSNET_GAT_BACKWARD', 'torch')
