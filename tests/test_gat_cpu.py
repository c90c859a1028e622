"""CPU-only: the GAT module keeps the reference's drop-in surface (tests/golden/gat.npz holds the
names, shapes and float64 scores of the unmodified reference class), the float64 mirror of
tests/gat_mirror.py reproduces the reference, the bias aliasing shows, and the two C entries refuse
bad arguments on the host before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

import gat_mirror as G


def _module(name):
  from lanczosnet_amd.model import GAT
  cfg, batch = G.case_inputs(name)
  return GAT(cfg), cfg, batch


def _params(name, g):
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  return G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_gat_mirrors_the_reference_surface(name):
  g = load_golden('gat.npz')
  net, cfg, _ = _module(name)
  named = list(net.named_parameters())
  assert [k for k, _ in named] == [str(k) for k in g[name + '_names']]      # order included: bias_* first
  assert ['x'.join(str(d) for d in p.shape) for _, p in named] == [str(s) for s in g[name + '_shapes']]
  assert named[0][0] == 'bias_0_0_0' and named[1][0] == 'bias_1_0_0'
  assert set(net.state_dict()) == set(str(k) for k in g[name + '_names'])
  # a dict with the reference's keys loads (strict)
  P = _params(name, g)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  assert torch.equal(net.embedding.weight.detach(), torch.from_numpy(P['embedding.weight']))
  # the init leaves every bias zero and draws Xavier weights (model/gat.py:88-123)
  fresh, _, _ = _module(name)
  E = cfg.dataset.num_bond_type
  assert float(fresh.att_net_1[0][E][0].bias.detach().abs().sum()) == 0.0
  w = fresh.filter[0][0][0].weight
  assert float(w.abs().max()) <= np.sqrt(6.0 / (w.shape[0] + w.shape[1])) + 1e-7


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_float64_mirror_matches_the_reference_float64_scores(name):
  """both are float64 evaluations of one formula: only the summation order differs"""
  g = load_golden('gat.npz')
  cfg, batch = G.case_inputs(name)
  s = G.forward(_params(name, g), cfg, batch['node_feat'], batch['L'], batch['node_mask']).numpy()
  ref = g[name + '_score64']
  err = np.abs(s - ref).max() / np.abs(ref).max()
  print('case %s: mirror vs reference float64 %.2e' % (name, err))
  assert err <= 1e-12


def test_only_the_last_channels_bias_is_read():
  """model/gat.py:62-70: bias_{h}_{jj}_{t} with jj < E is registered and never used"""
  g = load_golden('gat.npz')
  cfg, batch = G.case_inputs('c')
  E = cfg.dataset.num_bond_type
  P = _params('c', g)
  run = lambda Q: G.forward(Q, cfg, batch['node_feat'], batch['L'], batch['node_mask']).numpy()  # noqa: E731
  base = run(P)
  for jj in range(E):
    Q = dict(P)
    Q['bias_0_%d_0' % jj] = P['bias_0_%d_0' % jj] + 10.0
    assert np.array_equal(run(Q), base)
  Q = dict(P)
  Q['bias_0_%d_0' % E] = P['bias_0_%d_0' % E] + 10.0
  assert np.abs(run(Q) - base).max() > 1e-3 * np.abs(base).max()
  # the fixture says the same of the reference's gradients: None exactly on the unread biases
  names = [str(k) for k in g['c_names']]
  unread = {k for k in names if k.startswith('bias_') and int(k.split('_')[2]) < E}
  assert {k for k, n in zip(names, g['c_grad_none']) if n} == unread


def test_module_resolves_the_bias_by_name_and_routes_without_a_gpu():
  net, cfg, batch = _module('c')
  E = cfg.dataset.num_bond_type
  assert net._used_bias(1, 0) is getattr(net, 'bias_1_%d_0' % E)
  assert not isinstance(getattr(net, 'state_bias', None), list)       # no aliased Python list
  L = torch.from_numpy(batch['L'])
  assert net._why_not_hip(5, L, False, False) is None
  assert 'gradients' in net._why_not_hip(5, L, True, False)
  assert 'dropout' in net._why_not_hip(5, L, False, True)
  assert '33 nodes' in net._why_not_hip(33, L, False, False)
  assert 'float32' in net._why_not_hip(5, L.double(), False, False)


def test_cpu_module_raises():
  net, _, batch = _module('c')
  with pytest.raises(RuntimeError, match='GPU only'):
    net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']),
        mask=torch.from_numpy(batch['node_mask']))


def test_binding_knows_the_entries_and_they_validate_on_the_host():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  assert 'lnz_gat_attention' in _lib.SIGNATURES and 'lnz_gat_readout' in _lib.SIGNATURES
  assert _lib.ABI_VERSION == 7                                         # additive: the version stays
  null, one = C.c_void_p(0), C.c_void_p(64)   # never dereferenced: validation fails before any launch

  def att(N=8, Cc=2, H=2, Dh=16, ldw=None, ldo=None, Wh=one, out=C.c_void_p(1 << 20), sb=1, B=1):
    w = Cc * H * Dh
    return lib.lnz_gat_attention(Wh, w if ldw is None else ldw, one, sb, 1, 1, 1, one, one, one, one, one, B, N,
                                 Cc, H, Dh, 1, out, w if ldo is None else ldo, null)
  assert att(N=33) == _lib.LNZ_ENOTSUP and b'N = 33' in lib.lnz_last_error()
  assert att(Dh=6) == _lib.LNZ_ENOTSUP
  assert att(Dh=36) == _lib.LNZ_ENOTSUP
  assert att(Cc=9) == _lib.LNZ_ENOTSUP
  assert att(H=17) == _lib.LNZ_ENOTSUP
  assert att(ldw=66) == _lib.LNZ_ENOTSUP
  assert att(ldo=66) == _lib.LNZ_ENOTSUP
  assert att(N=0) == _lib.LNZ_EINVAL
  assert att(Wh=null) == _lib.LNZ_EINVAL
  assert att(ldw=60) == _lib.LNZ_EINVAL                                # below the width
  assert att(sb=-1) == _lib.LNZ_EINVAL
  assert att(Wh=C.c_void_p(68)) == _lib.LNZ_EINVAL                     # not 16-byte aligned
  assert att(out=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
  assert att(out=C.c_void_p(64 + 16)) == _lib.LNZ_EINVAL               # overlapping ranges

  def ro(N=8, CH=4, Dh=16, P=16, ld=None, Hl=one):
    return lib.lnz_gat_readout(Hl, CH * Dh if ld is None else ld, null, one, one, one, one, 1, N, CH, Dh, P, one,
                               null)
  assert ro(P=17) == _lib.LNZ_ENOTSUP
  assert ro(N=33) == _lib.LNZ_ENOTSUP
  assert ro(Dh=33) == _lib.LNZ_ENOTSUP
  assert ro(ld=60) == _lib.LNZ_EINVAL
  assert ro(Hl=null) == _lib.LNZ_EINVAL
  assert ro(P=0) == _lib.LNZ_EINVAL


def test_raw_ops_exist():
  from lanczosnet_amd import _torch_ext
  _torch_ext.load()
  assert hasattr(torch.ops.lanczosnet, 'raw_gat_attention') and hasattr(torch.ops.lanczosnet, 'raw_gat_readout')
