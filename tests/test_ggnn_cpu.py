"""CPU-only: the GGNN module keeps the reference's drop-in surface (tests/golden/ggnn.npz holds the
names, shapes and float64 scores of the unmodified reference class), the float64 mirror of
tests/ggnn_mirror.py reproduces the reference and leaves L alone, the routes answer without a GPU, and
the C entry refuses bad arguments on the host before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

import ggnn_mirror as G


def _module(name, **over):
  from lanczosnet_amd.model import GGNN
  cfg, batch, use_mask = G.case_inputs(name)
  if over:
    cfg = G.make_config(**dict(G.CASES[name][0], **over))
  return GGNN(cfg), cfg, batch


def _params(name, g):
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  return G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_ggnn_mirrors_the_reference_surface(name):
  g = load_golden('ggnn.npz')
  net, cfg, _ = _module(name)
  named = list(net.named_parameters())
  assert [k for k, _ in named] == [str(k) for k in g[name + '_names']]      # order included
  assert ['x'.join(str(d) for d in p.shape) for _, p in named] == [str(s) for s in g[name + '_shapes']]
  assert named[0][0] == 'embedding.weight' and named[1][0] == 'update_func.weight_ih'
  assert set(net.state_dict()) == set(str(k) for k in g[name + '_names'])
  # a dict with the reference's keys loads (strict)
  P = _params(name, g)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=True)
  assert torch.equal(net.update_func.weight_hh.detach(), torch.from_numpy(P['update_func.weight_hh']))


@pytest.mark.parametrize('name', ['a', 'c', 'e'])
def test_init_reproduces_the_reference_quirks(name):
  """model/ggnn.py:88-120: msg_func (a ModuleList) is skipped — default init, nonzero biases; the cell's
  and the three Sequentials' biases are zero, their weights Xavier-uniform"""
  net, cfg, _ = _module(name)
  for f in net.msg_func:
    assert float(f[0].bias.detach().abs().sum()) > 0.0 and float(f[2].bias.detach().abs().sum()) > 0.0
  assert float(net.update_func.bias_ih.detach().abs().sum()) == 0.0
  assert float(net.update_func.bias_hh.detach().abs().sum()) == 0.0
  for lin in (net.input_func[0], net.att_func[0], net.output_func[0]):
    assert float(lin.bias.detach().abs().sum()) == 0.0
  for w in (net.input_func[0].weight, net.att_func[0].weight, net.output_func[0].weight,
            net.update_func.weight_ih, net.update_func.weight_hh):
    w = w.detach()
    assert float(w.abs().max()) <= np.sqrt(6.0 / (w.shape[0] + w.shape[1])) + 1e-7
    assert float(w.abs().max()) > 0.5 * np.sqrt(6.0 / (w.shape[0] + w.shape[1]))


def test_init_draws_what_the_reference_draws():
  """the same seed gives the reference's own stream: creation order and weight_hh before weight_ih.
  Restated here: a module built by hand in the reference's order."""
  import torch.nn as nn
  cfg, _, _ = G.case_inputs('c')
  from lanczosnet_amd.model import GGNN
  torch.manual_seed(7)
  net = GGNN(cfg)
  torch.manual_seed(7)
  D, Cc = 32, 2
  emb = nn.Embedding(G.NUM_ATOM, 64)
  cell = nn.GRUCell(D * Cc, D)
  msg = [nn.Sequential(nn.Linear(D, 128), nn.ReLU(), nn.Linear(128, D)) for _ in range(Cc)]
  att, inp, outp = nn.Linear(D, 1), nn.Linear(64, D), nn.Linear(D, 16)
  for lin in (inp, att, outp):
    nn.init.xavier_uniform_(lin.weight.data)
  nn.init.xavier_uniform_(cell.weight_hh.data)
  nn.init.xavier_uniform_(cell.weight_ih.data)
  assert torch.equal(net.embedding.weight, emb.weight)
  assert torch.equal(net.msg_func[1][2].weight, msg[1][2].weight) and torch.equal(net.msg_func[0][0].bias, msg[0][0].bias)
  assert torch.equal(net.output_func[0].weight, outp.weight)
  assert torch.equal(net.update_func.weight_hh, cell.weight_hh) and torch.equal(net.update_func.weight_ih, cell.weight_ih)


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_float64_mirror_matches_the_reference_float64_scores(name):
  """both are float64 evaluations of one formula: only the summation order differs"""
  g = load_golden('ggnn.npz')
  cfg, batch, use_mask = G.case_inputs(name)
  L0 = batch['L'].copy()
  s = G.forward(_params(name, g), cfg, batch['node_feat'], batch['L'], batch['node_mask'] if use_mask else None).numpy()
  ref = g[name + '_score64']
  err = np.abs(s - ref).max() / np.abs(ref).max()
  print('case %s: mirror vs reference float64 %.2e' % (name, err))
  assert err <= 1e-12
  assert np.array_equal(batch['L'], L0)                                  # the mirror leaves L alone


def test_drawn_batches_have_degree_zero_rows_and_negative_entries():
  """a REAL row (inside the mask) without an edge in some channel: the EPS denominator is exercised"""
  for name in 'cd':
    _, batch, _ = G.case_inputs(name)
    assert (batch['L'] < 0).any()
  _, batch, _ = G.case_inputs('c')
  degree = (batch['L'] != 0).sum(axis=2)                                # [B, N, C]
  assert (degree[batch['node_mask'] != 0] == 0).any() and (degree > 1).any()


def test_module_routes_without_a_gpu():
  net, cfg, batch = _module('c')
  L = torch.from_numpy(batch['L'])
  assert net._why_not_hip(5, L, False, False) is None
  assert 'gradients' in net._why_not_hip(5, L, True, False)
  assert 'dropout' in net._why_not_hip(5, L, False, True)
  assert '33 nodes' in net._why_not_hip(33, L, False, False)
  assert 'float32' in net._why_not_hip(5, L.double(), False, False)
  wide, _, _ = _module('c', hidden=48)
  assert 'D = 48' in wide._why_not_hip(5, L, False, False)
  rnn, _, _ = _module('e')
  assert 'RNN update' in rnn._why_not_hip(5, L, False, False)


@pytest.mark.parametrize('over', [dict(msg=None), dict(update='MLP')])
def test_configurations_the_reference_cannot_run_raise_from_forward(over):
  net, _, batch = _module('c', **over)          # constructs, as the reference's does
  with pytest.raises(NotImplementedError, match='model/ggnn.py'):
    net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']), mask=torch.from_numpy(batch['node_mask']))


def test_cpu_module_raises():
  net, _, batch = _module('c')
  with pytest.raises(RuntimeError, match='GPU only'):
    net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']),
        mask=torch.from_numpy(batch['node_mask']))


def test_binding_knows_the_entry_and_it_validates_on_the_host():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  assert 'lnz_ggnn_forward' in _lib.SIGNATURES
  assert _lib.ABI_VERSION == 7                                         # additive: the version stays
  null, one = C.c_void_p(0), C.c_void_p(64)   # never dereferenced: validation fails before any launch
  far, far2 = C.c_void_p(1 << 30), C.c_void_p(1 << 31)

  def run(N=8, Cc=2, D=32, P=16, steps=2, B=1, ld0=None, ldso=None, state0=one, L=one, w=one, score=far,
          state_out=far2, sb=1, tile=0):
    return lib.lnz_ggnn_forward(state0, D if ld0 is None else ld0, L, sb, 1, 1, 1, null, w, one, one, one, one, one,
                                one, one, one, one, one, one, B, N, Cc, D, P, steps, 1, score, state_out,
                                D if ldso is None else ldso, tile, null)
  assert run(N=33) == _lib.LNZ_ENOTSUP and b'N = 33' in lib.lnz_last_error()
  assert run(Cc=9) == _lib.LNZ_ENOTSUP
  assert run(Cc=0) == _lib.LNZ_ENOTSUP
  assert run(D=48) == _lib.LNZ_ENOTSUP
  assert run(D=160) == _lib.LNZ_ENOTSUP
  assert run(D=0) == _lib.LNZ_ENOTSUP
  assert run(P=17) == _lib.LNZ_ENOTSUP
  assert run(P=0) == _lib.LNZ_ENOTSUP
  assert run(steps=-1) == _lib.LNZ_ENOTSUP
  assert run(ld0=34) == _lib.LNZ_ENOTSUP                                # rows not 16-byte aligned
  assert run(ldso=34) == _lib.LNZ_ENOTSUP
  assert run(state0=C.c_void_p(68)) == _lib.LNZ_ENOTSUP
  assert run(w=C.c_void_p(68)) == _lib.LNZ_ENOTSUP
  assert run(state_out=C.c_void_p((1 << 31) + 4)) == _lib.LNZ_ENOTSUP
  assert run(N=0) == _lib.LNZ_EINVAL
  assert run(B=0) == _lib.LNZ_EINVAL
  assert run(state0=null) == _lib.LNZ_EINVAL
  assert run(L=null) == _lib.LNZ_EINVAL
  assert run(w=null) == _lib.LNZ_EINVAL
  assert run(score=null) == _lib.LNZ_EINVAL
  assert run(ld0=28) == _lib.LNZ_EINVAL                                # below the width
  assert run(ldso=28) == _lib.LNZ_EINVAL
  assert run(sb=-1) == _lib.LNZ_EINVAL
  assert run(tile=48) == _lib.LNZ_EINVAL
  assert run(state_out=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
  assert run(state_out=C.c_void_p(64 + 16)) == _lib.LNZ_EINVAL          # overlapping ranges
  assert run(score=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()
  assert run(score=far2) == _lib.LNZ_EINVAL                             # score inside state_out


def test_raw_op_exists():
  from lanczosnet_amd import _torch_ext
  _torch_ext.load()
  assert hasattr(torch.ops.lanczosnet, 'raw_ggnn_forward')
