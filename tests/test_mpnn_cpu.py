"""CPU-only: the MPNN module keeps the reference's drop-in surface (tests/golden/mpnn.npz holds the
names, shapes, float64 scores and gradient sums of the unmodified reference class), both float64 mirrors
of tests/mpnn_mirror.py (the reference's pairwise formula and the kernel's factored form) reproduce the
reference and leave L alone, the routes answer without a GPU, and the C entries refuse bad arguments on
the host before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

import mpnn_mirror as G


def _module(name, **over):
  from lanczosnet_amd.model import MPNN
  cfg, batch, use_mask = G.case_inputs(name)
  if over:
    cfg = G.make_config(**dict(G.CASES[name][0], **over))
  return MPNN(cfg), cfg, batch


def _params(name, g):
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  return G.draw_params(zip([str(k) for k in g[name + '_names']], shapes), G.PARAM_SEED[name])


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_mpnn_mirrors_the_reference_surface(name):
  g = load_golden('mpnn.npz')
  net, cfg, _ = _module(name)
  named = list(net.named_parameters())
  assert [k for k, _ in named] == [str(k) for k in g[name + '_names']]      # order included
  assert ['x'.join(str(d) for d in p.shape) for _, p in named] == [str(s) for s in g[name + '_shapes']]
  assert named[0][0] == 'node_embedding.weight' and named[1][0] == 'input_func.0.weight'
  assert set(net.state_dict()) == set(str(k) for k in g[name + '_names'])
  P = _params(name, g)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=True)   # the reference's keys load
  assert torch.equal(net.att_func.W_1.detach(), torch.from_numpy(P['att_func.W_1']))
  assert torch.equal(net.att_func.LSTM.memory_gate[0].weight.detach(),
                     torch.from_numpy(P['att_func.LSTM.memory_gate.0.weight']))


def test_init_reproduces_the_reference_quirks():
  """model/mpnn.py:85-108: edge_func (a ModuleList) and att_func (a Set2Vec) are passed over — edge_func keeps
  torch's default init with nonzero biases, att_func its own constructor init (Xavier, zero gate biases); the
  cell's and the two Sequentials' biases are zero, their weights Xavier-uniform"""
  net, cfg, _ = _module('c')
  for f in net.edge_func:
    assert float(f[0].bias.detach().abs().sum()) > 0.0 and float(f[2].bias.detach().abs().sum()) > 0.0
    w = f[0].weight.detach()                                     # default init: bound 1 / sqrt(fan_in)
    assert float(w.abs().max()) <= 1.0 / np.sqrt(w.shape[1]) + 1e-7
  assert float(net.update_func.bias_ih.detach().abs().sum()) == 0.0
  assert float(net.update_func.bias_hh.detach().abs().sum()) == 0.0
  for lin in (net.input_func[0], net.output_func[0]) + tuple(gate[0] for gate in net.att_func.LSTM.gates()):
    assert float(lin.bias.detach().abs().sum()) == 0.0
  for w in (net.input_func[0].weight, net.output_func[0].weight, net.update_func.weight_ih,
            net.update_func.weight_hh, net.att_func.W_1, net.att_func.W_2, net.att_func.LSTM.forget_gate[0].weight):
    w = w.detach()
    assert float(w.abs().max()) <= np.sqrt(6.0 / (w.shape[0] + w.shape[1])) + 1e-7
    assert float(w.abs().max()) > 0.5 * np.sqrt(6.0 / (w.shape[0] + w.shape[1]))


@pytest.mark.parametrize('name', ['c', 'e'])
def test_init_draws_what_the_reference_draws(name):
  """the same seed gives the reference's own stream: creation order, Set2Vec's init inside its constructor,
  weight_hh before weight_ih.  Restated here: a module built by hand in the reference's order."""
  import torch.nn as nn
  cfg, _, _ = G.case_inputs(name)
  from lanczosnet_amd.model import MPNN
  torch.manual_seed(7)
  net = MPNN(cfg)
  torch.manual_seed(7)
  D, Cc = 32, 2
  emb = nn.Embedding(G.NUM_ATOM, 64)
  inp = nn.Linear(64, D)
  cell = nn.GRUCell(D * Cc, D)
  if name == 'e':
    edge = nn.Embedding(Cc, D * D)
  else:
    edge = [nn.Sequential(nn.Linear(2 * D, 64), nn.ReLU(), nn.Linear(64, D)) for _ in range(Cc)]
  gates = [nn.Linear(2 * D, D) for _ in range(4)]
  for lin in gates:
    nn.init.xavier_uniform_(lin.weight.data)
  W_1, W_2 = torch.ones(D, D), torch.ones(D, 1)
  nn.init.xavier_uniform_(W_1)
  nn.init.xavier_uniform_(W_2)
  outp = nn.Linear(2 * D, 16)
  for lin in (inp, outp):
    nn.init.xavier_uniform_(lin.weight.data)
  nn.init.xavier_uniform_(cell.weight_hh.data)
  nn.init.xavier_uniform_(cell.weight_ih.data)
  assert torch.equal(net.node_embedding.weight, emb.weight)
  assert torch.equal(net.input_func[0].weight, inp.weight) and torch.equal(net.output_func[0].weight, outp.weight)
  if name == 'e':
    assert torch.equal(net.edge_embedding.weight, edge.weight)
  else:
    assert torch.equal(net.edge_func[1][2].weight, edge[1][2].weight)
    assert torch.equal(net.edge_func[0][0].bias, edge[0][0].bias)
  assert torch.equal(net.att_func.LSTM.output_gate[0].weight, gates[2].weight)
  assert torch.equal(net.att_func.W_1.detach(), W_1) and torch.equal(net.att_func.W_2.detach(), W_2)
  assert torch.equal(net.update_func.weight_hh, cell.weight_hh) and torch.equal(net.update_func.weight_ih, cell.weight_ih)


@pytest.mark.parametrize('factored', [False, True])
@pytest.mark.parametrize('name', sorted(G.CASES))
def test_float64_mirrors_match_the_reference_float64_scores(name, factored):
  """float64 evaluations of one formula: only the summation order (and, factored, the split of the first
  Linear) differs"""
  g = load_golden('mpnn.npz')
  cfg, batch, use_mask = G.case_inputs(name)
  L0 = batch['L'].copy()
  s = G.forward(_params(name, g), cfg, batch['node_feat'], batch['L'], batch['node_mask'] if use_mask else None,
                factored=factored).numpy()
  ref = g[name + '_score64']
  err = np.abs(s - ref).max() / np.abs(ref).max()
  print('case %s: %s mirror vs reference float64 %.2e' % (name, 'factored' if factored else 'pairwise', err))
  assert err <= 1e-12
  assert np.array_equal(batch['L'], L0)                                  # the mirror leaves L alone


@pytest.mark.parametrize('D', [32, 64, 96, 128])
def test_a_zero_l_leaves_both_mirrors_with_the_gru_cell_on_a_zero_input(D):
  """the yardstick of the GPU test that compares the cell of ggnn_forward and mpnn_forward: with L = 0 the float64
  MPNN and GGNN mirrors, 'avg' and 'sum', are torch.nn.GRUCell on a zero input (asserted inside, to 1e-14)"""
  import test_gpu_mpnn as T
  S, L, W, Wg, truth, e32_m, e32_g = T.zero_message_case(D)
  assert not L.any() and all(torch.equal(a, b) for a, b in zip(W[4:8], Wg[4:8]))
  assert float((truth - S.double()).abs().max()) > 1e-2                  # the state moved
  assert 0.0 < e32_m < 1e-5 and 0.0 < e32_g < 1e-5


def test_the_module_float64_torch_restatement_matches_the_reference_on_the_host():
  """route 'mpnn_torch' is plain torch: called directly (forward() itself refuses a CPU module) in float64 it
  reproduces the reference's float64 scores, MLP and embedding, masked and not"""
  g = load_golden('mpnn.npz')
  for name in ('c', 'd', 'e', 'f'):
    net, cfg, batch = _module(name)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in _params(name, g).items()})
    net = net.double()
    use_mask = G.CASES[name][2]
    with torch.no_grad():
      s = net._torch_forward(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']).double(),
                             torch.from_numpy(batch['node_mask']) if use_mask else None).numpy()
    ref = g[name + '_score64']
    assert np.abs(s - ref).max() / np.abs(ref).max() <= 1e-12, name
    if name == 'c':   # what this agreement is worth: the drawn batch is asymmetric (a swap of the halves of W1
      L = batch['L']  # shows), has negative entries, rows of degree 0 inside the mask and a one-node molecule
      assert (L < 0).any() and ((L != 0) != (L.transpose(0, 2, 1, 3) != 0)).any()
      degree = (L != 0).sum(axis=2)                                       # [B, N, C]
      assert (degree[batch['node_mask'] != 0] == 0).any() and (degree > 1).any()
      assert int(batch['node_mask'].sum(axis=1).min()) == 1
      swapped = {k: (torch.cat([v[:, 32:], v[:, :32]], dim=1) if k.startswith('edge_func') and k.endswith('0.weight')
                     else v) for k, v in net.state_dict().items()}
      net.load_state_dict(swapped)
      with torch.no_grad():
        s2 = net._torch_forward(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']).double(),
                                torch.from_numpy(batch['node_mask'])).numpy()
      assert np.abs(s2 - ref).max() / np.abs(ref).max() > 1e-6            # ... and the swap does show


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
  many, _, _ = _module('c', num_bond_type=8)
  assert '9 channels' in many._why_not_hip(5, torch.zeros(1, 5, 5, 9), False, False)
  emb, _, _ = _module('e')
  assert 'edge embedding' in emb._why_not_hip(5, L, False, False)
  odd, _, _ = _module('c', input_dim=40)
  assert 'input_dim=40' in odd._why_not_hip(5, L, False, False)
  big, _, _ = _module('c', output_dim=17)
  assert 'output_dim=17' in big._why_not_hip(5, L, False, False)
  assert 'float32' in net.double()._why_not_hip(5, L, False, False)


def test_an_unknown_message_function_raises_at_construction():
  with pytest.raises(ValueError, match='Non-supported message function'):
    _module('c', msg='attention')


def test_cpu_module_raises():
  net, _, batch = _module('c')
  with pytest.raises(RuntimeError, match='GPU only'):
    net(torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L']),
        mask=torch.from_numpy(batch['node_mask']))


def test_binding_knows_the_entries_and_they_validate_on_the_host():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  assert 'lnz_mpnn_forward' in _lib.SIGNATURES and 'lnz_set2vec_readout' in _lib.SIGNATURES
  assert _lib.ABI_VERSION == 7                                         # additive: the version stays
  null, one = C.c_void_p(0), C.c_void_p(64)   # never dereferenced: validation fails before any launch
  far = C.c_void_p(1 << 30)

  def run(N=8, Cc=2, D=32, steps=2, B=1, ld0=None, ldso=None, state0=one, L=one, w=one, state_out=far, sb=1, tile=0):
    return lib.lnz_mpnn_forward(state0, D if ld0 is None else ld0, L, sb, 1, 1, 1, w, one, one, one, one, one, one,
                                one, B, N, Cc, D, steps, 1, state_out, D if ldso is None else ldso, tile, null)
  assert run(N=33) == _lib.LNZ_ENOTSUP and b'N = 33' in lib.lnz_last_error()
  for kw in (dict(Cc=9), dict(Cc=0), dict(D=48), dict(D=160), dict(D=0), dict(steps=-1), dict(ld0=34), dict(ldso=34),
             dict(state0=C.c_void_p(68)), dict(w=C.c_void_p(68)), dict(state_out=C.c_void_p((1 << 30) + 4))):
    assert run(**kw) == _lib.LNZ_ENOTSUP, kw
  for kw in (dict(N=0), dict(B=0), dict(state0=null), dict(L=null), dict(w=null), dict(state_out=null), dict(ld0=28),
             dict(ldso=28), dict(sb=-1), dict(tile=48), dict(state_out=C.c_void_p(64 + 16))):
    assert run(**kw) == _lib.LNZ_EINVAL, kw
  assert run(state_out=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()

  def read(N=8, D=32, P=16, steps=2, B=1, ld=None, X=one, w=one, score=far, mpw=0):
    return lib.lnz_set2vec_readout(X, D if ld is None else ld, null, w, one, one, one, one, one, B, N, D, P, steps,
                                   score, mpw, null)
  assert read(N=33) == _lib.LNZ_ENOTSUP and b'N = 33' in lib.lnz_last_error()
  for kw in (dict(D=48), dict(D=160), dict(P=17), dict(P=0), dict(steps=-1), dict(ld=34), dict(X=C.c_void_p(68)),
             dict(w=C.c_void_p(68))):
    assert read(**kw) == _lib.LNZ_ENOTSUP, kw
  for kw in (dict(N=0), dict(B=0), dict(X=null), dict(w=null), dict(score=null), dict(ld=28), dict(mpw=-1),
             dict(mpw=17)):
    assert read(**kw) == _lib.LNZ_EINVAL, kw
  assert read(score=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()


def test_raw_ops_exist():
  from lanczosnet_amd import _torch_ext
  _torch_ext.load()
  assert hasattr(torch.ops.lanczosnet, 'raw_mpnn_forward') and hasattr(torch.ops.lanczosnet, 'raw_set2vec_readout')
