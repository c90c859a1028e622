"""CPU-only: the GPNN module keeps the reference's drop-in surface (tests/golden/gpnn.npz holds the names,
shapes, float64 scores and gradient sums of the unmodified reference class), the float64 mirror of
tests/gpnn_mirror.py reproduces the reference and leaves the three graph tensors alone, the routes answer
without a GPU, the C entry refuses bad arguments on the host before any launch, and the partition Laplacians
match the reference's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

import gpnn_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(name, **over):
  from lanczosnet_amd.model import GPNN
  cfg, batch, use_mask = M.case_inputs(name)
  if over:
    cfg = M.make_config(**dict(M.CASES[name][0], **over))
  return GPNN(cfg), cfg, batch


def _params(name, g):
  shapes = [tuple(int(d) for d in str(s).split('x')) for s in g[name + '_shapes']]
  return M.draw_params(zip([str(k) for k in g[name + '_names']], shapes), M.PARAM_SEED[name])


def _call(net, batch):
  t = torch.from_numpy
  return net(t(batch['node_feat']), t(batch['L']), t(batch['L_cluster']), t(batch['L_cut']),
             mask=t(batch['node_mask']))


@pytest.mark.parametrize('name', sorted(M.CASES))
def test_gpnn_mirrors_the_reference_surface(name):
  from lanczosnet_amd import model
  assert 'GPNN' in model.__all__
  g = load_golden('gpnn.npz')
  net, cfg, _ = _module(name)
  named = list(net.named_parameters())
  names = [k for k, _ in named]
  assert names == [str(k) for k in g[name + '_names']]                     # order included
  assert ['x'.join(str(d) for d in p.shape) for _, p in named] == [str(s) for s in g[name + '_shapes']]
  # embedding, update_func, update_func_partition, state_func.0 / .2, msg_func.*, att_func, input_func, output_func
  assert names[0] == 'embedding.weight' and names[1] == 'update_func.weight_ih'
  assert names[5] == 'update_func_partition.weight_ih' and names[9:13] == [
      'state_func.0.weight', 'state_func.0.bias', 'state_func.2.weight', 'state_func.2.bias']
  assert names[13] == 'msg_func.0.0.weight' and names[-6:] == [
      'att_func.0.weight', 'att_func.0.bias', 'input_func.0.weight', 'input_func.0.bias', 'output_func.0.weight',
      'output_func.0.bias']
  assert set(net.state_dict()) == set(names)
  P = _params(name, g)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=True)
  assert torch.equal(net.update_func_partition.weight_hh.detach(),
                     torch.from_numpy(P['update_func_partition.weight_hh']))


@pytest.mark.parametrize('name', ['a', 'c', 'e'])
def test_init_reproduces_the_reference_quirks(name):
  """model/gpnn.py:107-139: msg_func (a ModuleList) is skipped — default init, nonzero biases; state_func, the
  three other Sequentials and both cells: zero biases, Xavier-uniform weights"""
  net, cfg, _ = _module(name)
  for f in net.msg_func:
    assert float(f[0].bias.detach().abs().sum()) > 0.0 and float(f[2].bias.detach().abs().sum()) > 0.0
  ws = []
  for cell in (net.update_func, net.update_func_partition):
    assert float(cell.bias_ih.detach().abs().sum()) == 0.0 and float(cell.bias_hh.detach().abs().sum()) == 0.0
    ws += [cell.weight_ih, cell.weight_hh]
  for lin in (net.input_func[0], net.att_func[0], net.output_func[0], net.state_func[0], net.state_func[2]):
    assert float(lin.bias.detach().abs().sum()) == 0.0
    ws.append(lin.weight)
  for w in ws:
    w = w.detach()
    assert float(w.abs().max()) <= np.sqrt(6.0 / (w.shape[0] + w.shape[1])) + 1e-7
    assert float(w.abs().max()) > 0.5 * np.sqrt(6.0 / (w.shape[0] + w.shape[1]))


def test_the_mlp_update_is_left_at_torchs_default_init():
  """model/gpnn.py:134-139 asks whether the two Sequentials are nn.Linear: they are not, nothing is drawn anew
  and the biases stay nonzero"""
  net, _, _ = _module('c', update='MLP')
  for seq in (net.update_func, net.update_func_partition):
    assert float(seq[0].bias.detach().abs().sum()) > 0.0
    bound = 1.0 / np.sqrt(seq[0].weight.shape[1])                          # kaiming_uniform(a = sqrt 5)
    assert float(seq[0].weight.detach().abs().max()) <= bound + 1e-7


def test_init_draws_what_the_reference_draws():
  """the same seed gives the reference's own stream: creation order, and both cells' weight_hh before
  weight_ih.  Restated here: a module built by hand in the reference's order."""
  import torch.nn as nn
  cfg, _, _ = M.case_inputs('c')
  from lanczosnet_amd.model import GPNN
  torch.manual_seed(7)
  net = GPNN(cfg)
  torch.manual_seed(7)
  D, Cc = 32, 2
  emb = nn.Embedding(M.NUM_ATOM, 64)
  cell, part = nn.GRUCell(D * Cc, D), nn.GRUCell(D, D)
  st = nn.Sequential(nn.Linear(3 * D, 512), nn.ReLU(), nn.Linear(512, D))
  msg = [nn.Sequential(nn.Linear(D, 128), nn.ReLU(), nn.Linear(128, D)) for _ in range(Cc)]
  att, inp, outp = nn.Linear(D, 1), nn.Linear(64, D), nn.Linear(D, 16)
  for lin in (inp, st[0], st[2], att, outp):                               # model/gpnn.py:108-113
    nn.init.xavier_uniform_(lin.weight.data)
  for c in (cell, part):
    nn.init.xavier_uniform_(c.weight_hh.data)
    nn.init.xavier_uniform_(c.weight_ih.data)
  assert torch.equal(net.embedding.weight, emb.weight)
  assert torch.equal(net.msg_func[1][2].weight, msg[1][2].weight) and torch.equal(net.msg_func[0][0].bias, msg[0][0].bias)
  assert torch.equal(net.state_func[0].weight, st[0].weight) and torch.equal(net.state_func[2].weight, st[2].weight)
  assert torch.equal(net.output_func[0].weight, outp.weight)
  for mine, ref in ((net.update_func, cell), (net.update_func_partition, part)):
    assert torch.equal(mine.weight_hh, ref.weight_hh) and torch.equal(mine.weight_ih, ref.weight_ih)


@pytest.mark.parametrize('name', sorted(M.CASES))
def test_float64_mirror_matches_the_reference_float64_scores(name):
  """both are float64 evaluations of one formula: only the summation order differs"""
  g = load_golden('gpnn.npz')
  cfg, batch, use_mask = M.case_inputs(name)
  keep = {k: batch[k].copy() for k in ('L', 'L_cluster', 'L_cut')}
  s = M.forward(_params(name, g), cfg, batch['node_feat'], batch['L'], batch['L_cluster'], batch['L_cut'],
                batch['node_mask'] if use_mask else None).numpy()
  ref = g[name + '_score64']
  err = np.abs(s - ref).max() / np.abs(ref).max()
  print('case %s: mirror vs reference float64 %.2e' % (name, err))
  assert err <= 1e-12
  for k, v in keep.items():
    assert np.array_equal(batch[k], v)                                     # the mirror leaves the graphs alone


@pytest.mark.parametrize('name', ['b', 'c'])
def test_mirror_gradients_match_the_reference_sums(name):
  """float64 autograd through the mirror against the reference's float32 gradient sums, at the bar the GPU
  training tests hold the torch route to (2e-4 |g|_1 + 1e-9)"""
  g = load_golden('gpnn.npz')
  cfg, batch, use_mask = M.case_inputs(name)
  P = {k: torch.from_numpy(v).double().requires_grad_() for k, v in _params(name, g).items()}
  m, Cc = cfg.model, cfg.dataset.num_bond_type + 1
  t = lambda x: torch.from_numpy(np.asarray(x)).double()  # noqa: E731
  ops_ = M.operands(P, Cc)
  S = P['embedding.weight'][torch.from_numpy(batch['node_feat'])] @ P['input_func.0.weight'].t() + P['input_func.0.bias']
  S = M.propagate(S, t(batch['L']), t(batch['L_cluster']), t(batch['L_cut']), *ops_[:16], m.num_prop,
                  m.num_prop_cluster, m.num_prop_cut, agg=m.aggregate_type, update=m.update_func)
  score = M.readout(S, torch.from_numpy(batch['node_mask']) if use_mask else None, *ops_[16:])
  loss = torch.nn.functional.mse_loss(score, t(batch['label']))
  assert abs(float(loss.detach()) - float(g[name + '_loss'])) < 1e-5 * abs(float(g[name + '_loss']))
  loss.backward()
  for k, gs, ga in zip(g[name + '_names'], g[name + '_gsum'], g[name + '_gabs']):
    gr = P[str(k)].grad
    assert gr is not None, k
    tol = 2e-4 * float(ga) + 1e-9
    assert abs(float(gr.sum()) - float(gs)) < tol, k
    assert abs(float(gr.abs().sum()) - float(ga)) < tol, k


def test_drawn_batches_have_what_the_kernel_tests_rely_on():
  """L: negative entries and a real row without an edge; L_cluster / L_cut: non-negative, a positive diagonal
  on every row (an 'avg' denominator is never near zero), the padded rows 1 on the diagonal"""
  for name in 'cd':
    _, batch, _ = M.case_inputs(name)
    assert (batch['L'] < 0).any()
  for name in 'abcd':
    _, batch, _ = M.case_inputs(name)
    for k in ('L_cluster', 'L_cut'):
      assert (batch[k] >= 0).all() and (np.diagonal(batch[k], axis1=1, axis2=2) > 0).all()
      assert float(batch[k].sum(axis=2).min()) >= 1.0 / batch[k].shape[1]   # the diagonal alone: 1 / (degree + 1)
  _, batch, _ = M.case_inputs('c')
  degree = (batch['L'] != 0).sum(axis=2)                                  # [B, N, C]
  assert (degree[batch['node_mask'] != 0] == 0).any() and (degree > 1).any()
  pad = batch['node_mask'] == 0
  assert pad.any()
  assert np.array_equal(np.diagonal(batch['L_cluster'], axis1=1, axis2=2)[pad], np.ones(int(pad.sum()), np.float32))
  assert (batch['L_cut'] != 0).sum() > batch['L_cut'].shape[0] * batch['L_cut'].shape[1]   # there are cut edges


def test_module_routes_without_a_gpu():
  net, cfg, batch = _module('c')
  L, Lcl, Lct = (torch.from_numpy(batch[k]) for k in ('L', 'L_cluster', 'L_cut'))
  assert net._why_not_hip(5, L, Lcl, Lct, False, False) is None
  assert 'gradients' in net._why_not_hip(5, L, Lcl, Lct, True, False)
  assert 'dropout' in net._why_not_hip(5, L, Lcl, Lct, False, True)
  assert '33 nodes' in net._why_not_hip(33, L, Lcl, Lct, False, False)
  assert 'float32' in net._why_not_hip(5, L.double(), Lcl, Lct, False, False)
  assert 'L_cluster' in net._why_not_hip(5, L, Lcl.double(), Lct, False, False)
  assert 'L_cut' in net._why_not_hip(5, L, Lcl, Lct.double(), False, False)
  wide, _, _ = _module('c', hidden=48)
  assert 'D = 48' in wide._why_not_hip(5, L, Lcl, Lct, False, False)
  rnn, _, _ = _module('e')
  assert 'RNN update' in rnn._why_not_hip(5, L, Lcl, Lct, False, False)
  neg, _, _ = _module('c', cut=-1)
  assert 'num_prop_cut=-1' in neg._why_not_hip(5, L, Lcl, Lct, False, False)
  assert net.last_route is None


@pytest.mark.parametrize('over', [dict(msg=None), dict(update='MLP')])
def test_configurations_the_reference_cannot_run_raise_from_forward(over):
  net, _, batch = _module('c', **over)          # constructs, as the reference's does
  with pytest.raises(NotImplementedError, match='model/gpnn.py'):
    _call(net, batch)


def test_cpu_module_raises():
  net, _, batch = _module('c')
  with pytest.raises(RuntimeError, match='GPU only'):
    _call(net, batch)


def test_binding_knows_the_entry_and_it_validates_on_the_host():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  assert 'lnz_gpnn_forward' in _lib.SIGNATURES
  assert _lib.ABI_VERSION == 7                                         # additive: the version stays
  null, one = C.c_void_p(0), C.c_void_p(64)   # never dereferenced: validation fails before any launch
  far, far2 = C.c_void_p(1 << 30), C.c_void_p(1 << 31)

  def run(N=8, Cc=2, D=32, P=16, steps=2, ncl=1, nct=1, B=1, ld0=None, ldso=None, state0=one, L=one, Lcl=one,
          Lct=one, w=one, wp=one, ws=one, score=far, state_out=far2, sb=1, clb=1, ctc=1, tile=0):
    return lib.lnz_gpnn_forward(state0, D if ld0 is None else ld0, L, sb, 1, 1, 1, Lcl, clb, 1, 1, Lct, 1, 1, ctc,
                                null, w, one, one, one, one, one, one, one, wp, one, one, one, ws, one, one, one,
                                one, one, one, one, B, N, Cc, D, P, steps, ncl, nct, 1, score, state_out,
                                D if ldso is None else ldso, tile, null)
  for kw in (dict(N=33), dict(Cc=9), dict(Cc=0), dict(D=48), dict(D=160), dict(D=0), dict(P=17), dict(P=0),
             dict(steps=-1), dict(ncl=-1), dict(nct=-1), dict(ld0=34), dict(ldso=34), dict(state0=C.c_void_p(68)),
             dict(w=C.c_void_p(68)), dict(wp=C.c_void_p(68)), dict(ws=C.c_void_p(68)),
             dict(state_out=C.c_void_p((1 << 31) + 4)), dict(tile=64)):
    assert run(**kw) == _lib.LNZ_ENOTSUP, kw
    assert b'lnz_gpnn_forward' in lib.lnz_last_error()
  assert run(N=33) == _lib.LNZ_ENOTSUP and b'N = 33' in lib.lnz_last_error()
  assert run(nct=-1) == _lib.LNZ_ENOTSUP and b'num_prop_cut = -1' in lib.lnz_last_error()
  for kw in (dict(N=0), dict(B=0), dict(state0=null), dict(L=null), dict(Lcl=null), dict(Lct=null), dict(w=null),
             dict(wp=null), dict(ws=null), dict(score=null), dict(ld0=28), dict(ldso=28), dict(sb=-1), dict(clb=-1),
             dict(ctc=-1), dict(tile=48), dict(state_out=one), dict(state_out=C.c_void_p(64 + 16)), dict(score=one),
             dict(score=far2)):
    assert run(**kw) == _lib.LNZ_EINVAL, kw
  assert run(state_out=one) == _lib.LNZ_EINVAL and b'alias' in lib.lnz_last_error()


def test_raw_op_exists():
  from lanczosnet_amd import _torch_ext
  _torch_ext.load()
  assert hasattr(torch.ops.lanczosnet, 'raw_gpnn_forward')


def test_the_header_names_the_entry_in_its_change_log_at_version_7():
  h = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  log = h[:h.index('#define LNZ_ABI_VERSION')]
  assert 'lnz_gpnn_forward' in log and '#define LNZ_ABI_VERSION 7' in h
  assert 'int lnz_gpnn_forward(' in h[h.index('#define LNZ_ABI_VERSION'):]


def test_partition_laplacians_match_the_reference():
  """get_L_cluster_cut on CPU tensors (plain torch: it runs wherever its operands live) against the
  reference's matrices of the fixture, and the mirror's numpy restatement to the bit"""
  from lanczosnet_amd.utils.spectral_graph_partition import get_L_cluster_cut
  g = load_golden('gpnn.npz')
  _, batch, _ = M.case_inputs('c')
  labels = g['part_node_label'].astype(np.int64)
  assert np.array_equal(labels, batch['node_label'])
  L_simple = torch.from_numpy(batch['L'][..., 0].copy())
  keep = L_simple.clone()
  Lcl, Lct = get_L_cluster_cut(L_simple, torch.from_numpy(labels))
  assert torch.equal(L_simple, keep)
  assert Lcl.dtype == torch.float32 and tuple(Lcl.shape) == tuple(g['part_L_cluster'].shape)
  assert np.abs(Lcl.numpy() - g['part_L_cluster']).max() <= 1e-6
  assert np.abs(Lct.numpy() - g['part_L_cut']).max() <= 1e-6
  assert np.array_equal(batch['L_cluster'], g['part_L_cluster'].astype(np.float32))
  assert np.array_equal(batch['L_cut'], g['part_L_cut'].astype(np.float32))
  # the collate fixture under the reference's spectral_clustering labels: the padded rows are isolated nodes
  _, big, _ = M.case_inputs('a')
  Lcl, Lct = get_L_cluster_cut(torch.from_numpy(big['L'][..., 0].copy()), torch.from_numpy(big['node_label']))
  assert np.abs(Lcl.numpy() - big['L_cluster']).max() <= 1e-6 and np.abs(Lct.numpy() - big['L_cut']).max() <= 1e-6
  pad = big['node_mask'] == 0
  assert pad.any() and np.array_equal(np.diagonal(Lct.numpy(), axis1=1, axis2=2)[pad], np.ones(int(pad.sum()), np.float32))
  with pytest.raises(ValueError):
    get_L_cluster_cut(torch.zeros(2, 3, 3), torch.zeros(2, 4, dtype=torch.long))


@pytest.mark.parametrize('D', [32, 64, 96, 128])
def test_the_identity_state_mlp_returns_its_state_block_exactly_in_float32(D):
  """the construction behind test_gpu_gpnn's comparison of the GGNN step in gpnn_forward and in ggnn_forward: with
  these weights state_func is the identity on S to the bit, whatever stands in the Sc and Sx blocks and in whatever
  order the chains are summed, so GPNN with both partition counts 0 is the GGNN recurrence"""
  Ws1, bs1, Ws2, bs2 = M.identity_state_mlp(D)
  assert tuple(Ws1.shape) == (M.STATE_HIDDEN, 3 * D) and tuple(Ws2.shape) == (D, M.STATE_HIDDEN)
  assert int((Ws1 != 0).sum()) == 2 * D and int((Ws2 != 0).sum()) == 2 * D and not bs1.any() and not bs2.any()
  assert not Ws1[:, D:].any() and not Ws1[2 * D:].any() and not Ws2[:, 2 * D:].any()
  g = torch.Generator().manual_seed(40 + D)
  S = torch.randn(14, 5, D, generator=g) * torch.tensor([1e-20, 1.0, 1e20, 3.0, 1e-3]).view(1, 5, 1)
  other = torch.randn(14, 5, 2 * D, generator=g)
  out = torch.relu(torch.cat([S, other], dim=2) @ Ws1.t() + bs1) @ Ws2.t() + bs2
  assert out.dtype == torch.float32 and torch.equal(out, S)
  perm = torch.randperm(M.STATE_HIDDEN, generator=g)                          # another order of the hidden sum
  assert torch.equal(torch.relu(torch.cat([S, other], dim=2) @ Ws1[perm].t()) @ Ws2[:, perm].t(), S)
  # ... and through the mirror: GPNN without partition steps is the GGNN recurrence to the bit
  W = [0.1 * torch.randn(*s, generator=g) for s in ((2, M.HIDDEN, D), (2, M.HIDDEN), (2, D, M.HIDDEN), (2, D),
                                                      (3 * D, 2 * D), (3 * D,), (3 * D, D), (3 * D,))]
  L = (torch.rand(14, 5, 5, 2, generator=g) < 0.4).float()
  z = torch.zeros(14, 5, 5)
  part = [torch.zeros(3 * D, D), torch.zeros(3 * D), torch.zeros(3 * D, D), torch.zeros(3 * D)]
  mine = M.propagate(S, L, z, z, *W, *part, Ws1, bs1, Ws2, bs2, 3, 0, 0)
  assert torch.equal(mine, M.G.propagate(S, L, *W, 3))
