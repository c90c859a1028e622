"""Training graphs of 33..128 nodes through the HIP backward of lnz_midgraph_forward
(csrc/conv_mid_grad.hip: lnz_midgraph_head_grad, lnz_midgraph_input_grad, lnz_midgraph_project;
`_MidGraphFusedFunction`).  Every test opts in (`mid_backward_impl = 'hip'`) and
reads from `ops.last_kernel()` that the new input-gradient kernel ran.

Bars: the project's gradient bars — loss within 1e-5, every parameter tensor's
norm and 16 fixed +-1 projections of its gradient within 1e-5 of |g| (tests/gradproj.py) — against
the unmodified reference's autograd where a fixture exists (train_paths.npz, runner_graph.npz), else
against a float64 restatement of the module's maths with autograd, written here.  The torch route's
own deviation from the same truth is printed beside the kernels'."""
import numpy as np
import pytest
import torch

import oracle
from conftest import load_golden
from gradproj import deterministic_dropout, project_torch
from graph_fixture import GRAPH_CFG
from test_gpu_midgraph import DIST16, _graphs, _net, _t

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KERNEL = 'midgraph_input_grad_kernel<'
SMALL = dict(hidden_dim=[128] * 3, num_layer=3)


def _hip(net):
  net.mid_backward_impl = 'hip'
  return net.train()


def _ran_hip():
  from lanczosnet_amd import ops
  return ops.last_kernel().startswith(KERNEL)


@pytest.fixture(autouse=True)
def launches(monkeypatch):
  """Every call of ops.midgraph_input_grad during a test: what shows that a step did NOT take the new
  route (lnz_last_kernel() keeps the calling thread's last note, which an earlier test may have left)."""
  from lanczosnet_amd import ops
  calls, real = [], ops.midgraph_input_grad

  def counted(*a, **kw):
    calls.append(1)
    return real(*a, **kw)
  monkeypatch.setattr(ops, 'midgraph_input_grad', counted)
  return calls


def _grads(net):
  return {k: p.grad.clone() for k, p in net.named_parameters()}


def _step(net, X, L, D, V, mask, label):
  net.zero_grad(set_to_none=True)
  _, loss = net(X, L, D, V, label=label, mask=mask)
  loss.backward()
  return loss.detach(), _grads(net)


def _truth(net, X, L, D, V, mask, label):
  """float64 restatement of `_torch_forward` (model/lanczos_net.py:143-199 of the reference) with
  autograd: loss and gradients by parameter name."""
  P = {k: v.detach().double().requires_grad_(True) for k, v in net.named_parameters()}
  B = L.shape[0]
  Lc, Vd = L.double().permute(0, 3, 1, 2), V.double()
  state = X.double() if net.general else P['embedding.weight'][X]
  S, nl = net.num_scale_long, net.num_layer
  pows = torch.stack([D.double() ** p for p in net.long_diffusion_dist], dim=2) if S else None
  for t in range(nl):
    W, bias = P['filter.%d.weight' % t], P['filter.%d.bias' % t]
    Wc = W.view(W.shape[0], -1, state.shape[2])
    out, c = bias.view(1, 1, -1), 0
    if S:
      G = pows
      if net._has_mlp():
        h = pows.reshape(-1, S)
        for i in (0, 2, 4, 6):
          h = h @ P['spectral_filter.%d.%d.weight' % (t, i)].t() + P['spectral_filter.%d.%d.bias' % (t, i)]
          h = torch.relu(h) if i < 6 else h
        G = h.view(B, -1, S)
      Y = Vd.transpose(1, 2) @ state
      for s in range(S):
        out = out + Vd @ (G[:, :, s:s + 1] * (Y @ Wc[:, c].t()))
        c += 1
    for e in range(Lc.shape[1]):
      out = out + Lc[:, e] @ (state @ Wc[:, c].t())
      c += 1
    state = torch.relu(out)
  y = (state @ P['filter.%d.weight' % nl].t() + P['filter.%d.bias' % nl]) * \
      torch.sigmoid(state @ P['att_func.0.weight'].t() + P['att_func.0.bias'])
  m = (mask != 0).double().unsqueeze(2)
  loss = net.loss_func((y * m).sum(dim=1) / m.sum(dim=1), label.double())
  names = list(P)
  return loss.detach(), dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names])))


def _deviation(grads, truth):
  """Worst of |projection of (g - truth)| and | |g| - |truth| |, in units of |truth|, over the tensors."""
  worst = (0.0, None)
  for i, k in enumerate(sorted(truth)):
    t = truth[k]
    nrm = float(t.norm())
    if nrm == 0.0:
      assert float(grads[k].abs().max()) == 0.0, k
      continue
    e = max(float(np.abs(project_torch(grads[k].double() - t, i)).max()) / nrm,
            abs(float(grads[k].double().norm()) - nrm) / nrm)
    if e >= worst[0]:
      worst = (e, k)
  return worst


def _against_float64(net, X, L, D, V, mask, label, tag, launches):
  _hip(net)
  loss, g = _step(net, X, L, D, V, mask, label)
  assert _ran_hip() and len(launches) == 1 and net.last_route == 'mid_train_hip'
  net.mid_backward_impl = 'torch'
  loss_t, g_t = _step(net, X, L, D, V, mask, label)
  assert len(launches) == 1 and net.last_route == 'torch'
  loss64, truth = _truth(net, X, L, D, V, mask, label)
  e_hip, e_torch = _deviation(g, truth), _deviation(g_t, truth)
  print('%s: gradients vs float64 autograd, worst of |g|: HIP %.2e (%s), torch route %.2e (%s); loss %.2e / %.2e'
        % (tag, e_hip[0], e_hip[1], e_torch[0], e_torch[1], abs(float(loss) - float(loss64)) / float(loss64),
           abs(float(loss_t) - float(loss64)) / float(loss64)))
  assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
  assert e_hip[0] < 1e-5, e_hip


def _batch(rs, cfg, B, N, nmin, K, p=0.3, second=None, net_seed=3, general=True, name='LanczosNetGeneral'):
  """net + inputs.  second: None = the collated L (equal channels); 'all' / 'mixed' = channel 1
  replaced by a sparser graph's Laplacian in every / every other graph; 'nonsym' = by a
  non-symmetric operator."""
  from lanczosnet_amd import ops
  net, _ = _net(cfg, net_seed, general=general, name=name)
  ns, adj, mask = _graphs(rs, B, N, nmin, p)
  n = _t(ns)
  L = ops.laplacian_l4(_t(adj), n).clone()
  D, V = ops.lanczos_ritz(L[:, :, :, 0], n, K)
  mm = _t(mask[:, :, None] * mask[:, None, :]).float()
  if second in ('all', 'mixed'):
    _, adj2, _ = _graphs(np.random.RandomState(5), B, N, nmin, 0.05)
    sel = slice(None, None, 2 if second == 'mixed' else 1)
    L[sel, :, :, 1] = (ops.laplacian_l4(_t(adj2), n)[:, :, :, 0] * mm)[sel]
  elif second == 'nonsym':
    L[:, :, :, 1] = _t(rs.randn(B, N, N).astype(np.float32) * 0.1) * mm
    assert not torch.equal(L[..., 1], L[..., 1].transpose(1, 2))
  if general:
    X = _t(rs.randn(B, N, cfg['input_dim']).astype(np.float32) * mask[:, :, None])
  else:
    X = _t(rs.randint(0, cfg['num_atom'], size=(B, N)).astype(np.int64))
  label = _t(rs.randn(B, cfg['output_dim']).astype(np.float32))
  assert net._mid_hip_supported(N, K, L.shape[3])
  return net, X, L, D, V, _t(mask), label, ns


# ---- 1. the unmodified reference
def test_hip_backward_matches_the_reference_on_its_own_training_batch(launches):
  from graph_fixture import load_split, pad_batch
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  from test_gpu_train_paths import _check
  items, ref, seed, _ = load_split('train')
  _, X, mask, n = pad_batch(items)
  B, N = mask.shape
  L = np.zeros((B, N, N, 2), np.float32)
  L[..., 0] = ref['L0']
  L[..., 1] = ref['L0']
  net = LanczosNetGeneral(make_model_config(GRAPH_CFG, general=True))
  net.load_state_dict({k: torch.from_numpy(v) for k, v in
                       oracle.make_lanczosnet_params(GRAPH_CFG, seed, general=True).items()})
  net = _hip(net.to(DEV))
  _, loss = net(_t(X), _t(L), _t(ref['D']), _t(ref['V']), label=_t(ref['label']), mask=_t(mask))
  _check(net, loss, load_golden('train_paths.npz'), 'graph')
  assert _ran_hip() and len(launches) == 1


# ---- 2. other shapes against float64
# Two shapes of the forward's list are NOT here: (64, 100, K = 20, eight scales) and (70, 128, K = 32,
# [2, 5]).  On them the fp32 torch route itself misses the bar against float64 (3.9e-5 and 2.1e-5 /
# 2.4e-5 of |g|; the kernels 1.8e-5 and 1.4e-5 / 4.2e-4): with 6..7 million ReLU inputs one of them
# lies within fp32 rounding of zero, the fp32 and the float64 forward disagree on its sign, and ONE
# dropped element is 1 / sqrt(7e6) = 4e-4 of a tensor whose contributions add incoherently (DESIGN.md
# §4.9b).  The reference's configuration is held to the reference itself (above, and the runner loop);
# the full tile with K = 32 is here at a batch of six, and its 70-graph batch (two launches) in the
# bitwise test below.
@pytest.mark.parametrize('B,N,nmin,K,long_dist,din,second', [
    (5, 33, 33, 20, [1, 2, 3, 5, 7, 10, 20, 30], 10, None),     # just beyond the 32-node tile
    (6, 128, 90, 32, [2, 5], 10, None),                         # full tile, K = 32
    (9, 64, 40, 20, [], 16, None),                              # no long scales at all
    (12, 48, 34, 12, [1, 3, 7], 128, None),                     # input width 128
    (24, 96, 40, 20, DIST16[:9], 10, None),                     # nine long scales: MLP gradients by autograd
    (10, 70, 34, 32, DIST16, 10, None),                         # sixteen, K = 32
    (16, 80, 40, 20, [1, 2, 3, 5, 7, 10, 20, 30], 10, 'all'),   # two operator channels that differ
    (16, 80, 40, 20, [1, 2, 3, 5, 7, 10, 20, 30], 10, 'mixed'),  # folded and unfolded graphs in one batch
])
def test_hip_backward_matches_float64_autograd(B, N, nmin, K, long_dist, din, second, launches):
  rs = np.random.RandomState(B + N)
  cfg = dict(GRAPH_CFG, num_eig_vec=K, long_diffusion_dist=long_dist, input_dim=din)
  net, X, L, D, V, mask, label, _ = _batch(rs, cfg, B, N, nmin, K, second=second)
  _against_float64(net, X, L, D, V, mask, label, 'B=%d N=%d K=%d S=%d din=%d %s' % (B, N, K, len(long_dist), din, second), launches)


def test_hip_backward_of_the_embedding_model(launches):
  rs = np.random.RandomState(11)
  cfg = dict(oracle.DEFAULT_QM8_CFG, num_bond_type=1, **SMALL)
  net, X, L, D, V, mask, label, _ = _batch(rs, cfg, 20, 60, 40, cfg['num_eig_vec'], p=0.1, net_seed=2,
                                           general=False, name='LanczosNet')
  _against_float64(net, X, L, D, V, mask, label, 'embedding model', launches)
  assert net.embedding.weight.grad.abs().max() > 0


# ---- 3. a non-symmetric operator channel
def test_hip_backward_does_not_assume_a_symmetric_operator(launches):
  rs = np.random.RandomState(17)
  net, X, L, D, V, mask, label, _ = _batch(rs, dict(GRAPH_CFG), 12, 72, 40, 20, second='nonsym')
  _against_float64(net, X, L, D, V, mask, label, 'non-symmetric channel', launches)


# ---- 4. padding and batch independence, on the launches themselves
def _launches(net, X, L, V, G, mask, gscore):
  from lanczosnet_amd import ops
  mid = net._plan_mid_backward()['mid']
  X0 = torch.nn.functional.pad(X, (0, mid['din0p'] - X.shape[2])).contiguous()
  _, Xw = ops.midgraph_forward(X0, L, V, G, mask, mid['W'], mid['bias'], mid['Whead'], mid['bhead'],
                               net.num_layer, return_work=True)
  dOut = torch.empty_like(Xw)
  ops.midgraph_head_grad(Xw, mask, gscore, mid['Whead'], mid['bhead'], dOut)
  ops.midgraph_input_grad(dOut, Xw, L, V, G, mid['Wt'], X.shape[1], mid['din0p'])
  dG = ops.midgraph_project(dOut, Xw, X0, L, V, G, mid['W'])[3]
  return dOut, dG


def test_padding_and_batch_position_do_not_change_a_graphs_gradients():
  from lanczosnet_amd import ops
  rs = np.random.RandomState(23)
  B, N, K = 12, 80, 20
  net, X, L, D, V, mask, _, ns = _batch(rs, dict(GRAPH_CFG, **SMALL), B, N, 40, K)
  G = ops.spectral_gains(D, net.long_diffusion_dist, net.num_layer, net._plan_mid_backward()['mlp_pack'])
  gscore = _t(rs.randn(B, 2).astype(np.float32))
  with torch.no_grad():
    dOut, dG = _launches(net, X, L, V, G, mask, gscore)
    assert dOut.abs().max() > 0 and dG.abs().max() > 0
    for b in range(B):   # rows at or beyond the node count: exactly zero, in every layer
      assert not dOut[:, b, int(ns[b]):].any(), b
    # the same graphs padded to N = 96
    pad = 96 - N
    Fp = torch.nn.functional.pad
    dOut2, dG2 = _launches(net, Fp(X, (0, 0, 0, pad)), Fp(L, (0, 0, 0, pad, 0, pad)).contiguous(),
                           Fp(V, (0, 0, 0, pad)).contiguous(), G, Fp(mask, (0, pad)), gscore)
    assert torch.equal(dOut2[:, :, :N], dOut) and not dOut2[:, :, N:].any()
    assert torch.equal(dG2, dG)
    # ... and reversed, in a batch of 9 of them
    idx = torch.arange(B - 1, 2, -1, device=DEV)
    dOut3, dG3 = _launches(net, X[idx], L[idx].contiguous(), V[idx].contiguous(), G[:, idx].contiguous(),
                           mask[idx], gscore[idx])
    assert torch.equal(dOut3, dOut[:, idx]) and torch.equal(dG3, dG[:, idx])


def test_a_batch_beyond_the_resident_workgroups_goes_out_in_chunks_with_the_same_bits():
  """70 graphs on the full tile with K = 32 = 280 workgroups, more than the chip holds: consecutive
  launches.  Every graph's dOut and gain gradients equal those it gets in a batch of its own kind."""
  from lanczosnet_amd import ops
  rs = np.random.RandomState(198)
  B, N, K = 70, 128, 32
  cfg = dict(GRAPH_CFG, num_eig_vec=K, long_diffusion_dist=[2, 5])
  net, X, L, D, V, mask, _, ns = _batch(rs, cfg, B, N, 90, K)
  G = ops.spectral_gains(D, net.long_diffusion_dist, net.num_layer, net._plan_mid_backward()['mlp_pack'])
  gscore = _t(rs.randn(B, 2).astype(np.float32))
  with torch.no_grad():
    dOut, dG = _launches(net, X, L, V, G, mask, gscore)
    assert torch.isfinite(dOut).all() and dOut[0].abs().max() > 0 and dG.abs().max() > 0
    for lo, hi in ((0, 8), (60, 70)):
      d2, g2 = _launches(net, X[lo:hi], L[lo:hi], V[lo:hi], G[:, lo:hi].contiguous(), mask[lo:hi], gscore[lo:hi])
      assert torch.equal(d2, dOut[:, lo:hi]) and torch.equal(g2, dG[:, lo:hi]), lo


# ---- 5. bitwise repeatability
def test_two_identical_steps_give_the_same_bits(monkeypatch, launches):
  rs = np.random.RandomState(29)
  net, X, L, D, V, mask, label, _ = _batch(rs, dict(GRAPH_CFG), 64, 100, 20, 20)
  _hip(net)
  _, g1 = _step(net, X, L, D, V, mask, label)
  assert _ran_hip()
  _, g2 = _step(net, X, L, D, V, mask, label)
  monkeypatch.setenv('LNZ_MID_FENCED', '1')
  _, g3 = _step(net, X, L, D, V, mask, label)
  assert _ran_hip() and len(launches) == 3
  for k in g1:
    assert torch.equal(g1[k], g2[k]), k
    assert torch.equal(g1[k], g3[k]), k


# ---- 6. equal channels
def test_equal_operator_channels_get_equal_weight_gradients(launches):
  rs = np.random.RandomState(31)
  net, X, L, D, V, mask, label, _ = _batch(rs, dict(GRAPH_CFG, **SMALL), 10, 90, 40, 20)
  assert torch.equal(L[..., 0], L[..., 1])
  _hip(net)
  _step(net, X, L, D, V, mask, label)
  assert _ran_hip() and len(launches) == 1
  S = net.num_scale_long
  for t in range(net.num_layer):
    g = net.filter[t].weight.grad.view(128, S + 2, -1)
    assert g[:, S].abs().max() > 0 and torch.equal(g[:, S], g[:, S + 1]), t


# ---- 7. the reference runner's loop
def test_reference_graph_runner_loop_trains_through_the_hip_backward(tmp_path, monkeypatch):
  import pickle
  import os
  import oracle.graph_runner as restated
  import runner_harness as H
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset.graph_data import GraphData
  from lanczosnet_amd.model import LanczosNetGeneral
  from test_graph_runner_dropin import _splits, _write_pickles
  monkeypatch.setattr(LanczosNetGeneral, 'mid_backward_impl', 'hip')
  ran, real = [], ops.midgraph_input_grad

  def counted(*a, **kw):
    out = real(*a, **kw)
    ran.append(ops.last_kernel())
    return out
  monkeypatch.setattr(ops, 'midgraph_input_grad', counted)
  g = load_golden('runner_graph.npz')
  _write_pickles(str(tmp_path / 'data'), _splits(g))
  cfg = H.graph_config(str(tmp_path / 'data'), str(tmp_path / 'exp'), use_gpu=True,
                       max_epoch=int(g['max_epoch']))
  H.seed_like_run_exp(int(g['seed']))
  runner = restated.GraphRunner(cfg, dict(LanczosNetGeneral=LanczosNetGeneral, GraphData=GraphData))
  best = runner.train()
  stats = pickle.load(open(os.path.join(cfg.save_dir, 'train_stats.p'), 'rb'))
  tl, vl = np.asarray(stats['train_loss']), np.asarray(stats['val_loss'])
  rel = np.abs(tl - g['train_loss']) / np.abs(g['train_loss'])
  relv = np.abs(vl - g['val_loss']) / np.abs(g['val_loss'])
  print('graph runner, HIP backward: train-loss rel dev max %.2e (first %.2e, last %.2e); val MSE rel dev %.2e'
        % (rel.max(), rel[0], rel[-1], relv.max()))
  assert len(ran) == len(g['train_loss']) and all(k.startswith(KERNEL) for k in ran), ran
  assert tl.shape == g['train_loss'].shape and vl.shape == g['val_loss'].shape
  assert rel[0] < 1e-5
  assert rel.max() < 5e-4
  assert relv[0] < 1e-5 and relv.max() < 5e-4
  assert abs(best - float(g['best_val'])) < 5e-4 * float(g['best_val'])


# ---- 8. routing: everything else takes the torch route, bit for bit
@pytest.mark.parametrize('case', ['switch off', 'short scales', 'width 64', 'dropout', 'backward_impl torch',
                                  'N <= 32', 'N > 128'])
def test_outside_the_envelope_the_torch_route_is_taken_unchanged(case, launches):
  import warnings
  cfg = dict(GRAPH_CFG, **SMALL)
  B, N, nmin = 6, 60, 34
  if case == 'short scales':
    cfg['short_diffusion_dist'] = [1, 2]
  elif case == 'width 64':
    cfg['hidden_dim'] = [64] * 3
  elif case == 'N <= 32':
    N, nmin = 30, 12
  elif case == 'N > 128':
    N, nmin = 132, 100
  from lanczosnet_amd import ops
  rs = np.random.RandomState(37)
  ns, adj, mask = _graphs(rs, B, N, nmin, 0.3)
  n = _t(ns)
  L = ops.laplacian_l4(_t(adj), n)
  D, V = ops.lanczos_ritz(L[:, :, :, 0], n, 20)
  X = _t(rs.randn(B, N, 10).astype(np.float32) * mask[:, :, None])
  label, mask = _t(rs.randn(B, 2).astype(np.float32)), _t(mask)
  res = []
  for opted in (True, False):
    net, _ = _net(cfg, 3)
    net.train()
    if case == 'dropout':
      net.dropout = 0.3
    if opted:
      net.mid_backward_impl = 'torch' if case == 'switch off' else 'hip'
      if case == 'backward_impl torch':
        net.backward_impl = 'torch'
    with warnings.catch_warnings(), deterministic_dropout():
      warnings.simplefilter('ignore')
      res.append(_step(net, X, L, D, V, mask, label))
    assert not launches, case
  assert torch.equal(res[0][0], res[1][0])
  for k in res[0][1]:
    assert torch.equal(res[0][1][k], res[1][1][k]), (case, k)
