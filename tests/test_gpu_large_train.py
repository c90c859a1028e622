"""Training edge-list batches beyond 192 nodes through the opt-in HIP backward on the sparse image
(`_LargeSparseFusedFunction`; csrc/conv_sparse_grad.hip: lnz_large_grad_project, lnz_large_grad_spectral,
lnz_large_grad_input).  Every module test opts in (`large_backward_impl = 'hip'`) and reads
from `ops.last_kernel()` that the new input-gradient kernel ran.

Bars: the project's gradient bars (tests/gradproj.py) — loss within 1e-5, every
parameter tensor's norm and 16 fixed +-1 projections of its gradient within 1e-5 of |g| — against a
float64 restatement of `_torch_forward` with autograd, written here, on `L.to_dense()` (beyond 4096
nodes: on a float64 L built here from the edge list).

ReLU sign flips (tests/test_gpu_mid_train.py): with hundreds of thousands of ReLU inputs
one of them can lie within fp32 rounding of zero; the fp32 and the float64 forward then disagree on its
sign and NO fp32 implementation meets the bar.  So every case first holds the densify + autograd route —
the only route before this one existed — to the same truth, and asserts that IT meets 1e-5 on the
recorded seed (at most five seeds, 0 .. 4, were tried per case; the first that passed is the one in the
parametrisation).  Both routes' deviations are printed.

The kernels alone: integer cases on which the fp32 result must EQUAL float64 numpy (tests/large_train_fixture.py)."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import edge_graphs as eg
import large_train_fixture as F
import oracle
from gradproj import deterministic_dropout, project_torch
from graph_fixture import GRAPH_CFG

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KERNEL = 'large_grad_input_kernel'
EIGHT = [1, 2, 3, 5, 7, 10, 20, 30]     # config/graph_lanczos_net.yaml
SIXTEEN = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15, 20, 25, 30, 40, 50]
G, Q = 'LanczosNetGeneral', 'LanczosNet'


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@contextlib.contextmanager
def _no_densify():
  with warnings.catch_warnings():
    warnings.filterwarnings('error', message='.*densified.*')
    yield


@pytest.fixture(autouse=True)
def launches(monkeypatch):
  """Every call of ops.large_grad_input during a test (lnz_last_kernel() keeps the last note of a thread,
  which an earlier test may have left: the count shows that a step did NOT take the new route)."""
  from lanczosnet_amd import ops
  calls, real = [], ops.large_grad_input

  def counted(*a, **kw):
    calls.append(1)
    return real(*a, **kw)
  monkeypatch.setattr(ops, 'large_grad_input', counted)
  return calls


def _graphs(ns, seed, degree=6.0):
  rs = np.random.RandomState(1000 + seed)
  return [dict(n=int(n), edges=eg.gnp_edges(int(n), degree / n, rs)) for n in ns]


def _net(model, seed, K, long_dist, din, layers, **over):
  from lanczosnet_amd import model as M
  from lanczosnet_amd.utils.arg_helper import make_model_config
  general = model == G
  base = GRAPH_CFG if general else dict(oracle.DEFAULT_QM8_CFG, num_bond_type=1)
  cfg = dict(base, num_eig_vec=K, long_diffusion_dist=long_dist, hidden_dim=[128] * layers, num_layer=layers,
             spectral_filter_kind='MLP', short_diffusion_dist=[], **over)
  if din is not None:
    cfg['input_dim'] = din
  P = oracle.make_lanczosnet_params(cfg, 3 + seed, general=general)
  net = getattr(M, model)(make_model_config(cfg, general=general))
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  return net.to(DEV).train(), cfg


def _batch(graphs, K, din, seed, cfg=None, **collate):
  """The collate's batch of the graphs; for the embedding model (din None) node ids in place of features."""
  from lanczosnet_amd.dataset import collate_graph_edges
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    b = collate_graph_edges(collate.pop('items', None) or eg.items(graphs, dim=din or 4, seed=5 + seed), K,
                            device=DEV, **collate)
  if din is None:
    rs = np.random.RandomState(77 + seed)
    b['node_feat'] = _t(rs.randint(0, cfg['num_atom'], size=tuple(b['node_mask'].shape)).astype(np.int64))
    b['label'] = _t(rs.randn(b['node_mask'].shape[0], cfg['output_dim']).astype(np.float32))
  return b


def _grads(net):
  return {k: p.grad.clone() for k, p in net.named_parameters()}


def _step(net, b, L=None):
  net.zero_grad(set_to_none=True)
  _, loss = net(b['node_feat'], b['L'] if L is None else L, b['D'], b['V'], label=b['label'], mask=b['node_mask'])
  loss.backward()
  return loss.detach(), _grads(net)


def _hip_step(net, b, launches, n_launch):
  from lanczosnet_amd import ops
  net.large_backward_impl = 'hip'
  before = len(launches)
  with _no_densify():
    out = _step(net, b)
  assert ops.last_kernel().startswith(KERNEL), ops.last_kernel()
  assert len(launches) - before == n_launch
  return out


def _torch_step(net, b, launches):
  net.large_backward_impl = 'torch'
  before = len(launches)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    out = _step(net, b)
  assert len(launches) == before
  return out


def _truth(net, X, Ls, D, V, mask, label):
  """float64 restatement of `_torch_forward` (model/lanczos_net.py:143-199 of the reference) with autograd:
  loss and gradients by parameter name.  Ls: the operator channels, each [B,N,N] float64."""
  P = {k: v.detach().double().requires_grad_(True) for k, v in net.named_parameters()}
  B = V.shape[0]
  Vd = V.double()
  state = X.double() if net.general else P['embedding.weight'][X]
  S, nl = net.num_scale_long, net.num_layer
  pows = torch.stack([D.double() ** p for p in net.long_diffusion_dist], dim=2) if S else None
  for t in range(nl):
    W, bias = P['filter.%d.weight' % t], P['filter.%d.bias' % t]
    Wc = W.view(W.shape[0], -1, state.shape[2])
    out, c = bias.view(1, 1, -1), 0
    if S:
      Gn = pows
      if net._has_mlp():
        h = pows.reshape(-1, S)
        for i in (0, 2, 4, 6):
          h = h @ P['spectral_filter.%d.%d.weight' % (t, i)].t() + P['spectral_filter.%d.%d.bias' % (t, i)]
          h = torch.relu(h) if i < 6 else h
        Gn = h.view(B, -1, S)
      Y = Vd.transpose(1, 2) @ state
      for s in range(S):
        out = out + Vd @ (Gn[:, :, s:s + 1] * (Y @ Wc[:, c].t()))
        c += 1
    for Lc in Ls:
      out = out + Lc @ (state @ Wc[:, c].t())
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
    t = truth[k].double()
    nrm = float(t.norm())
    if nrm == 0.0:
      assert float(grads[k].abs().max()) == 0.0, k
      continue
    e = max(float(np.abs(project_torch(grads[k].double() - t, i)).max()) / nrm,
            abs(float(grads[k].double().norm()) - nrm) / nrm)
    if e >= worst[0]:
      worst = (e, k)
  return worst


def _ragged(N, B):
  return [N] + [N - 57 + 13 * b for b in range(B - 1)]


# B, N, node counts, K, long scales, input width (None: the embedding model's), layers, model, seed
CASES = {
    'N193 the first K-step size': (3, 193, [193, 193, 193], 20, EIGHT, 10, 2, G, 0),
    'B10 N257 one row in the second chunk': (10, 257, [257] + [200 + 6 * i for i in range(9)], 20, EIGHT, 10, 2, G, 0),
    'K64 S1 width 128': (3, 300, [300, 193, 262], 64, [1], 128, 2, G, 0),
    'K17 S16 width 127': (3, 257, _ragged(257, 3), 17, SIXTEEN, 127, 2, G, 1),   # (seed 0: the torch route 3.2e-3)
    'no long scales': (3, 257, _ragged(257, 3), 20, [], 10, 2, G, 0),
    'seven layers': (3, 257, _ragged(257, 3), 20, EIGHT, 10, 7, G, 0),
    'embedding model': (3, 257, _ragged(257, 3), 20, EIGHT, None, 2, Q, 0),
}


def _case(name, seed=None):
  B, N, ns, K, long_dist, din, layers, model, recorded = CASES[name]
  seed = recorded if seed is None else seed
  assert len(ns) == B and max(ns) == N
  graphs = _graphs(ns, seed)
  assert eg.max_row_entries(graphs) <= eg.conv_cap(N)
  net, cfg = _net(model, seed, K, long_dist, din, layers)
  b = _batch(graphs, K, din, seed, cfg)
  return net, b, graphs


# ---- 1. against float64 autograd ---------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_hip_backward_matches_float64_autograd(name, launches):
  from lanczosnet_amd import ops
  net, b, _ = _case(name)
  L = b['L']
  assert isinstance(L, ops.SparseLaplacian) and L.images is None and int(L.image.flags.item()) == 0
  Ld = L.to_dense().double()
  assert torch.equal(Ld[..., 0], Ld[..., 1]) and torch.equal(Ld[..., 0], Ld[..., 0].transpose(1, 2))
  loss64, truth = _truth(net, b['node_feat'], [Ld[..., 0], Ld[..., 1]], b['D'], b['V'], b['node_mask'], b['label'])
  loss_t, g_t = _torch_step(net, b, launches)
  n_launch = net.num_layer - (1 if net.general else 0)
  loss, g = _hip_step(net, b, launches, n_launch)
  e_hip, e_torch = _deviation(g, truth), _deviation(g_t, truth)
  print('%s: gradients vs float64 autograd, worst of |g|: HIP %.2e (%s), torch route %.2e (%s); loss %.2e / %.2e'
        % (name, e_hip[0], e_hip[1], e_torch[0], e_torch[1], abs(float(loss) - float(loss64)) / float(loss64),
           abs(float(loss_t) - float(loss64)) / float(loss64)))
  assert e_torch[0] < 1e-5, ('the seed: the densify + autograd route itself misses the bar here', e_torch)
  assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
  assert e_hip[0] < 1e-5, e_hip
  # both edge-channel blocks of every mix weight get the same gradient
  S = net.num_scale_long
  for t in range(net.num_layer):
    gw = g['filter.%d.weight' % t].view(128, S + 2, -1)
    assert gw[:, S].abs().max() > 0 and torch.equal(gw[:, S], gw[:, S + 1]), t
  if not net.general:
    assert g['embedding.weight'].abs().max() > 0


def test_the_training_score_is_the_inference_score_bit_for_bit(launches):
  """One graph-sized chunk pair of the forward's projection (N <= 256: two partial sums, whose float atomics
  commute): the same launches on the same operands give the same bits."""
  net, b, _ = _case('N193 the first K-step size')
  net.large_backward_impl = 'hip'
  with _no_densify():
    score = net(b['node_feat'], b['L'], b['D'], b['V'], mask=b['node_mask'])
    assert score.requires_grad and score.grad_fn is not None
    with torch.no_grad():
      ref = net(b['node_feat'], b['L'], b['D'], b['V'], mask=b['node_mask'])
  assert net._large_sparse_state[torch.device(DEV).index]['image_from'] == 'edges'
  assert torch.equal(score.detach(), ref)


# ---- 2. what the parent cannot do -------------------------------------------------------------------------
def test_no_dense_operator_is_allocated(launches):
  """B 2, N 2100 (wide by size), two layers.  The step holds the layer states [2,B,N,128] and works on a
  handful of buffers of one state's size; the bound is 4 x (states + image bytes).  One dense [B,N,N,2]
  fp32 tensor is 70 MB, and the densify route holds two.  Measured on the SECOND step: the first one
  also allocates the GEMM library's workspace (tens of MB, once per process and stream)."""
  N = 2100
  graphs = _graphs([N, N - 49], 0)
  assert eg.max_row_entries(graphs) <= eg.conv_cap(N)
  net, cfg = _net(G, 0, 8, EIGHT, 10, 2)
  b = _batch(graphs, 8, 10, 0)
  _hip_step(net, b, launches, 1)
  img = b['L'].image
  B = len(graphs)
  states = net.num_layer * B * N * 128 * 4
  image = sum(t.numel() * t.element_size() for t in (img.entries, img.values, img.counts))
  bound = 4 * (states + image)
  assert bound < B * N * N * 2 * 4 / 2
  net.large_backward_impl = 'hip'
  net.zero_grad(set_to_none=True)
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    loss, _ = _hip_step(net, b, launches, 1)
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - before
  print('peak allocation of one step: %.1f MB (states %.1f MB, image %.1f MB, bound %.1f MB; a dense L: %.1f MB)'
        % (peak / 1e6, states / 1e6, image / 1e6, bound / 1e6, B * N * N * 8 / 1e6))
  assert not [w for w in rec if issubclass(w.category, UserWarning) and 'densified' in str(w.message)]
  assert torch.isfinite(loss) and peak < bound


def _dense_l4_float64(graphs, N):
  """[B,N,N] float64 on the device: L4 = D^-1/2 (I + A) D^-1/2 of every graph, from its edge list."""
  L = torch.zeros((len(graphs), N, N), dtype=torch.float64, device=DEV)
  for bi, g in enumerate(graphs):
    n = g['n']
    s = _t(1.0 / np.sqrt(eg.row_entries(g).astype(np.float64)))
    u, v = _t(g['edges'][:, 0].astype(np.int64)), _t(g['edges'][:, 1].astype(np.int64))
    L[bi, u, v] = s[u] * s[v]
    L[bi, v, u] = s[u] * s[v]
    i = torch.arange(n, device=DEV)
    L[bi, i, i] = s * s
  return L


def test_training_beyond_the_dense_limit(launches):
  """B 2, N 4104: past `to_dense`'s 4096 nodes and into 16-bit columns beyond 4095.  One optimizer step, and the
  gradients against float64 autograd on a dense L built here from the edges (270 MB)."""
  from lanczosnet_amd import ops
  N, K = 4104, 20
  graphs = _graphs([N, N - 9], 0)
  assert eg.max_row_entries(graphs) <= eg.conv_cap(N)
  net, cfg = _net(G, 0, K, EIGHT, 10, 2)
  b = _batch(graphs, K, 10, 0)
  assert isinstance(b['L'], ops.SparseLaplacian) and int(b['L'].image.flags.item()) == 0
  opt = torch.optim.Adam(net.parameters(), lr=1e-3)
  before = {k: p.detach().clone() for k, p in net.named_parameters()}
  loss, g = _hip_step(net, b, launches, 1)
  assert torch.isfinite(loss) and all(torch.isfinite(x).all() for x in g.values())
  L64 = _dense_l4_float64(graphs, N)
  loss64, truth = _truth(net, b['node_feat'], [L64, L64], b['D'], b['V'], b['node_mask'], b['label'])
  del L64
  e = _deviation(g, truth)
  print('N = 4104: gradients vs float64 autograd, worst of |g|: %.2e (%s); loss %.2e'
        % (e[0], e[1], abs(float(loss) - float(loss64)) / float(loss64)))
  assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
  assert e[0] < 1e-5, e
  opt.step()
  assert any(not torch.equal(p.detach(), before[k]) for k, p in net.named_parameters())
  with torch.no_grad(), _no_densify():
    _, loss2 = net(b['node_feat'], b['L'], b['D'], b['V'], label=b['label'], mask=b['node_mask'])
  assert torch.isfinite(loss2)


# ---- 3. properties -------------------------------------------------------------------------------------------
def test_two_identical_steps_give_the_same_bits(launches):
  """(N <= 256: the forward's projection adds two partial sums per graph with float atomics, which commute;
  with three or more the FORWARD's states differ in the last bit between runs — csrc/conv_large.hip,
  tests/test_gpu_edge_collate.py.  The backward launches themselves: the ops-level test below, N = 300.)"""
  ns = [250, 201, 233]
  net, cfg = _net(G, 1, 20, EIGHT, 10, 3)
  b = _batch(_graphs(ns, 1), 20, 10, 1)
  l1, g1 = _hip_step(net, b, launches, 2)
  l2, g2 = _hip_step(net, b, launches, 2)
  assert torch.equal(l1, l2)
  for k in g1:
    assert torch.equal(g1[k], g2[k]), k


def test_a_graphs_gradients_do_not_depend_on_batch_position_or_padding(launches):
  """The same 193-node graph alone (N = 193) and as graph 2 of three padded to 257, with a one-hot grad_score:
  the same parameter gradients.  Two fp32 evaluations of one sum in different tilings (the library GEMMs
  split their rows by the batch's size): held to the gradient bar, 1e-5 of |g|, against each other."""
  from lanczosnet_amd import ops
  g193 = _graphs([193], 2)[0]
  others = _graphs([257, 220], 3)
  net, cfg = _net(G, 2, 20, EIGHT, 10, 2)
  net.large_backward_impl = 'hip'
  alone = _batch([g193], 20, 10, 2)
  its = eg.items(others, dim=10, seed=9) + eg.items([g193], dim=10, seed=7)
  batch = _batch(None, 20, 10, 2, items=its)
  # the graph's own features and Ritz pairs, padded
  pad = 257 - 193
  Fp = torch.nn.functional.pad
  batch['node_feat'][2] = Fp(alone['node_feat'][0], (0, 0, 0, pad))
  batch['D'][2] = alone['D'][0]
  batch['V'][2] = Fp(alone['V'][0], (0, 0, 0, pad))
  res = []
  for bt, row in ((alone, 0), (batch, 2)):
    net.zero_grad(set_to_none=True)
    with _no_densify():
      score = net(bt['node_feat'], bt['L'], bt['D'], bt['V'], mask=bt['node_mask'])
    gs = torch.zeros_like(score)
    gs[row, 1] = 1.0
    score.backward(gs)
    assert ops.last_kernel().startswith(KERNEL)
    res.append((score[row].detach().clone(), _grads(net)))
  assert len(launches) == 2
  assert float((res[0][0] - res[1][0]).abs().max()) <= 1e-5 * float(res[0][0].abs().max())
  e = _deviation(res[1][1], res[0][1])
  print('alone vs in a padded batch: worst deviation %.2e of |g| (%s)' % e)
  assert e[0] < 1e-5, e


# ---- 4. the kernels alone: integer cases, fp32 == float64 ------------------------------------------------------
@pytest.mark.parametrize('shape', F.GRAD_SHAPES)
def test_grad_project_equals_float64(shape):
  from lanczosnet_amd import ops
  c = F.project_case(*shape)
  outs = []
  for key in ('dX', 'dX_clean', 'dX'):
    dX = _t(c[key])
    A, db = ops.large_grad_project(dX, _t(c['Xout']), _t(c['V']), _t(c['n']))
    outs.append((dX, A, db))
  dX, A, db = outs[0]
  assert np.array_equal(dX.cpu().numpy().astype(np.float64), c['dP'])
  assert np.array_equal(A.cpu().numpy().astype(np.float64), c['A'])
  assert np.array_equal(db.cpu().numpy().astype(np.float64), c['db'])
  # garbage (NaN, 3e38) in the rows at or beyond n_nodes changes nothing; a second call gives the same bits
  for other in outs[1:]:
    for x, y in zip(outs[0], other):
      assert torch.equal(x, y)
  # no node counts: every row is live
  full = _t(c['dX_clean'])
  A2, db2 = ops.large_grad_project(full, _t(c['Xout']), _t(c['V']), None)
  assert torch.equal(A2, A) and torch.equal(db2, db) and torch.equal(full, dX)


@pytest.mark.parametrize('shape', F.GRAD_SHAPES)
def test_grad_spectral_equals_float64(shape):
  from lanczosnet_amd import ops
  B, N, K, S, d = shape
  c = F.spectral_case(*shape)
  dG, Q, dY = ops.large_grad_spectral(_t(c['A']), _t(c['Y']), _t(c['G']), _t(c['W']), d)
  assert tuple(dG.shape) == (B, K, S) and tuple(Q.shape) == (B, K, S, d) and tuple(dY.shape) == (B, K, 128)
  assert np.array_equal(dG.cpu().numpy().astype(np.float64), c['dG'])
  assert np.array_equal(Q.cpu().numpy().astype(np.float64), c['Q'])
  assert np.array_equal(dY.cpu().numpy().astype(np.float64), c['dY'])
  none, Q2, dY2 = ops.large_grad_spectral(_t(c['A']), _t(c['Y']), _t(c['G']), _t(c['W']), d, want_dgains=False)
  assert none is None and torch.equal(Q2, Q) and torch.equal(dY2, dY)


@pytest.mark.parametrize('shape', F.GRAD_SHAPES)
def test_grad_input_equals_float64(shape):
  from lanczosnet_amd import ops
  B, N, K, S, d = shape
  c = F.input_case(*shape)
  out = torch.full((B, N, 128), float('nan'), device=DEV)
  got = ops.large_grad_input(_t(c['dZ']), _t(c['Wn']), _t(c['V']), _t(c['dY']), d, out=out)
  assert got is out and ops.last_kernel().startswith(KERNEL)
  assert np.array_equal(out.cpu().numpy().astype(np.float64), c['dX'])
  # no long scales: the node-space term alone
  out2 = torch.full((B, N, 128), float('nan'), device=DEV)
  ops.large_grad_input(_t(c['dZ']), _t(c['Wn']), None, None, d, out=out2)
  ref = np.zeros((B, N, 128))
  ref[..., :d] = (c['dZ'].astype(np.float64) @ c['Wn'].astype(np.float64))[..., :d]
  assert np.array_equal(out2.cpu().numpy().astype(np.float64), ref)


def test_backward_launches_repeat_their_bits_beyond_one_chunk():
  """Real-valued operands at N = 300 (two chunks of the projection, five row tiles of the input gradient)."""
  from lanczosnet_amd import ops
  rs = np.random.RandomState(5)
  B, N, K, S, d = 5, 300, 20, 8, 128
  g, x = _t(rs.randn(B, N, 128).astype(np.float32)), _t(rs.randn(B, N, 128).astype(np.float32))
  V = _t((rs.randn(B, N, K) / np.sqrt(N)).astype(np.float32))
  W = _t((rs.randn(128, (S + 2) * d) * 0.05).astype(np.float32))
  Gn = _t(rs.randn(B, S, K).astype(np.float32))
  runs = []
  for _ in range(2):
    dP = g.clone()
    A, db = ops.large_grad_project(dP, x, V, None)
    Y = torch.bmm(V.transpose(1, 2), x)
    dG, Qm, dY = ops.large_grad_spectral(A, Y, Gn, W, d)
    out = ops.large_grad_input(dP, W[:, :128].contiguous(), V, dY, d, out=torch.empty_like(dP))
    runs.append((dP, A, db, dG, Qm, dY, out))
  for a, b_ in zip(*runs):
    assert torch.isfinite(a).all() and torch.equal(a, b_)
  # ... and agree with float64 (fp32 accumulation over at most 300 rows / 192 columns: 1e-5 of the largest entry)
  dP64 = (g.double() * (x > 0))
  A64 = V.double().transpose(1, 2) @ dP64
  assert float((runs[0][1].double() - A64).abs().max()) < 1e-5 * float(A64.abs().max())
  dX64 = dP64 @ W[:, :128].double() + V.double() @ runs[0][5].double()
  assert float((runs[0][6].double() - dX64).abs().max()) < 1e-5 * float(dX64.abs().max())


# ---- 5. the envelope: everything else takes today's route, bit for bit ------------------------------------------
@pytest.mark.parametrize('case', ['typed batch', 'dense L', 'dropout', 'switch off', 'bf16 mode', 'raised image flag'])
def test_outside_the_envelope_the_torch_route_is_taken_unchanged(case, launches):
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_adjacency
  K = 20
  over, L = {}, None
  if case == 'raised image flag':
    graphs, N = eg.star_case()
    assert eg.max_row_entries(graphs) > ops.large_sparse_row_cap(N)
  else:
    graphs = _graphs([257, 230, 201], 4)
  if case == 'typed batch':
    rs = np.random.RandomState(102)
    its = [dict(it, edge_type=rs.randint(0, 2, size=g['edges'].shape[0])) for it, g in
           zip(eg.items(graphs, dim=10, seed=9), graphs)]
    over = dict(num_bond_type=2)
    b = _batch(None, K, 10, 4, items=its, num_edge_type=2)
    assert b['L'].images is not None and b['L'].channels == 3
  else:
    b = _batch(graphs, K, 10, 4)
    assert isinstance(b['L'], ops.SparseLaplacian)
  if case == 'dense L':
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      L = collate_graph_adjacency(eg.items(graphs, dim=10, seed=9, dense=True), K, device=DEV)['L']
    assert isinstance(L, torch.Tensor)
  if case == 'raised image flag':
    assert int(b['L'].image.flags.item()) != 0
  res = []
  for opted in (True, False):
    net, _ = _net(G, 4, K, EIGHT, 10, 2, **over)
    if case == 'dropout':
      net.dropout = 0.3
    if case == 'bf16 mode':
      net.gemm_mode = 'bf16'
    net.large_backward_impl = 'hip' if opted and case != 'switch off' else 'torch'
    seen = []
    route = net._route
    net._route = lambda *a, **kw: seen.append(route(*a, **kw)) or seen[-1]
    with warnings.catch_warnings(), deterministic_dropout():
      warnings.simplefilter('ignore')
      res.append(_step(net, b, L))
    assert seen == ['torch'] and not launches, (case, seen)
  assert torch.equal(res[0][0], res[1][0])
  for k in res[0][1]:
    assert torch.equal(res[0][1][k], res[1][1][k]), (case, k)
