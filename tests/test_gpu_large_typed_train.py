"""Training TYPED edge-list batches (two or more edge types: R = E + 1 = 3 .. 8 distinct operators, one sparse
image each) through the opt-in HIP backward (`_LargeSparseFusedFunction` on R operators; lnz_large_sparse_conv_split_f32 in
csrc/conv_sparse.hip, lnz_large_grad_input_channels in csrc/conv_sparse_grad.hip).  Every module
test opts in (`large_typed_backward_impl = 'hip'`), turns the 'densified' warning into an error, patches
`SparseLaplacian.to_dense` to raise during the step and reads from `ops.last_kernel()` that the new
input-gradient kernel ran.

Bars: the project's gradient bars (tests/gradproj.py) — loss within 1e-5, every parameter
tensor's norm and 16 fixed +-1 projections of its gradient within 1e-5 of |g| — against float64 autograd over
the float64 restatement of the reference forward (tests/test_gpu_large_train.py's `_truth`, restated here) on the
R channels of `L.to_dense()` (beyond its limit: on float64 per-channel L4 matrices built from the edges).

ReLU sign flips (tests/test_gpu_large_train.py): every case first holds the densify + autograd route — the only
route before this one — to the same truth and asserts that IT meets 1e-5 on the recorded seed (seeds 0 .. 4
were tried in order; the first on which that route passed is the one in the parametrisation).  Both routes'
deviations are printed.

The kernels alone: the split gather against the unchanged one-operator gather, bit for bit; the input gradient
on integer cases on which the fp32 result must EQUAL float64 numpy (tests/large_typed_train_fixture.py)."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import edge_graphs as eg
import large_typed_train_fixture as F
import oracle
from gradproj import deterministic_dropout, project_torch
from graph_fixture import GRAPH_CFG

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KERNEL = 'large_grad_input_channels_kernel'
ROUTE = 'large_typed_train_hip'
EIGHT = [1, 2, 3, 5, 7, 10, 20, 30]     # config/graph_lanczos_net.yaml
SIXTEEN = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15, 20, 25, 30, 40, 50]
G, Q = 'LanczosNetGeneral', 'LanczosNet'


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@contextlib.contextmanager
def _no_dense(monkeypatch):
  """No 'densified' warning and no dense L: `SparseLaplacian.to_dense` raises inside."""
  from lanczosnet_amd import ops

  def refuse(self):
    raise AssertionError('SparseLaplacian.to_dense was called during the step')
  with warnings.catch_warnings(), monkeypatch.context() as mp:
    warnings.filterwarnings('error', message='.*densified.*')
    mp.setattr(ops.SparseLaplacian, 'to_dense', refuse)
    yield


@pytest.fixture(autouse=True)
def launches(monkeypatch):
  """Every call of ops.large_grad_input_channels ('typed') and of ops.large_grad_input ('untyped') during a
  test: lnz_last_kernel() keeps a thread's last note, which an earlier test may have left — the counts show
  which route a step took."""
  from lanczosnet_amd import ops
  calls = dict(typed=0, untyped=0)
  real_t, real_u = ops.large_grad_input_channels, ops.large_grad_input

  def typed(*a, **kw):
    calls['typed'] += 1
    return real_t(*a, **kw)

  def untyped(*a, **kw):
    calls['untyped'] += 1
    return real_u(*a, **kw)
  monkeypatch.setattr(ops, 'large_grad_input_channels', typed)
  monkeypatch.setattr(ops, 'large_grad_input', untyped)
  return calls


def _graphs(ns, seed, E, degree=6.0):
  rs = np.random.RandomState(1000 + seed)
  graphs = [dict(n=int(n), edges=eg.gnp_edges(int(n), degree / n, rs)) for n in ns]
  return F.with_types(graphs, E, 2000 + seed)


def _net(model, seed, K, long_dist, din, layers, E, **over):
  from lanczosnet_amd import model as M
  from lanczosnet_amd.utils.arg_helper import make_model_config
  general = model == G
  base = GRAPH_CFG if general else oracle.DEFAULT_QM8_CFG
  cfg = dict(base, num_eig_vec=K, long_diffusion_dist=long_dist, hidden_dim=[128] * layers, num_layer=layers,
             spectral_filter_kind='MLP', short_diffusion_dist=[], num_bond_type=E, **over)
  if din is not None:
    cfg['input_dim'] = din
  P = oracle.make_lanczosnet_params(cfg, 3 + seed, general=general)
  net = getattr(M, model)(make_model_config(cfg, general=general))
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV).train()
  net.large_backward_impl = 'torch'
  return net, cfg


def _items(graphs, dim, seed):
  return [dict(it, edge_type=g['edge_type']) for it, g in zip(eg.items(graphs, dim=dim, seed=seed), graphs)]


def _batch(graphs, K, din, seed, E, cfg=None, items=None):
  """The collate's typed batch of the graphs; for the embedding model (din None) node ids in place of features."""
  from lanczosnet_amd.dataset import collate_graph_edges
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    b = collate_graph_edges(items or _items(graphs, din or 4, 5 + seed), K, device=DEV, num_edge_type=E)
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


def _hip_step(net, b, launches, monkeypatch):
  from lanczosnet_amd import ops
  net.large_typed_backward_impl = 'hip'
  before = dict(launches)
  with _no_dense(monkeypatch):
    out = _step(net, b)
  assert ops.last_kernel().startswith(KERNEL), ops.last_kernel()
  assert launches['typed'] - before['typed'] == net.num_layer - (1 if net.general else 0)
  assert launches['untyped'] == before['untyped'] == 0
  return out


def _torch_step(net, b, launches):
  net.large_typed_backward_impl = 'torch'
  before = dict(launches)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    out = _step(net, b)
  assert launches == before
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
    assert c == Wc.shape[1]
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


# B, N, node counts, E, K, long scales, input width (None: the embedding model's), layers, model, seed
CASES = {
    'N193 E2 K20 S8 width 10': (3, 193, [193, 193, 193], 2, 20, EIGHT, 10, 2, G, 0),
    'N257 ragged E7 K17 S16 width 127': (3, 257, _ragged(257, 3), 7, 17, SIXTEEN, 127, 2, G, 0),
    'N300 E3 K64 S1 width 128': (3, 300, [300, 193, 262], 3, 64, [1], 128, 2, G, 0),
    'no long scales': (3, 257, _ragged(257, 3), 2, 20, [], 10, 2, G, 0),
    'seven layers': (3, 257, _ragged(257, 3), 2, 20, EIGHT, 10, 7, G, 0),
    'embedding model': (3, 257, _ragged(257, 3), 2, 20, EIGHT, None, 2, Q, 0),
}


def _case(name, seed=None):
  B, N, ns, E, K, long_dist, din, layers, model, recorded = CASES[name]
  seed = recorded if seed is None else seed
  assert len(ns) == B and max(ns) == N
  graphs = _graphs(ns, seed, E)
  assert eg.max_row_entries(graphs) <= eg.conv_cap(N)
  net, cfg = _net(model, seed, K, long_dist, din, layers, E)
  b = _batch(graphs, K, din, seed, E, cfg)
  return net, b, graphs, E


# ---- 1. the kernels alone ------------------------------------------------------------------------------------
_GATHER = {}


def _gather_batch(name):
  """The typed batch of a gather case, its source P and the R one-operator references — built once."""
  if name not in _GATHER:
    from lanczosnet_amd import ops
    graphs, N, E = F.gather_case(name)
    edges, off, n, et = F.pack_typed(graphs)
    L = ops.sparse_laplacian_from_edges(_t(edges), _t(off), _t(n), N, edge_type=_t(et), num_edge_type=E)
    imgs = L.images
    assert imgs is not None and imgs.R == E + 1 and int(imgs.flags.item()) == 0
    B = len(graphs)
    rs = np.random.RandomState(41 + E + N)
    P = rs.randn(B, N, 128).astype(np.float32) * (np.arange(N)[None, :, None] < n[:, None, None])
    P = _t(P)
    refs = []
    for c in range(E + 1):
      im = imgs.channel(c)
      ref = torch.zeros((B, N, 128), dtype=torch.float32, device=DEV)
      ops._abi().large_sparse_conv_f32(im.entries, im.values, im.counts, im.cap, P, B, N, 0, ref)
      refs.append(ref)
    _GATHER[name] = (imgs, P, torch.stack(refs), graphs, E)
  return _GATHER[name]


@pytest.mark.parametrize('name', F.GATHER_CASES)
def test_split_gather_is_the_one_operator_gather_per_channel(name):
  from lanczosnet_amd import ops
  imgs, P, refs, graphs, E = _gather_batch(name)
  R, B, N = imgs.R, imgs.B, imgs.N
  out = torch.full((R, B, N, 128), float('nan'), device=DEV)
  keep = P.clone()
  got = ops.large_sparse_conv_split(imgs, P, out=out)
  assert got is out and ops.last_kernel() == 'sparse_conv_split_f32_kernel', ops.last_kernel()
  assert torch.equal(P, keep)
  assert torch.isfinite(out).all()
  for c in range(R):
    assert torch.equal(out[c], refs[c]), (name, c)
    assert float(refs[c].abs().max()) > 0
  # the channels are different operators, and the typed ones do not add up to channel 0 (own degrees)
  assert not torch.equal(out[0], out[1]) and not torch.equal(out[1], out[2])
  # the counts the schedule meets
  counts = imgs.counts.cpu().numpy()
  for b, g in enumerate(graphs):
    assert np.array_equal(counts[:, b, :g['n']], F.channel_row_entries(g, E)), (name, b)
  # a second call, allocating its own result: the same bits
  again = ops.large_sparse_conv_split(imgs, P)
  assert torch.equal(again, out)


@pytest.mark.parametrize('shape', F.INPUT_SHAPES)
def test_grad_input_channels_equals_float64(shape):
  from lanczosnet_amd import ops
  B, N, K, R, d = shape
  c = F.input_channels_case(*shape)
  opt = lambda x: None if x is None else _t(x)   # noqa: E731
  out = torch.full((B, N, 128), float('nan'), device=DEV)
  got = ops.large_grad_input_channels(_t(c['dZ']), _t(c['Wn']), opt(c['V']), opt(c['dY']), d, out=out)
  assert got is out and ops.last_kernel().startswith(KERNEL)
  res = out.cpu().numpy().astype(np.float64)
  assert np.array_equal(res, c['dX'])
  assert (res[..., d:] == 0).all()


def _real_input_operands(B, N, K, d):
  """Real-valued (dZ [3,B,N,128], Wn [3,128,128] with columns >= d zero, V, dY) from RandomState(6), on the device."""
  rs = np.random.RandomState(6)
  dZ = _t(rs.randn(3, B, N, 128).astype(np.float32))
  Wn = (rs.randn(3, 128, 128) * 0.05).astype(np.float32)
  Wn[:, :, d:] = 0.0
  V = _t((rs.randn(B, N, K) / np.sqrt(N)).astype(np.float32))
  dY = _t(rs.randn(B, K, 128).astype(np.float32))
  return dZ, _t(Wn), V, dY


# the one-operator kernel that lnz_large_grad_input launched before it became the R = 1 of the channels kernel:
# its output on the MI355X for `_real_input_operands`' channel 0 — key: (B, N, K, d)
PARENT_GOLDEN = {'k20_d128': (2, 65, 20, 128),    # one full 64-row tile and one row of a second; K a multiple of 4
                 'k17_d127': (2, 65, 17, 127)}    # K padded to 20, a partial last column tile


def test_grad_input_channels_with_one_channel_is_grad_input_bit_for_bit(launches):
  """Both dX entries at R = 1 reproduce, bit for bit, what the retired one-operator kernel gave for the same
  real-valued operands (tests/golden/large_grad_input_parent.npz); and two calls at R = 3 (B 5, N 300, K 20,
  d 128) give the same bits."""
  import os
  from lanczosnet_amd import ops
  golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'large_grad_input_parent.npz'))
  assert sorted(golden.files) == sorted(PARENT_GOLDEN)
  for key, (B, N, K, d) in PARENT_GOLDEN.items():
    dZ, Wn, V, dY = _real_input_operands(B, N, K, d)
    want = _t(golden[key])
    assert want.dtype == torch.float32 and tuple(want.shape) == (B, N, 128) and float(want.abs().max()) > 0
    one = ops.large_grad_input_channels(dZ[:1], Wn[:1], V, dY, d,
                                        out=torch.full((B, N, 128), float('nan'), device=DEV))
    assert ops.last_kernel() == 'large_grad_input_channels_kernel'
    ref = ops.large_grad_input(dZ[0], Wn[0], V, dY, d, out=torch.full((B, N, 128), float('nan'), device=DEV))
    assert ops.last_kernel() == 'large_grad_input_kernel'
    assert torch.equal(one, want) and torch.equal(ref, want), key
    assert torch.isfinite(one).all() and (one[..., d:] == 0).all()
  B, N, K, d = 5, 300, 20, 128
  dZ, Wn, V, dY = _real_input_operands(B, N, K, d)
  one = ops.large_grad_input_channels(dZ[:1], Wn[:1], V, dY, d, out=torch.full((B, N, 128), float('nan'), device=DEV))
  runs = [ops.large_grad_input_channels(dZ, Wn, V, dY, d, out=torch.full((B, N, 128), float('nan'), device=DEV))
          for _ in range(2)]
  assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], one)
  # ... and agree with float64 (fp32 accumulation over 3 x 128 + 20 terms: 1e-5 of the largest entry)
  dX64 = torch.einsum('cbno,coi->bni', dZ.double(), Wn.double()) + V.double() @ dY.double()
  assert float((runs[0].double() - dX64).abs().max()) < 1e-5 * float(dX64.abs().max())


# ---- 2. against float64 autograd -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_hip_backward_matches_float64_autograd(name, launches, monkeypatch):
  from lanczosnet_amd import ops
  net, b, graphs, E = _case(name)
  L = b['L']
  R = E + 1
  assert isinstance(L, ops.SparseLaplacian) and L.images is not None and L.channels == R
  assert int(L.images.flags.item()) == 0
  Ld = L.to_dense().double()
  assert tuple(Ld.shape) == (L.B, L.N, L.N, R)
  Ls = [Ld[..., c] for c in range(R)]
  for c in range(R):
    assert torch.equal(Ls[c], Ls[c].transpose(1, 2))
  assert not torch.equal(Ls[0], Ls[1])
  # the float64 operators built from the edges are those operators
  L64 = _t(np.stack([F.l4_channels_float64(g, E, L.N) for g in graphs]))            # [B,R,N,N]
  assert float((L64.permute(0, 2, 3, 1) - Ld).abs().max()) < 1e-6
  loss64, truth = _truth(net, b['node_feat'], Ls, b['D'], b['V'], b['node_mask'], b['label'])
  loss_t, g_t = _torch_step(net, b, launches)
  loss, g = _hip_step(net, b, launches, monkeypatch)
  e_hip, e_torch = _deviation(g, truth), _deviation(g_t, truth)
  print('%s: gradients vs float64 autograd, worst of |g|: HIP %.2e (%s), torch route %.2e (%s); loss %.2e / %.2e'
        % (name, e_hip[0], e_hip[1], e_torch[0], e_torch[1], abs(float(loss) - float(loss64)) / float(loss64),
           abs(float(loss_t) - float(loss64)) / float(loss64)))
  assert e_torch[0] < 1e-5, ('the seed: the densify + autograd route itself misses the bar here', e_torch)
  assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
  assert e_hip[0] < 1e-5, e_hip
  # every channel block of every mix weight gets a gradient of its own
  S = net.num_scale_long
  for t in range(net.num_layer):
    gw = g['filter.%d.weight' % t].view(128, S + R, -1)
    for c in range(R):
      assert gw[:, S + c].abs().max() > 0, (t, c)
    assert not all(torch.equal(gw[:, S], gw[:, S + c]) for c in range(1, R)), t
  if not net.general:
    assert g['embedding.weight'].abs().max() > 0


# ---- 3. what the densify route cannot do -------------------------------------------------------------------------
SEED_2740 = 2   # (seed 0: the torch route on a dense L 3.6e-5, HIP 1.7e-5 .. 2.6e-5; seed 1: the torch route 3.1e-4)


def test_training_beyond_the_dense_limit_of_typed_batches(launches, monkeypatch):
  """B 2, N 2740, E 2: (E + 1) N = 8220 > 8192 — the batch has no dense form.  The gradients against float64
  autograd on float64 per-channel L4 matrices built here from the edges (2 x 3 x 60 MB).
  The seed (ReLU sign flips, this file's header): the densify route raises here, so the route it WOULD take —
  `_torch_forward` under autograd — is handed those matrices rounded to fp32 as a dense [B,N,N,3] L, and must
  meet the bar on the recorded seed itself.  Seeds 0, 1, 2 were tried in that order; on 0 and 1 that route misses
  the bar (3.6e-5 and 3.1e-4 of |g|; the HIP route: 1.7e-5 .. 2.6e-5 from run to run and 2.2e-6), on 2 both meet
  it (torch 4.3e-6, HIP 2.8e-6)."""
  from lanczosnet_amd import ops
  N, K, E = 2740, 20, 2
  graphs = _graphs([N, N - 9], SEED_2740, E)
  assert eg.max_row_entries(graphs) <= eg.conv_cap(N)
  net, cfg = _net(G, SEED_2740, K, EIGHT, 10, 2, E)
  b = _batch(graphs, K, 10, SEED_2740, E)
  L = b['L']
  assert isinstance(L, ops.SparseLaplacian) and L.channels * L.N > ops.LAPLACIAN_MAX_CHANNEL_NODES
  assert int(L.images.flags.item()) == 0
  with pytest.raises(ops.NotSupported):
    L.to_dense()
  net.large_typed_backward_impl = 'torch'
  with pytest.raises(ops.NotSupported), warnings.catch_warnings():
    warnings.simplefilter('ignore')
    _step(net, b)
  assert launches == dict(typed=0, untyped=0)
  loss, g = _hip_step(net, b, launches, monkeypatch)
  assert torch.isfinite(loss) and all(torch.isfinite(x).all() for x in g.values())
  L64 = _t(np.stack([F.l4_channels_float64(gr, E, N) for gr in graphs]))             # [B,R,N,N]
  loss64, truth = _truth(net, b['node_feat'], [L64[:, c] for c in range(E + 1)], b['D'], b['V'], b['node_mask'],
                         b['label'])
  L32 = L64.permute(0, 2, 3, 1).float().contiguous()      # what `to_dense` would hold, had it the room
  del L64
  net.large_typed_backward_impl = 'torch'
  seen = []
  route = net._route
  net._route = lambda *a, **kw: seen.append(route(*a, **kw)) or seen[-1]
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    loss_t, g_t = _step(net, b, L32)
  del L32
  assert seen == ['torch'] and launches['untyped'] == 0
  e, e_torch = _deviation(g, truth), _deviation(g_t, truth)
  print('N = 2740, E = 2: gradients vs float64 autograd, worst of |g|: HIP %.2e (%s), torch route on a dense L '
        'built here %.2e (%s); loss %.2e / %.2e'
        % (e[0], e[1], e_torch[0], e_torch[1], abs(float(loss) - float(loss64)) / float(loss64),
           abs(float(loss_t) - float(loss64)) / float(loss64)))
  assert e_torch[0] < 1e-5, ('the seed: autograd through the torch restatement itself misses the bar here', e_torch)
  assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
  assert e[0] < 1e-5, e


# ---- 4. properties ---------------------------------------------------------------------------------------------------
def test_the_training_score_is_the_inference_score_and_steps_repeat_their_bits(launches, monkeypatch):
  """N <= 256: the forward's projection adds two partial sums per graph with float atomics, which commute (three
  or more: the forward's own states differ in the last bit between runs, tests/test_gpu_large_train.py)."""
  E = 3
  net, cfg = _net(G, 1, 20, EIGHT, 10, 3, E)
  b = _batch(_graphs([250, 201, 233], 1, E), 20, 10, 1, E)
  net.large_typed_backward_impl = 'hip'
  seen = []
  route = net._route
  net._route = lambda *a, **kw: seen.append(route(*a, **kw)) or seen[-1]
  with _no_dense(monkeypatch):
    score = net(b['node_feat'], b['L'], b['D'], b['V'], mask=b['node_mask'])
    assert score.requires_grad and score.grad_fn is not None
    with torch.no_grad():
      ref = net(b['node_feat'], b['L'], b['D'], b['V'], mask=b['node_mask'])
  assert seen == [ROUTE, 'large_hip']
  assert net._large_sparse_state[torch.device(DEV).index]['image_from'] == 'edges'
  assert torch.equal(score.detach(), ref)
  l1, g1 = _hip_step(net, b, launches, monkeypatch)
  l2, g2 = _hip_step(net, b, launches, monkeypatch)
  assert torch.equal(l1, l2)
  for k in g1:
    assert torch.equal(g1[k], g2[k]), k


def test_a_graphs_gradients_do_not_depend_on_batch_position_or_padding(launches, monkeypatch):
  """The same 193-node typed graph alone (N = 193) and as graph 2 of three padded to 257, with a one-hot
  grad_score: two fp32 evaluations of one sum in different tilings, held to 1e-5 of |g| against each other."""
  from lanczosnet_amd import ops
  E = 2
  g193 = _graphs([193], 2, E)[0]
  others = _graphs([257, 220], 3, E)
  net, cfg = _net(G, 2, 20, EIGHT, 10, 2, E)
  net.large_typed_backward_impl = 'hip'
  alone = _batch([g193], 20, 10, 2, E)
  batch = _batch(None, 20, 10, 2, E, items=_items(others, 10, 9) + _items([g193], 10, 7))
  pad = 257 - 193
  Fp = torch.nn.functional.pad
  batch['node_feat'][2] = Fp(alone['node_feat'][0], (0, 0, 0, pad))
  batch['D'][2] = alone['D'][0]
  batch['V'][2] = Fp(alone['V'][0], (0, 0, 0, pad))
  res = []
  for bt, row in ((alone, 0), (batch, 2)):
    net.zero_grad(set_to_none=True)
    with _no_dense(monkeypatch):
      score = net(bt['node_feat'], bt['L'], bt['D'], bt['V'], mask=bt['node_mask'])
      gs = torch.zeros_like(score)
      gs[row, 1] = 1.0
      score.backward(gs)
    assert ops.last_kernel().startswith(KERNEL)
    res.append((score[row].detach().clone(), _grads(net)))
  assert launches == dict(typed=2, untyped=0)
  assert float((res[0][0] - res[1][0]).abs().max()) <= 1e-5 * float(res[0][0].abs().max())
  e = _deviation(res[1][1], res[0][1])
  print('alone vs in a padded batch: worst deviation %.2e of |g| (%s)' % e)
  assert e[0] < 1e-5, e


# ---- 5. the envelope: everything else takes today's route, bit for bit ----------------------------------------------
@pytest.mark.parametrize('case', ['switch off', 'dense L', 'dropout', 'bf16 mode', 'raised image flag'])
def test_outside_the_envelope_the_torch_route_is_taken_unchanged(case, launches):
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_adjacency
  K, E = 20, 2
  L = None
  if case == 'raised image flag':
    graphs, N = eg.star_case()
    graphs = F.with_types(graphs, E, 51)
    assert eg.max_row_entries(graphs) > ops.large_sparse_row_cap(N)
  else:
    graphs = _graphs([257, 230, 201], 4, E)
  b = _batch(graphs, K, 10, 4, E)
  assert isinstance(b['L'], ops.SparseLaplacian) and b['L'].images is not None and b['L'].channels == 3
  if case == 'dense L':
    items = []
    for it, g in zip(eg.items(graphs, dim=10, seed=9), graphs):
      n, e, ty = g['n'], g['edges'], g['edge_type']
      a = np.zeros((n, n, E), np.float32)
      a[e[:, 0], e[:, 1], ty] = 1.0
      a[e[:, 1], e[:, 0], ty] = 1.0
      items.append(dict(node_feat=it['node_feat'], label=it['label'], adjs=a))
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      L = collate_graph_adjacency(items, K, device=DEV)['L']
    assert isinstance(L, torch.Tensor) and tuple(L.shape) == (3, 257, 257, 3)
  if case == 'raised image flag':
    assert int(b['L'].images.flags.item()) != 0
  res = []
  for opted in (True, False):
    net, _ = _net(G, 4, K, EIGHT, 10, 2, E)
    if case == 'dropout':
      net.dropout = 0.3
    if case == 'bf16 mode':
      net.gemm_mode = 'bf16'
    net.large_typed_backward_impl = 'hip' if opted and case != 'switch off' else 'torch'
    seen = []
    route = net._route
    net._route = lambda *a, **kw: seen.append(route(*a, **kw)) or seen[-1]
    with warnings.catch_warnings(), deterministic_dropout():
      warnings.simplefilter('ignore')
      res.append(_step(net, b, L))
    assert seen == ['torch'] and launches == dict(typed=0, untyped=0), (case, seen)
  assert torch.equal(res[0][0], res[1][0])
  for k in res[0][1]:
    assert torch.equal(res[0][1][k], res[1][1][k]), (case, k)


def test_the_typed_switch_leaves_untyped_batches_alone(launches):
  """The typed switch on, `large_backward_impl = 'torch'`: an untyped edge-list batch still takes 'torch'."""
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_edges
  rs = np.random.RandomState(1004)
  graphs = [dict(n=n, edges=eg.gnp_edges(n, 6.0 / n, rs)) for n in (257, 230)]
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    b = collate_graph_edges(eg.items(graphs, dim=10, seed=9), 20, device=DEV)
  assert isinstance(b['L'], ops.SparseLaplacian) and b['L'].images is None
  net, _ = _net(G, 4, 20, EIGHT, 10, 2, 1)
  net.large_typed_backward_impl, net.large_backward_impl = 'hip', 'torch'
  seen = []
  route = net._route
  net._route = lambda *a, **kw: seen.append(route(*a, **kw)) or seen[-1]
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    loss, _ = _step(net, b)
  assert seen == ['torch'] and launches == dict(typed=0, untyped=0) and torch.isfinite(loss)
