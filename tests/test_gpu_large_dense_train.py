"""Training DENSE collated batches beyond 128 nodes through the opt-in HIP backward on the sparse image(s) of the
tensor (`large_dense_backward_impl = 'hip'`: routes 'large_dense_train_hip' / 'large_dense_channels_train_hip';
csrc/sparse_symmetry.hip: lnz_large_sparse_image_symmetry).

1. The symmetry kernel alone against the numpy restatement of its status rule (tests/symmetry_mirror.py).
2. Gradients against float64 autograd: the bars and the seed protocol of tests/test_gpu_large_train.py — loss within
   1e-5, every parameter tensor's norm and 16 fixed +-1 projections of its gradient within 1e-5 of |g|, against a
   float64 restatement of `_torch_forward` with autograd, written here, on the dense L the module was given.  With
   hundreds of thousands of ReLU inputs one can lie within fp32 rounding of zero, and then NO fp32 implementation
   meets the bar: every case first holds the switch-off route — the only route before this one existed — to the
   same truth and asserts that IT meets 1e-5 on the recorded seed (seeds 0 .. 4 were tried per case; the first that
   passed is the one in the parametrisation).  Both routes' deviations are printed.
3. The same graphs through `collate_graph_edges` + LANCZOSNET_LARGE_BACKWARD=hip and through
   `collate_graph_adjacency` + the new switch: the same bits.
4. Refusals, 5. the switch's own scope: today's route, bit for bit.  6. Properties."""
import contextlib
import re
import warnings

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import edge_graphs as eg
import oracle
import symmetry_mirror as SM
from gradproj import deterministic_dropout, project_torch
from graph_fixture import GRAPH_CFG

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KERNEL, KERNEL_CH = 'large_grad_input_kernel', 'large_grad_input_channels_kernel'
ONE, EACH = 'large_dense_train_hip', 'large_dense_channels_train_hip'
EIGHT = [1, 2, 3, 5, 7, 10, 20, 30]     # config/graph_lanczos_net.yaml
G, Q = 'LanczosNetGeneral', 'LanczosNet'


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(autouse=True)
def launches(monkeypatch):
  """Every call, during a test, of the two input-gradient launches ('one', 'each'), the image launches ('image')
  and the symmetry check ('check'): lnz_last_kernel() keeps a thread's last note, which an earlier test may have
  left — the counts show which route a step took and what it launched."""
  from lanczosnet_amd import ops
  calls = dict(one=0, each=0, image=0, check=0, kernel=None)

  def counted(name, key):
    real = getattr(ops, name)

    def fn(*a, **kw):
      calls[key] += 1
      out = real(*a, **kw)
      if key in ('one', 'each'):
        calls['kernel'] = torch.ops.lanczosnet.last_kernel()   # (the launching thread's own note)
      return out
    monkeypatch.setattr(ops, name, fn)
  counted('large_grad_input', 'one')
  counted('large_grad_input_channels', 'each')
  counted('large_sparse_image', 'image')
  counted('large_sparse_image_channels', 'image')
  counted('large_sparse_image_symmetry', 'check')
  return calls


class _NoSquareAllocation(TorchDispatchMode):
  """Fails the step that produces a tensor with two dimensions of N nodes outside the storage of the dense L it
  was given: the permuted [B,C,N,N] copy of `_torch_forward`, a densified channel, an N x N product."""

  def __init__(self, L, N):
    super().__init__()
    self.N, self.own = N, L.untyped_storage().data_ptr()
    self.seen = 0

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    out = func(*args, **(kwargs or {}))
    for t in (out if isinstance(out, (tuple, list)) else (out,)):
      if isinstance(t, torch.Tensor):
        self.seen += 1
        if list(t.shape).count(self.N) >= 2 and t.untyped_storage().data_ptr() != self.own:
          raise AssertionError('%s produced a tensor of shape %s' % (func, tuple(t.shape)))
    return out


def _graphs(ns, seed, degree=6.0):
  rs = np.random.RandomState(1000 + seed)
  return [dict(n=int(n), edges=eg.gnp_edges(int(n), degree / n, rs)) for n in ns]


def _net(model, seed, K, long_dist, din, layers, E=1, **over):
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
  # every switch a route depends on, pinned (the environment may set the class defaults)
  net.large_backward_impl = net.large_typed_backward_impl = net.large_dense_backward_impl = 'torch'
  net.mid_backward_impl, net.backward_impl, net.gemm_mode, net.large_sparse_channels = 'torch', 'hip', 'fp32', 'one'
  return net, cfg


def _dense_items(graphs, din, seed, E=1):
  """The collate items with adjs [n,n,E]: E = 1 the graph; E >= 2: every edge in the channel of its `edge_type`."""
  its = eg.items(graphs, dim=din, seed=seed, dense=True)
  if E > 1:
    for it, g in zip(its, graphs):
      A = np.zeros((g['n'], g['n'], E), np.float32)
      e, ty = g['edges'], g['edge_type']
      A[e[:, 0], e[:, 1], ty] = 1.0
      A[e[:, 1], e[:, 0], ty] = 1.0
      it['adjs'] = A
  return its


def _batch(graphs, K, din, seed, cfg=None, E=1, items=None):
  """`collate_graph_adjacency`'s batch of the graphs (L a dense [B,N,N,E+1] float32 tensor); for the embedding
  model (din None) node ids in place of features."""
  from lanczosnet_amd.dataset import collate_graph_adjacency
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    b = collate_graph_adjacency(items or _dense_items(graphs, din or 4, 5 + seed, E), K, device=DEV)
  assert isinstance(b['L'], torch.Tensor) and b['L'].dtype == torch.float32
  if din is None:
    rs = np.random.RandomState(77 + seed)
    b['node_feat'] = _t(rs.randint(0, cfg['num_atom'], size=tuple(b['node_mask'].shape)).astype(np.int64))
    b['label'] = _t(rs.randn(b['node_mask'].shape[0], cfg['output_dim']).astype(np.float32))
  return b


def _grads(net):
  return {k: p.grad.clone() for k, p in net.named_parameters()}


def _step(net, b, L=None, mask=None):
  net.zero_grad(set_to_none=True)
  _, loss = net(b['node_feat'], b['L'] if L is None else L, b['D'], b['V'], label=b['label'],
                mask=b['node_mask'] if mask is None else mask)
  loss.backward()
  return loss.detach(), _grads(net)


@contextlib.contextmanager
def _routes(net):
  seen = []
  route = net._route
  net._route = lambda *a, **kw: seen.append(route(*a, **kw)) or seen[-1]
  try:
    yield seen
  finally:
    del net._route


def _hip_step(net, b, launches, L=None, mask=None, each=False, watch=True):
  """One step with the switch on: the route, the kernel's name, the counted launches, and no N x N tensor.
  watch: the backward runs on the CALLING thread, so that the dispatch mode sees its allocations too; the
  input-gradient kernel's name is then read where it is launched (lnz_last_kernel() is per thread, and that thread
  goes on to launch the filter-MLP gradients).  Without: autograd's own thread, and `ops.last_kernel()` after
  `backward()` as a user reads it."""
  from lanczosnet_amd import ops
  L = b['L'] if L is None else L
  net.large_dense_backward_impl = 'hip'
  before = dict(launches, kernel=None)
  launches['kernel'] = None
  with contextlib.ExitStack() as stack:
    stack.enter_context(warnings.catch_warnings())
    seen = stack.enter_context(_routes(net))
    if watch:
      stack.enter_context(torch.autograd.set_multithreading_enabled(False))
      mode = stack.enter_context(_NoSquareAllocation(L, L.shape[1]))
    warnings.filterwarnings('error', message='.*(large_dense_backward_impl|densified).*')
    out = _step(net, b, L, mask)
  assert seen == [EACH if each else ONE], seen
  assert not watch or mode.seen > 20
  name = launches['kernel'] if watch else ops.last_kernel()
  assert name.startswith(KERNEL_CH if each else KERNEL), name
  n_launch = net.num_layer - (1 if net.general else 0)
  assert launches['each' if each else 'one'] - before['each' if each else 'one'] == n_launch
  assert launches['one' if each else 'each'] == before['one' if each else 'each']
  return out


def _torch_step(net, b, launches, L=None, mask=None):
  net.large_dense_backward_impl = 'torch'
  before = dict(launches)
  with warnings.catch_warnings(), _routes(net) as seen:
    warnings.simplefilter('ignore')
    out = _step(net, b, L, mask)
  assert seen == ['torch'] and launches == before
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


def _channels64(L):
  return [L[..., c].double() for c in range(L.shape[3])]


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------
def _weighted(ns, N, seed, full_row=None):
  """[B,N,N] float32, symmetric bit for bit: ~6 weighted neighbours per node and a diagonal, graph b on its first
  ns[b] nodes.  full_row = (b, entries): node 0 of graph b gets exactly that many entries."""
  rs = np.random.RandomState(seed)
  L = np.zeros((len(ns), N, N), np.float32)
  for b, n in enumerate(ns):
    e = eg.gnp_edges(n, 6.0 / max(n, 1), rs)
    if full_row is not None and full_row[0] == b:
      e = e[(e != 0).all(axis=1)]
      nb = np.arange(1, full_row[1], dtype=np.int32)
      e = np.concatenate([e, np.stack([np.zeros_like(nb), nb], axis=1)], axis=0)
    w = (rs.rand(e.shape[0]) + 0.25).astype(np.float32)
    L[b, e[:, 0], e[:, 1]] = w
    L[b, e[:, 1], e[:, 0]] = w
    i = np.arange(n)
    L[b, i, i] = (rs.rand(n) + 0.25).astype(np.float32)
  return L


def _image_and_status(dense_channels):
  """dense_channels: list of [B,N,N] float32 (numpy) -> (host image arrays, cap, device status): one channel ->
  ops.large_sparse_image of the channels-last PAIR [B,N,N,2] (odd N: ascending entry order, even N: pair order);
  several -> ops.large_sparse_image_channels."""
  from lanczosnet_amd import ops
  if len(dense_channels) == 1:
    L = _t(np.stack([dense_channels[0]] * 2, axis=3))
    img = ops.large_sparse_image(L, values=True)
    assert ops.last_kernel().startswith('sparse_image_kernel<%s>' % ('pair' if L.shape[1] % 2 == 0 else 'strided'))
  else:
    img = ops.large_sparse_image_channels(_t(np.stack(dense_channels, axis=3)))
  st = ops.large_sparse_image_symmetry(img)
  assert ops.last_kernel() == 'sparse_image_symmetry_kernel'
  st2 = ops.large_sparse_image_symmetry(img)
  assert torch.equal(st, st2), 'two calls, two answers'
  host = (img.entries.cpu().numpy(), img.values.cpu().numpy(), img.counts.cpu().numpy())
  return host, img.cap, int(img.flags.item()), st.cpu().numpy()


SHAPES = {   # name -> (ns, N, channels)
    'N129 odd, ascending order': ([129, 100, 129], 129, 1),
    'N130 pair order': ([130, 97, 130], 130, 1),
    'N257 ragged, three channels': ([257, 200, 231], 257, 3),
}


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_symmetry_kernel_matches_the_numpy_rule(shape):
  ns, N, R = SHAPES[shape]
  cap = eg.conv_cap(N)
  assert cap == 32
  base = [_weighted(ns, N, 40 + c, full_row=(2, cap)) for c in range(R)]

  def nxt(x, k):
    for _ in range(k):
      x = np.nextafter(np.float32(x), np.float32(np.inf))
    return x

  def first_edge(Lb, lo=1):
    i, j = np.nonzero(np.triu(Lb, 1)[lo:, :])
    return int(i[0]) + lo, int(j[0])

  def run(ch, want):
    host, c, flags, st = _image_and_status(ch)
    assert c == cap and flags == 0
    ref = SM.status_rule(*host, cap)
    assert st.tolist() == ref.tolist(), (shape, st, ref)
    assert st.tolist() == want, (shape, st, want)
    return host
  B = len(ns)
  clean = [0] * (R * B)
  host = run(base, clean)                                     # symmetric: all words 0
  assert int(host[2].reshape(-1, B, N)[0, 2, 0]) == cap       # (a row holding exactly cap entries, its mirrors found)
  r = R - 1                                                   # the channel the defects go to (R = 3: channel 2 only)
  i, j = first_edge(base[r][1])
  # one mirror zeroed in graph 1 only
  ch = [x.copy() for x in base]
  ch[r][1, j, i] = 0.0
  want = list(clean)
  want[r * B + 1] = 1
  run(ch, want)
  # a mirror moved by one ulp: accepted; by two: bit 1
  ch = [x.copy() for x in base]
  ch[r][1, j, i] = nxt(ch[r][1, j, i], 1)
  run(ch, clean)
  ch[r][1, j, i] = nxt(ch[r][1, j, i], 1)
  want = list(clean)
  want[r * B + 1] = 2
  run(ch, want)
  # the defect at row / column n - 1 (graph 1 is ragged: n - 1 < N - 1; graph 0: n - 1 = N - 1), both bits
  ch = [x.copy() for x in base]
  want = list(clean)
  for b in (0, 1):
    n = ns[b]
    ch[r][b, n - 1, 0] = 0.0
    ch[r][b, 0, n - 1] = 0.5                                  # (0, n - 1) without (n - 1, 0)
    want[r * B + b] |= 1
  ch[r][0, N - 1, 5], ch[r][0, 5, N - 1] = 0.75, -0.75         # ... and a pair a sign apart in the last row
  want[r * B + 0] |= 2
  run(ch, want)
  # the full row's last mirror gone: found missing at entry `cap - 1` of the row
  ch = [x.copy() for x in base]
  ch[r][2, cap - 1, 0] = 0.0
  want = list(clean)
  want[r * B + 2] = 1
  run(ch, want)
  # a graph of zero nodes
  ch = [x.copy() for x in base]
  for x in ch:
    x[1] = 0.0
  host = run(ch, clean)
  assert not host[2].reshape(-1, B, N)[:, 1].any()


def test_symmetry_kernel_is_safe_on_a_flagged_image():
  """A star of 301 nodes: row 0 overflows the 32 entries; the launch runs, its answer is ignored."""
  from lanczosnet_amd import ops
  graphs, N = eg.star_case()
  L = _t(np.concatenate([eg.dense_adjs(graphs[:1], N)] * 2, axis=3) + np.eye(N, dtype=np.float32)[None, :, :, None])
  img = ops.large_sparse_image(L, values=True)
  st = ops.large_sparse_image_symmetry(img)
  torch.cuda.synchronize()
  assert int(img.flags.item()) & 2 and tuple(st.shape) == (1,)
  with pytest.raises(ValueError):
    ops.large_sparse_image_symmetry(ops.large_sparse_image(L))     # no values


# ---- 2. against float64 autograd -------------------------------------------------------------------------------
def _ragged(N, B):
  return [N] + [N - 57 + 13 * b for b in range(B - 1)]


# node counts, K, long scales, input width (None: the embedding model's), layers, model, recorded seed
CASES = {
    'N129 ragged K20 S8': ([129, 100, 113], 20, EIGHT, 10, 2, G, 0),
    'N257 ragged K20 S8': (_ragged(257, 3), 20, EIGHT, 10, 2, G, 0),
    'N260 the image of the collate': ([260, 203, 216], 20, EIGHT, 10, 2, G, 0),
    'K64 S1 width 128': ([300, 193, 262], 64, [1], 128, 2, G, 0),
    'no long scales': (_ragged(257, 3), 20, [], 10, 2, G, 0),
    'embedding model': (_ragged(257, 3), 20, EIGHT, None, 2, Q, 0),
    'seven layers': (_ragged(257, 3), 20, EIGHT, 10, 7, G, 0),
}


def _case(name, seed=None):
  ns, K, long_dist, din, layers, model, recorded = CASES[name]
  seed = recorded if seed is None else seed
  graphs = _graphs(ns, seed)
  assert eg.max_row_entries(graphs) <= eg.conv_cap(max(ns))
  net, cfg = _net(model, seed, K, long_dist, din, layers)
  return net, _batch(graphs, K, din, seed, cfg)


def _against_truth(name, net, b, launches, L=None, mask=None, each=False):
  """-> (loss, gradients) of the HIP step, after both routes were held to float64 autograd."""
  L = b['L'] if L is None else L
  mask = b['node_mask'] if mask is None else mask
  loss64, truth = _truth(net, b['node_feat'], _channels64(L), b['D'], b['V'], mask, b['label'])
  loss_t, g_t = _torch_step(net, b, launches, L, mask)
  loss, g = _hip_step(net, b, launches, L, mask, each=each)
  e_hip, e_torch = _deviation(g, truth), _deviation(g_t, truth)
  print('%s: gradients vs float64 autograd, worst of |g|: HIP %.2e (%s), switch off %.2e (%s); loss %.2e / %.2e'
        % (name, e_hip[0], e_hip[1], e_torch[0], e_torch[1], abs(float(loss) - float(loss64)) / float(loss64),
           abs(float(loss_t) - float(loss64)) / float(loss64)))
  assert e_torch[0] < 1e-5, ('the seed: the switch-off route itself misses the bar here', e_torch)
  assert abs(float(loss) - float(loss64)) < 1e-5 * abs(float(loss64))
  assert e_hip[0] < 1e-5, e_hip
  return loss, g


@pytest.mark.parametrize('name', sorted(CASES))
def test_hip_backward_matches_float64_autograd(name, launches):
  from lanczosnet_amd import ops
  net, b = _case(name)
  L = b['L']
  N = L.shape[1]
  assert torch.equal(L[..., 0], L[..., 1]) and torch.equal(L[..., 0], L[..., 0].transpose(1, 2))
  # (the collate's K-step pass leaves the image where it reads L in place: 193 .. 2048 nodes, N a multiple of 4)
  riding = ops.attached_sparse_image(L) is not None
  assert riding == (N > 192 and N % 4 == 0) and (riding or name != 'N260 the image of the collate')
  loss, g = _against_truth(name, net, b, launches)
  st = net._large_dense_state[torch.device(DEV).index]
  assert st['image_from'] == ('collate' if riding else 'module') and st['last_flags'] == 0
  assert launches['check'] == 1 and launches['image'] == (0 if riding else 1)
  assert ops.attached_sparse_image(L).symmetric is True
  # both edge-channel blocks of every mix weight get the same gradient
  S = net.num_scale_long
  for t in range(net.num_layer):
    gw = g['filter.%d.weight' % t].view(128, S + 2, -1)
    assert gw[:, S].abs().max() > 0 and torch.equal(gw[:, S], gw[:, S + 1]), t
  if not net.general:
    assert g['embedding.weight'].abs().max() > 0
  # the tensor is reused: the verdict rides on its image, nothing is asked again
  before = dict(launches)
  _hip_step(net, b, launches, watch=False)
  assert (launches['check'], launches['image']) == (before['check'], before['image'])


def test_the_modules_own_image_gives_the_collates_bits(launches):
  """N 252 (N <= 256: the forward's projection adds two partial sums, which commute; a multiple of 4: the collate
  reads L in place and leaves its image).  The batch of the collate, whose image rides on L, and `L.clone()`,
  which carries none: the module builds it, and the gradients are the same bits."""
  from lanczosnet_amd import ops
  ns, seed = [252, 201, 233], 0
  net, cfg = _net(G, seed, 20, EIGHT, 10, 2)
  b = _batch(_graphs(ns, seed), 20, 10, seed)
  assert ops.attached_sparse_image(b['L']) is not None
  l1, g1 = _against_truth('N252 collate', net, b, launches)
  assert net._large_dense_state[torch.device(DEV).index]['image_from'] == 'collate' and launches['image'] == 0
  Lc = b['L'].clone()
  assert ops.attached_sparse_image(Lc) is None
  l2, g2 = _hip_step(net, b, launches, L=Lc)
  assert net._large_dense_state[torch.device(DEV).index]['image_from'] == 'module' and launches['image'] == 1
  assert ops.attached_sparse_image(Lc) is not None and launches['check'] == 2
  assert torch.equal(l1, l2)
  for k in g1:
    assert torch.equal(g1[k], g2[k]), k


def _weighted_batch(ns, K, seed):
  """A weighted batch as the reference builds it: L = D^-1/2 (I + A) D^-1/2 with real edge weights, in float64 on
  the host, (s_i a_ij) s_j in that order, then cast — and every fourth stored mirror below the diagonal moved one
  fp32 ulp, which such a cast can do and the rule accepts.  Both channels are that operator."""
  from lanczosnet_amd import ops
  N, B = max(ns), len(ns)
  rs = np.random.RandomState(300 + seed)
  L64 = np.zeros((B, N, N), np.float64)
  for b, g in enumerate(_graphs(ns, seed)):
    n, e = g['n'], g['edges']
    A = np.zeros((n, n), np.float64)
    w = rs.rand(e.shape[0]) + 0.5
    A[e[:, 0], e[:, 1]] = w
    A[e[:, 1], e[:, 0]] = w
    A += np.eye(n)
    s = 1.0 / np.sqrt(A.sum(axis=1))
    L64[b, :n, :n] = (s[:, None] * A) * s[None, :]
  L32 = L64.astype(np.float32)
  bi, i, j = np.nonzero(np.tril(L32, -1))
  pick = np.arange(0, bi.shape[0], 4)
  L32[bi[pick], i[pick], j[pick]] = np.nextafter(L32[bi[pick], i[pick], j[pick]], np.float32(1e9))
  up, lo = L32, np.swapaxes(L32, 1, 2)
  ulps = np.abs(up.view(np.int32).astype(np.int64) - np.ascontiguousarray(lo).view(np.int32).astype(np.int64))
  assert int(ulps.max()) == 1 and int((ulps == 1).sum()) >= 2 * len(pick) > 100
  L = _t(np.stack([L32, L32], axis=3))
  n_nodes = _t(np.array(ns, np.int32))
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    D, V = ops.lanczos_ritz_collated(L, n_nodes, K)
  mask = np.zeros((B, N), np.uint8)
  for b, n in enumerate(ns):
    mask[b, :n] = 1
  rs = np.random.RandomState(5 + seed)
  return dict(L=L, D=D, V=V, node_mask=_t(mask), node_feat=_t(rs.randn(B, N, 10).astype(np.float32) * mask[..., None]),
              label=_t(rs.randn(B, 2).astype(np.float32)))


def test_mirrors_one_ulp_apart_are_accepted_and_meet_the_bar(launches):
  net, cfg = _net(G, 0, 20, EIGHT, 10, 2)
  b = _weighted_batch(_ragged(257, 3), 20, 0)
  assert not torch.equal(b['L'][..., 0], b['L'][..., 0].transpose(1, 2))
  _against_truth('weighted, mirrors <= 1 ulp apart', net, b, launches)
  assert launches['check'] == 1


def test_a_zero_stride_expanded_single_channel(launches):
  net, b = _case('N257 ragged K20 S8')
  L1 = b['L'][..., :1].contiguous()
  L = L1.expand(-1, -1, -1, 2)
  assert L.stride(3) == 0
  _, g = _against_truth('expanded single channel', net, b, launches, L=L)
  assert launches['image'] == 1 and launches['check'] == 1


def _typed_case(seed, ns, K=20, layers=2, channels='each'):
  import large_typed_train_fixture as TF
  graphs = TF.with_types(_graphs(ns, seed), 2, 2000 + seed)
  net, cfg = _net(G, seed, K, EIGHT, 10, layers, E=2)
  net.large_sparse_channels = channels
  return net, _batch(graphs, K, 10, seed, cfg, E=2)


def test_three_distinct_channels_each_get_their_own_gradient(launches):
  from lanczosnet_amd import ops
  net, b = _typed_case(0, _ragged(257, 3))
  L = b['L']
  assert L.shape[3] == 3 and L.stride(3) != 0 and not torch.equal(L[..., 1], L[..., 2])
  _, g = _against_truth('three distinct channels', net, b, launches, each=True)
  assert launches['image'] == 1 and launches['check'] == 1
  imgs = ops.attached_sparse_images(L)
  assert imgs is not None and imgs.R == 3 and imgs.symmetric is True
  S = net.num_scale_long
  for t in range(net.num_layer):
    gw = g['filter.%d.weight' % t].view(128, S + 3, -1)
    for c in range(3):
      assert gw[:, S + c].abs().max() > 0
      for c2 in range(c):
        assert not torch.equal(gw[:, S + c], gw[:, S + c2]), (t, c, c2)


# ---- 3. same graphs, two surfaces ------------------------------------------------------------------------------
def test_edge_lists_and_the_dense_collate_give_the_same_bits(launches):
  """Graphs of 193 .. 256 nodes: `collate_graph_edges` + large_backward_impl = 'hip' against
  `collate_graph_adjacency` + the new switch.  The images are bit-identical (ops.dense_entry_orders), and so are
  the loss and every gradient."""
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_edges
  ns, seed = [250, 201, 233], 1
  graphs = _graphs(ns, seed)
  net, cfg = _net(G, seed, 20, EIGHT, 10, 3)
  dense = _batch(graphs, 20, 10, seed)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    edges = collate_graph_edges(eg.items(graphs, dim=10, seed=5 + seed), 20, device=DEV)
  assert isinstance(edges['L'], ops.SparseLaplacian)
  for k in ('D', 'V', 'node_feat', 'label', 'node_mask'):
    assert torch.equal(dense[k], edges[k]), k
  net.large_backward_impl = 'hip'
  with warnings.catch_warnings(), _routes(net) as seen:
    warnings.filterwarnings('error', message='.*densified.*')
    l_e, g_e = _step(net, edges)
  assert seen == ['large_train_hip'] and ops.last_kernel().startswith(KERNEL)
  net.large_backward_impl = 'torch'
  l_d, g_d = _hip_step(net, dense, launches, watch=False)
  assert torch.equal(l_e, l_d)
  for k in g_e:
    assert torch.equal(g_e[k], g_d[k]), k


# ---- 4. refusals keep today's bits -----------------------------------------------------------------------------
def _refusal_batch(case):
  """-> (net, batch, L, warning pattern)."""
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_edges
  if case == 'distinct channels under one':
    net, b = _typed_case(4, [257, 230, 201], channels='one')
    return net, b, b['L'], r"operator channels of graph 0 differ"
  graphs = eg.star_case()[0] if case == 'a row beyond row_cap' else _graphs([257, 230, 201], 4)
  net, cfg = _net(G, 4, 20, EIGHT, 10, 2)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    b = collate_graph_edges(eg.items(graphs, dim=10, seed=9), 20, device=DEV)
    L = b['L'].to_dense()
  if case == 'a row beyond row_cap':
    assert eg.max_row_entries(graphs) > ops.large_sparse_row_cap(L.shape[1])
    return net, b, L, r'graph 0 has a row of more than row_cap = 32'
  # an asymmetric operator: the diffusion map L7 of the same graphs, as an expanded single channel
  L7 = ops.laplacian(_t(eg.dense_adjs(graphs, 257)), b['L'].n_nodes, 'L7')[..., :1].contiguous().expand(-1, -1, -1, 2)
  assert not torch.equal(L7[..., 0], L7[..., 0].transpose(1, 2))
  return net, b, L7, r'graph 0 \(operator channel 0\) is not symmetric: .*more than one fp32 ulp apart'


@pytest.mark.parametrize('case', ['an asymmetric operator', 'a row beyond row_cap', 'distinct channels under one'])
def test_refusals_keep_todays_bits(case, launches):
  net, b, L, pattern = _refusal_batch(case)
  off = _torch_step(net, b, launches, L)
  net.large_dense_backward_impl = 'hip'
  with warnings.catch_warnings(record=True) as rec, _routes(net) as seen:
    warnings.simplefilter('always')
    on = _step(net, b, L)
  assert seen == ['torch'] and launches['one'] == launches['each'] == 0
  assert launches['image'] == 1 and launches['check'] == 1
  msgs = [str(w.message) for w in rec
          if issubclass(w.category, UserWarning) and 'large_dense_backward_impl' in str(w.message)]
  assert len(msgs) == 1 and re.search(pattern, msgs[0]), msgs
  assert torch.equal(on[0], off[0])
  for k in on[1]:
    assert torch.equal(on[1][k], off[1][k]), (case, k)
  st = net._large_dense_state[torch.device(DEV).index]
  assert st['skip'] == net.large_sparse_backoff and '%d dense batches' % st['skip'] in msgs[0]
  # the same tensor again: its verdict is on the image; another tensor inside the back-off: neither launch runs
  for L2 in (L, L.clone() if L.stride(3) != 0 else L[..., :1].contiguous().expand(-1, -1, -1, 2)):
    with warnings.catch_warnings(record=True) as rec, _routes(net) as seen:
      warnings.simplefilter('always')
      again = _step(net, b, L2)
    assert seen == ['torch'] and launches['image'] == 1 and launches['check'] == 1
    assert not [w for w in rec if 'large_dense_backward_impl' in str(w.message)]      # once per module
    assert torch.equal(again[0], off[0])
  assert st['skip'] == net.large_sparse_backoff - 1


# ---- 5. the switch's own scope ---------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['dropout', 'bf16 mode', 'switch off', 'N = 128', 'backward_impl torch',
                                  'a SparseLaplacian batch', 'only the two old switches'])
def test_outside_its_scope_the_torch_route_is_taken_unchanged(case, launches):
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_edges
  K = 20
  ns = [128, 100, 111] if case == 'N = 128' else [257, 230, 201]
  graphs = _graphs(ns, 4)
  if case == 'a SparseLaplacian batch':
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      b = collate_graph_edges(eg.items(graphs, dim=10, seed=9), K, device=DEV)
    assert isinstance(b['L'], ops.SparseLaplacian)
  else:
    b = _batch(graphs, K, 10, 4)
  res = []
  for opted in (True, False):
    net, _ = _net(G, 4, K, EIGHT, 10, 2)
    if case == 'dropout':
      net.dropout = 0.3
    if case == 'bf16 mode':
      net.gemm_mode = 'bf16'
    if case == 'backward_impl torch':
      net.backward_impl = 'torch'
    if case == 'only the two old switches':
      net.large_backward_impl = net.large_typed_backward_impl = 'hip' if opted else 'torch'
    else:
      net.large_dense_backward_impl = 'hip' if opted and case != 'switch off' else 'torch'
    with warnings.catch_warnings(), deterministic_dropout(), _routes(net) as seen:
      warnings.simplefilter('ignore')
      res.append(_step(net, b))
    assert seen == ['torch'], (case, seen)
    assert launches == dict(one=0, each=0, image=0, check=0, kernel=None), (case, launches)
  assert torch.equal(res[0][0], res[1][0])
  for k in res[0][1]:
    assert torch.equal(res[0][1][k], res[1][1][k]), (case, k)


# ---- 6. properties ---------------------------------------------------------------------------------------------
def test_two_identical_steps_give_the_same_bits(launches):
  """(N <= 256: the forward's projection adds two partial sums per graph with float atomics, which commute.)"""
  net, cfg = _net(G, 1, 20, EIGHT, 10, 3)
  b = _batch(_graphs([250, 201, 233], 1), 20, 10, 1)
  l1, g1 = _hip_step(net, b, launches)
  l2, g2 = _hip_step(net, b, launches)
  assert torch.equal(l1, l2)
  for k in g1:
    assert torch.equal(g1[k], g2[k]), k


def test_a_graphs_gradients_do_not_depend_on_batch_position_or_padding(launches):
  """The same 193-node graph alone (N = 193) and as graph 2 of three padded to 257, with a one-hot grad_score: two
  fp32 evaluations of one sum in different tilings, held to the gradient bar, 1e-5 of |g|, against each other."""
  from lanczosnet_amd import ops
  g193 = _graphs([193], 2)[0]
  others = _graphs([257, 220], 3)
  net, cfg = _net(G, 2, 20, EIGHT, 10, 2)
  net.large_dense_backward_impl = 'hip'
  alone = _batch([g193], 20, 10, 2)
  its = eg.items(others, dim=10, seed=9, dense=True) + eg.items([g193], dim=10, seed=7, dense=True)
  batch = _batch(None, 20, 10, 2, items=its)
  pad = 257 - 193
  Fp = torch.nn.functional.pad
  batch['node_feat'][2] = Fp(alone['node_feat'][0], (0, 0, 0, pad))
  batch['D'][2] = alone['D'][0]
  batch['V'][2] = Fp(alone['V'][0], (0, 0, 0, pad))
  res = []
  for bt, row in ((alone, 0), (batch, 2)):
    net.zero_grad(set_to_none=True)
    with _routes(net) as seen:
      score = net(bt['node_feat'], bt['L'], bt['D'], bt['V'], mask=bt['node_mask'])
    assert seen == [ONE]
    gs = torch.zeros_like(score)
    gs[row, 1] = 1.0
    score.backward(gs)
    assert ops.last_kernel().startswith(KERNEL)
    res.append((score[row].detach().clone(), _grads(net)))
  assert launches['one'] == 2
  assert float((res[0][0] - res[1][0]).abs().max()) <= 1e-5 * float(res[0][0].abs().max())
  e = _deviation(res[1][1], res[0][1])
  print('alone vs in a padded batch: worst deviation %.2e of |g| (%s)' % e)
  assert e[0] < 1e-5, e


def test_a_mask_that_is_not_a_prefix_meets_the_bar(launches):
  """Every seventh node of every graph is masked OUT of the readout while L still couples it to its neighbours:
  rows outside the mask get a zero gradient from the readout and a non-zero one through L and V, as autograd
  computes it (no node counts are handed to lnz_large_grad_project)."""
  net, b = _case('N257 ragged K20 S8')
  mask = b['node_mask'].clone()
  mask[:, 3::7] = 0
  assert bool((mask[:, :-1] < mask[:, 1:]).any())
  _against_truth('a mask with holes', net, b, launches, mask=mask)


def test_no_dense_operator_is_allocated(launches):
  """B 2, N 2100, two layers, as tests/test_gpu_large_train.py::test_no_dense_operator_is_allocated: the second
  step's peak allocation above the resident batch (the dense L and the image the first step left on it) stays
  under 4 x (states + image bytes); ONE permuted copy of the operator is 70 MB."""
  from lanczosnet_amd import ops
  N = 2100
  graphs = _graphs([N, N - 49], 0)
  assert eg.max_row_entries(graphs) <= eg.conv_cap(N)
  net, cfg = _net(G, 0, 8, EIGHT, 10, 2)
  b = _batch(graphs, 8, 10, 0)
  loss1, _ = _hip_step(net, b, launches)
  img = ops.attached_sparse_image(b['L'])
  assert launches['image'] == 1 and img is not None and img.cap == 72
  B = len(graphs)
  states = net.num_layer * B * N * 128 * 4
  image = sum(t.numel() * t.element_size() for t in (img.entries, img.values, img.counts))
  bound = 4 * (states + image)
  assert bound < B * N * N * 2 * 4 / 2
  net.zero_grad(set_to_none=True)
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  loss, _ = _hip_step(net, b, launches)
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - before
  print('peak allocation of one step: %.1f MB (states %.1f MB, image %.1f MB, bound %.1f MB; the dense L: %.1f MB)'
        % (peak / 1e6, states / 1e6, image / 1e6, bound / 1e6, B * N * N * 8 / 1e6))
  assert launches['image'] == 1 and launches['check'] == 1
  assert torch.isfinite(loss) and torch.isfinite(loss1) and peak < bound
