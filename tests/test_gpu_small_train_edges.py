"""Training graphs of at most 32 nodes through the HIP backward (`_LanczosNetFusedFunction`,
`_fused_conv_backward`; lnz_lanczosnet_input_grad, lnz_lanczosnet_messages, lnz_lanczosnet_gain_grad,
lnz_head_backward, lnz_spectral_mlp_grad, lnz_embedding_grad) at the edges of its
envelope, against a float64 restatement of the reference's maths with autograd, written here.

The truth (`_truth`) works from the raw parameters in the REFERENCE's channel order of
`filter.t.weight`'s column blocks (model/lanczos_net.py:163-180: short-diffusion channels, long
channels, the E + 1 operator channels), so the module's channel reordering is under test too, and it
keeps the pre-activation output of every conv layer and the input state as graph nodes:
dLoss/dout_l and dLoss/dX_0 come out beside the parameter gradients.  It is computed once per case
and shared (`_truth_of`).

Bars: the project's gradient bars, applied by `_deviation` of
test_gpu_mid_train.py — loss within 1e-5, every parameter tensor's norm and 16 fixed +-1 projections
of its gradient within 1e-5 of |g| (tests/gradproj.py), a tensor whose true gradient is exactly zero
exactly zero — and, for the input-gradient kernel's own outputs, the project's fp32 bar
`rel_err < 1e-5` per layer, with everything that is padding exactly zero.  The fp32 torch route's own
deviation from the same truth is printed beside the kernels'.

Conditioning.  The bar is met only where fp32 itself can meet it: no ReLU input within fp32 rounding
of zero (the caveat above the case list of test_gpu_mid_train.py).  Every case below was checked on
the CPU: `_truth` run in fp32 against `_truth` in float64 (mean squared error loss), worst deviation
of |g| over the tensors, and the module's `_torch_forward` scores in fp32 against float64:
see CONDITIONING.  No true gradient of any case is exactly zero."""
import functools

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err
from test_gpu_mid_train import _deviation, _step
from test_gpu_parity import _model, _t, draw_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KERNEL = 'lanczosnet_strip_kernel<1,'

# name: (B, N, n_min, n_max, K, short, long, filter kind, din, dout, layers, bond types, general)
CASES = {
    'full tile, K = 32': (3, 32, 32, 32, 32, [], [1, 2, 4], 'MLP', 32, 5, 2, 3, False),
    'one-node molecules, K > n, one output': (4, 9, 1, 3, 20, [], [1, 3, 7], 'MLP', 32, 1, 2, 3, False),
    'a single layer, 31 outputs, odd K': (5, 17, 5, 17, 7, [], [2, 5], 'MLP', 64, 31, 1, 1, False),
    'no long scales': (6, 24, 8, 24, 20, [1, 2], [], 'MLP', 128, 4, 3, 2, False),
    'eight short scales, power gains': (5, 20, 6, 20, 12, [1, 2, 3, 4, 5, 6, 7, 8], [1, 2], 'None', 32, 3, 2, 2, False),
    'General, input width 1, eight long': (7, 26, 3, 26, 5, [], [1, 2, 3, 5, 7, 10, 20, 30], 'MLP', 1, 2, 3, 1, True),
    'General, input width 65 (pads to 128)': (7, 32, 17, 32, 20, [2], [3, 10], 'MLP', 65, 16, 2, 3, True),
    'B = 1': (1, 32, 31, 31, 20, [], [1, 2, 4], 'MLP', 32, 5, 2, 3, False),
    # 8 short + 12 long + 12 operator channels = the 32 of MAX_CHANNELS; eleven bond types are more than
    # draw_batch draws: `_many_bond_types`.  Seven graphs of 6..16 nodes: two strips.
    '32 channels': (7, 16, 6, 16, 16, [1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15, 20], 'MLP',
                    32, 3, 2, 11, False),
}
IDS = list(CASES)

# CONDITIONING (module docstring), all nine cases, on the CPU: `_truth` in fp32 against `_truth` in
# float64 — worst deviation of |g| over the parameter tensors (the tensor), worst rel_err of a layer's
# dLoss/dout_l, rel_err of dLoss/dX_0; the loss of the module's fp32 `_torch_forward` against float64.
#   full tile, K = 32                       9.6e-7 (spectral_filter.1.4.weight)   3e-7   4e-7   6e-8
#   one-node molecules (n = 3, 1, 1, 1)     7.2e-7 (att_func.0.weight)            2e-7   2e-7   3e-8
#   a single layer, 31 outputs, odd K       9.4e-7 (spectral_filter.0.0.weight)   3e-7   3e-7   6e-8
#   no long scales                          4.9e-7 (filter.3.weight)              3e-7   3e-7   2e-8
#   eight short scales, power gains         5.1e-7 (att_func.0.weight)            2e-7   2e-7   9e-9
#   General, input width 1, eight long      2.4e-6 (spectral_filter.0.2.weight)   2e-7   2e-7   5e-8
#   General, input width 65                 1.5e-6 (spectral_filter.1.0.weight)   3e-7   3e-7   7e-8
#   B = 1 (n = 31)                          6.2e-7 (spectral_filter.0.2.bias)     3e-7   3e-7   3e-8
#   32 channels                             1.1e-6 (att_func.0.weight)            2e-7   4e-7   7e-8
# fp32 alone stays four times inside the gradient bar and thirty times inside the kernel-output bar on
# every case: no seed had to be changed.


def _many_bond_types(rs, ns, N, E):
  """[B, N, N, E]: per bond type a random symmetric 0/1 graph on each molecule's nodes; a random
  spanning tree, its edges dealt over the types, keeps every molecule connected."""
  adjs = np.zeros((len(ns), N, N, E), np.float32)
  for b, n in enumerate(ns):
    for e in range(E):
      up = np.triu(rs.rand(n, n) < 0.12, 1).astype(np.float32)
      adjs[b, :n, :n, e] = up + up.T
    for v in range(1, n):
      u, e = int(rs.randint(0, v)), int(rs.randint(E))
      adjs[b, u, v, e] = adjs[b, v, u, e] = 1.0
  return adjs


@functools.lru_cache(maxsize=None)
def _case(name):
  """cfg, parameters and host inputs of a case (numpy): seeds as in test_forward_edge_shapes."""
  B, N, nmin, nmax, K, short, long_, kind, din, dout, layers, bonds, general = CASES[name]
  cfg = dict(num_atom=9, num_bond_type=bonds, short_diffusion_dist=short, long_diffusion_dist=long_,
             num_eig_vec=K, spectral_filter_kind=kind, input_dim=din, hidden_dim=[128] * layers,
             output_dim=dout, num_layer=layers)
  P = oracle.make_lanczosnet_params(cfg, 100 + N + K, general=general)
  b = draw_batch(B, seed=N * 7 + K, n_min=nmin, n_max=nmax, N=N, num_atom=9, num_bond_type=min(bonds, 6),
                 num_label=dout)
  ns = [int(n) for n in b['n_nodes']]
  adjs = b['adjs']
  if bonds > 6:
    adjs = _many_bond_types(np.random.RandomState(N * 7 + K + 1), ns, N, bonds)
  L = np.zeros((B, N, N, bonds + 1), np.float32)
  Dl, Vl = [], []
  for i, n in enumerate(ns):
    simple = (adjs[i, :n, :n].sum(axis=2) > 0).astype(np.float64)
    assert (np.linalg.matrix_power(simple + np.eye(n), n) > 0).all(), 'connected'
    L[i, :n, :n] = oracle.laplacian_multi_l4(adjs[i, :n, :n])
    if bonds > 6:   # (graphs of different types may share an edge: channel 0 is the 0/1 union's)
      L[i, :n, :n, 0] = oracle.laplacian_l4(simple)
    e, V, _ = oracle.graph_laplacian_eigs(simple, graph_laplacian_type='L4')
    Dl.append(e); Vl.append(V)
  D, V = oracle.collate_eigs(Dl, Vl, N, K)
  if general:
    X = np.random.RandomState(N * 7 + K + 2).randn(B, N, din).astype(np.float32) * b['node_mask'][:, :, None]
  else:
    X = b['node_feat']
  return dict(cfg=cfg, P=P, general=general, X=X, L=L, D=D, V=V, mask=b['node_mask'], label=b['label'], ns=ns)


def _host_net(c):
  """The module on the host: parameter names and order, `loss_func`, `_torch_forward` (plain torch)."""
  from lanczosnet_amd.model import LanczosNet, LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  net = (LanczosNetGeneral if c['general'] else LanczosNet)(make_model_config(c['cfg'], general=c['general']))
  net.load_state_dict({k: torch.from_numpy(v) for k, v in c['P'].items()})
  return net


def _truth(net, X, L, D, V, mask, label, dtype=torch.float64, objective=None, inputs=False):
  """The reference's forward (model/lanczos_net.py:143-197, model/lanczos_net_general.py) restated in
  `dtype` from the raw parameters, with autograd.  Returns (loss, parameter gradients by name,
  [dLoss/dout_l] per conv layer (pre-activation), dLoss/dX_0).  objective: a callable score -> scalar in place
  of the module's loss; inputs: a fifth value, dLoss/d(D, V) by name."""
  P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in net.named_parameters()}
  B, N = mask.shape
  Lc = L.to(dtype).permute(0, 3, 1, 2)
  Dd, Vd = (t.to(dtype).clone().requires_grad_(True) for t in (D, V))
  x0 = X.to(dtype).clone().requires_grad_(True) if net.general else P['embedding.weight'][X]
  S, nl = net.num_scale_long, net.num_layer
  pows = torch.stack([Dd ** p for p in net.long_diffusion_dist], dim=2) if S else None
  state, outs = x0, []
  for t in range(nl):
    W, bias = P['filter.%d.weight' % t], P['filter.%d.bias' % t]
    Wc = W.view(W.shape[0], -1, state.shape[2])       # column blocks in the reference's order
    assert Wc.shape[1] == net.num_scale_short + S + Lc.shape[1]
    out, c = bias.view(1, 1, -1).expand(B, N, -1), 0
    for p in net.short_diffusion_dist:                # 1. L_0^p (X W_c^T)
      z = state @ Wc[:, c].t()
      for _ in range(p):
        z = Lc[:, 0] @ z
      out, c = out + z, c + 1
    if S:                                             # 2. V diag(G_s) V^T (X W_c^T)
      G = pows
      if net.spectral_filter_kind == 'MLP':
        h = pows.reshape(-1, S)
        for i in (0, 2, 4, 6):
          h = h @ P['spectral_filter.%d.%d.weight' % (t, i)].t() + P['spectral_filter.%d.%d.bias' % (t, i)]
          h = torch.relu(h) if i < 6 else h
        G = h.view(B, -1, S)
      for s in range(S):
        out, c = out + Vd @ (G[:, :, s:s + 1] * (Vd.transpose(1, 2) @ (state @ Wc[:, c].t()))), c + 1
    for e in range(Lc.shape[1]):                      # 3. the E + 1 operator channels
      out, c = out + Lc[:, e] @ (state @ Wc[:, c].t()), c + 1
    outs.append(out)
    state = torch.relu(out)
  y = (state @ P['filter.%d.weight' % nl].t() + P['filter.%d.bias' % nl]) * \
      torch.sigmoid(state @ P['att_func.0.weight'].t() + P['att_func.0.bias'])
  m = (mask != 0).to(dtype).unsqueeze(2)
  score = (y * m).sum(dim=1) / m.sum(dim=1)
  loss = net.loss_func(score, label.to(dtype)) if objective is None else objective(score)
  names = list(P)
  g = torch.autograd.grad(loss, [P[k] for k in names] + outs + [x0], retain_graph=inputs)
  res = loss.detach(), dict(zip(names, g[:len(names)])), list(g[len(names):-1]), g[-1]
  if not inputs:
    return res
  return res + (dict(zip('DV', torch.autograd.grad(loss, [Dd, Vd], allow_unused=True))),)


def _host_inputs(c):
  return tuple(torch.from_numpy(np.ascontiguousarray(c[k])) for k in ('X', 'L', 'D', 'V', 'mask', 'label'))


@functools.lru_cache(maxsize=None)
def _truth_of(name):
  """float64 truth of a case, computed once on the host: (loss, parameter gradients, dout_l, dX_0) on
  the device, never written to afterwards."""
  c = _case(name)
  loss, g, douts, dx0 = _truth(_host_net(c), *_host_inputs(c))
  return float(loss), {k: v.to(DEV) for k, v in g.items()}, [d.to(DEV) for d in douts], dx0.to(DEV)


def _device(name):
  c = _case(name)
  net = _model(c['cfg'], c['P'], general=c['general']).train()
  net.backward_impl = 'hip'
  X, L, D, V, mask, label = (_t(c[k]) for k in ('X', 'L', 'D', 'V', 'mask', 'label'))
  assert net._fused_backward_supported()
  assert net._route(L.shape[1], V.shape[2], L.shape[3], True, False, False) == 'fused_train_hip'
  return net, (X, L, D, V, mask, label)


def _hip_step(net, args):
  from lanczosnet_amd import ops
  loss, g = _step(net, *args)
  assert net.last_route == 'fused_train_hip'
  assert ops.last_kernel().startswith(KERNEL), ops.last_kernel()
  return loss, g


def _meets_the_bar(name, tag, loss, g):
  loss64, truth, _, _ = _truth_of(name)
  e = _deviation(g, truth)
  assert set(g) == set(truth)
  assert abs(float(loss) - loss64) < 1e-5 * abs(loss64), (tag, float(loss), loss64)
  assert e[0] < 1e-5, (tag, e)
  return e, abs(float(loss) - loss64) / abs(loss64)


# ---- 2. parameter gradients at edge shapes
@pytest.mark.parametrize('name', IDS, ids=IDS)
def test_parameter_gradients_match_float64_autograd(name):
  net, args = _device(name)
  loss, g = _hip_step(net, args)
  net.backward_impl = 'torch'
  loss_t, g_t = _step(net, *args)
  assert net.last_route == 'fused_train_torch'
  loss64, truth, _, _ = _truth_of(name)
  e_hip, e_torch = _deviation(g, truth), _deviation(g_t, truth)
  print('%s: gradients vs float64 autograd, worst of |g|: HIP %.2e (%s), torch route %.2e (%s); loss %.2e / %.2e'
        % (name, e_hip[0], e_hip[1], e_torch[0], e_torch[1], abs(float(loss) - loss64) / abs(loss64),
           abs(float(loss_t) - loss64) / abs(loss64)))
  assert all(float(v.norm()) > 0 for v in truth.values())   # (no case rests on the exact-zero rule alone)
  _meets_the_bar(name, name, loss, g)


# ---- 3. the input-gradient kernel's own outputs
@pytest.fixture
def launches(monkeypatch):
  """The buffers every call of ops.lanczosnet_input_grad during a test was given."""
  from lanczosnet_amd import ops
  calls, real = [], ops.lanczosnet_input_grad

  def kept(plan, Lp, V, G, mask_u8, act, dy, dx0, tiling, row_off=None, dy_compact=None, dbias_part=None):
    real(plan, Lp, V, G, mask_u8, act, dy, dx0, tiling, row_off=row_off, dy_compact=dy_compact,
         dbias_part=dbias_part)
    calls.append(dict(plan=plan, dy=dy, dx0=dx0, tiling=tiling, row_off=row_off, dy_compact=dy_compact,
                      dbias_part=dbias_part))
  monkeypatch.setattr(ops, 'lanczosnet_input_grad', kept)
  return calls


@pytest.mark.parametrize('name', ['full tile, K = 32', 'General, input width 65 (pads to 128)'])
def test_input_gradient_kernel_outputs(name, launches):
  from lanczosnet_amd import ops
  c = _case(name)
  net, args = _device(name)
  _hip_step(net, args)
  assert len(launches) == 1
  k = launches[0]
  dy, dx0, dyc, dbp = k['dy'], k['dx0'], k['dy_compact'], k['dbias_part']
  _, _, douts, dx0_true = _truth_of(name)
  ns, Lnum = c['ns'], net.num_layer
  B, N = c['mask'].shape
  din, din0p = c['cfg']['input_dim'], k['plan']['din0']
  assert tuple(dy.shape) == (Lnum, B, 32, 128) and tuple(dx0.shape) == (B, 32, din0p) and din0p % 64 == 0
  # dy: every layer's pre-activation gradient; rows n_b .. 31 exactly zero
  for la in range(Lnum):
    got = torch.cat([dy[la][b, :n] for b, n in enumerate(ns)]).cpu().numpy()
    ref = torch.cat([douts[la][b, :n] for b, n in enumerate(ns)]).cpu().numpy()
    e = rel_err(got, ref)
    print('%s: dY_%d vs float64 %.2e' % (name, la, e))
    assert e < 1e-5, (la, e)
    for b, n in enumerate(ns):
      assert not douts[la][b, n:].any()            # (the truth's own padded rows)
      assert not dy[la][b, n:].any(), (la, b)
  # dx0: real rows and columns; padded rows and columns din .. din0p - 1 exactly zero
  got = torch.cat([dx0[b, :n, :din] for b, n in enumerate(ns)]).cpu().numpy()
  ref = torch.cat([dx0_true[b, :n] for b, n in enumerate(ns)]).cpu().numpy()
  e = rel_err(got, ref)
  print('%s: dX_0 vs float64 %.2e' % (name, e))
  assert e < 1e-5, e
  assert not dx0[:, :, din:].any()
  for b, n in enumerate(ns):
    assert not dx0[b, n:].any(), b
  # dy_compact: row offsets from the mask (exclusive scan of the node counts), bit-equal copies.  The
  # input-gradient kernel writes layers 0 .. L-2; the last layer's copy is lnz_head_backward's.
  assert [int(r.sum()) for r in c['mask']] == ns and all(c['mask'][b, :n].all() for b, n in enumerate(ns))
  off = np.concatenate([[0], np.cumsum(ns)])
  assert tuple(dyc.shape) == (Lnum, int(off[-1]), 128)
  assert k['row_off'].cpu().tolist() == off[:-1].tolist()
  for la in range(Lnum):
    for b, n in enumerate(ns):
      assert torch.equal(dyc[la][off[b]:off[b] + n], dy[la][b, :n]), (la, b)
  # dbias_part: per-strip column sums of dY_l, l <= L-2 (the last layer's come from the head's backward)
  strips = k['tiling'][0].strips
  n_strips = int(strips[(strips.numel() - 1) // ops.STRIP_INTS * ops.STRIP_INTS])
  assert 1 <= n_strips <= dbp.shape[0] and tuple(dbp.shape[1:]) == (Lnum, 128)
  assert not dbp[n_strips:].any() and not dbp[:, Lnum - 1].any()
  for la in range(Lnum - 1):
    ref = torch.cat([douts[la][b, :n] for b, n in enumerate(ns)]).sum(dim=0)
    err = float((dbp.sum(dim=0)[la].double() - ref).norm() / ref.norm())
    print('%s: column sums of dY_%d vs float64 %.2e of their norm' % (name, la, err))
    assert err < 1e-5, (la, err)


# ---- 4. the switches inside the backward
@pytest.mark.parametrize('variant', ['default', 'train_static_rows', 'head_grad_impl torch', 'LANCZOSNET_DGAINS torch'])
def test_backward_switches_meet_the_same_bar(variant, monkeypatch):
  """Dead eigen slots (K = 20 > n) and the smallest row count (one-node molecules): the graph-capture
  row masking, the head's gradient by autograd, the gain gradient by library GEMMs.  For the MLP
  tensors this also shows that running the MLP backward on the live eigen rows only loses nothing."""
  name = 'one-node molecules, K > n, one output'
  net, args = _device(name)
  if variant == 'train_static_rows':
    net.train_static_rows = True
  elif variant == 'head_grad_impl torch':
    net.head_grad_impl = 'torch'
  elif variant == 'LANCZOSNET_DGAINS torch':
    monkeypatch.setenv('LANCZOSNET_DGAINS', 'torch')
  assert net.head_grad_impl == ('torch' if variant == 'head_grad_impl torch' else 'hip')
  assert net.mlp_grad_impl == 'hip'
  loss, g = _hip_step(net, args)
  e, el = _meets_the_bar(name, variant, loss, g)
  print('%s, %s: gradients vs float64 autograd, worst of |g|: HIP %.2e (%s); loss %.2e' % (name, variant, e[0], e[1], el))
