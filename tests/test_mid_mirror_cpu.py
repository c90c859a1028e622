"""tests/mid_mirror.py against itself and against float64 autograd, on the host: what keeps the mirror
the GPU tests of the 33..128-node kernels lean on (tests/test_gpu_mid_edges.py) from being wrong.

1. float64 autograd through the mirror's forward reproduces `head_grad` o `input_grad` (dOut of every
   layer, dX0, the head's gradients) and the parameter gradients assembled from `project` the way
   `_MidGraphFusedFunction.backward` assembles them (dW_s = sum_b A^T Q, dW_c = sum_b dOut^T M, db),
   and dG, to 1e-12 relative.
2. CONDITIONING of test_gpu_mid_edges.py: on every case there, the mirror in fp32 stays at least four
   times inside the 1e-5 bar against the mirror in float64 on the same inputs."""
import numpy as np
import pytest
import torch

import mid_mirror as m
import test_gpu_mid_edges as E


def _rel(a, b):
  return float((a - b).abs().max() / b.abs().max())


def _small(C, S, seed):
  rs = np.random.RandomState(seed)
  ns, N, K, din0, nl, dout = [7, 4, 1], 7, 5, 16, 3, 3
  B = len(ns)
  f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
  L, V, mask = np.zeros((B, N, N, C)), np.zeros((B, N, K)), np.zeros((B, N), np.uint8)
  for b, n in enumerate(ns):
    L[b, :n, :n, 0] = E._sym_norm(rs, n, 0.4)
    if C == 2:
      L[b, :n, :n, 1] = rs.randn(n, n) * 0.3   # unequal, and not symmetric
    V[b, :n, :min(n, K)] = np.linalg.qr(rs.randn(n, min(n, K)))[0]
    mask[b, :n] = 1
  mask[0, 2] = 0
  W = [f(rs.randn(128, S + C, d) / np.sqrt((S + C) * d)) for d in [din0] + [128] * (nl - 1)]
  return dict(L=f(L), V=f(V), mask=torch.from_numpy(mask), G=f(rs.uniform(-1, 1, size=(nl, B, S, K))) if S else None,
              X0=f(rs.randn(B, N, din0)), W=W, bias=f(rs.randn(nl, 128) * 0.1),
              Whead=f(rs.randn(dout + 1, 128) / np.sqrt(128)), bhead=f(rs.randn(dout + 1) * 0.1),
              gscore=f(rs.randn(B, dout)), din0=din0)


@pytest.mark.parametrize('C,S', [(2, 3), (1, 0)], ids=['C=2 unequal, S=3', 'C=1, S=0'])
def test_autograd_through_the_forward_reproduces_the_backward_functions(C, S):
  c = _small(C, S, 40 + C)
  req = lambda t: t.clone().requires_grad_(True)
  X0, W, bias, Wh, bh = req(c['X0']), [req(w) for w in c['W']], req(c['bias']), req(c['Whead']), req(c['bhead'])
  G = req(c['G']) if S else None
  # the forward layer by layer, every state a node of the graph; the same numbers as forward()
  X, states = X0, []
  for l in range(len(W)):
    X = m.conv_layer(X, c['L'], c['V'], G[l] if S else None, W[l], bias[l])
    states.append(X)
  score = m.readout(X, c['mask'], Wh, bh)
  st, sc = m.forward(c['X0'], c['L'], c['V'], c['G'], c['mask'], c['W'], c['bias'], c['Whead'], c['bhead'])
  assert torch.equal(st, torch.stack(states).detach()) and torch.equal(sc, score.detach())
  assert all(0.2 < float((s > 0).double().mean()) < 0.8 for s in st)   # (the ReLU masks are no formality)
  leaves = states + [X0] + W + [bias, Wh, bh] + ([G] if S else [])
  g = torch.autograd.grad((score * c['gscore']).sum(), leaves)
  nl = len(W)
  g_states, g_X0, g_W, g_bias, g_Wh, g_bh = g[:nl], g[nl], g[nl + 1:2 * nl + 1], g[2 * nl + 1], g[2 * nl + 2], g[2 * nl + 3]
  # head_grad o input_grad
  d_last, dWh, dbh = m.head_grad(st[-1], c['mask'], c['gscore'], c['Whead'], c['bhead'])
  dOut, dX0 = m.input_grad(d_last, st, c['L'], c['V'], c['G'], c['W'], c['din0'])
  for l in range(nl):
    assert _rel(dOut[l], g_states[l] * (st[l] > 0)) < 1e-12, l
  assert _rel(dX0, g_X0) < 1e-12
  assert _rel(dWh.sum(dim=0), g_Wh) < 1e-12 and _rel(dbh.sum(dim=0), g_bh) < 1e-12
  # the parameter gradients from the projections
  A, Q, M, dG, db = m.project(dOut, st, c['X0'], c['L'], c['V'], c['G'], c['W'])
  dW, dbias = m.param_grads(dOut, A, Q, M, db, c['W'])
  for l in range(nl):
    assert dW[l].shape == g_W[l].shape
    for ch in range(S + C):   # every channel block on its own scale
      assert _rel(dW[l][:, ch], g_W[l][:, ch]) < 1e-12, (l, ch)
    assert _rel(dbias[l], g_bias[l]) < 1e-12, l
  if S:
    assert _rel(dG.transpose(2, 3), g[-1]) < 1e-12
  else:
    assert A is None and Q is None and dG is None


def test_non_finite_ritz_entries_are_read_as_zero():
  c = _small(2, 3, 7)
  V = c['V'].clone()
  V[0, 1, 1], V[1, 0, 2] = float('nan'), float('-inf')
  Vz = torch.where(torch.isfinite(V), V, torch.zeros_like(V))
  args = lambda v: (c['X0'], c['L'], v, c['G'], c['mask'], c['W'], c['bias'], c['Whead'], c['bhead'])
  for a, b in zip(m.forward(*args(V)), m.forward(*args(Vz))):
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize('name', E.IDS, ids=E.IDS)
def test_fp32_alone_stays_four_times_inside_the_bar(name):
  c = E._case(name)
  with torch.no_grad():
    dev = E._deviations(c, E._mirror_chain(c, torch.float32))
  print('%-42s %s' % (name, E._line(dev)))
  assert E._inside(dev, E.BAR / 4), E._worst_of(dev)
