"""Helper of the MPNN training tests (not a test): the backward formulas of csrc/mpnn_grad.hip written out in
torch, in the dtype of their operands, next to the float64 autograd through tests/mpnn_mirror.py that they are
held to, the kink condition every kernel-level case has to meet, the case table of the GPU tests with its
seeds, and the differentiable restatement of the whole net the module tests differentiate.

One step, from S = S_t and dS' = dL/dS_{t+1} (P_c, Q_c, R_c, M_c, gi, gh, r, z, n recomputed as the forward does):
    dn = dS' (1 - z) ; dz = dS' (S - n) ; dS = dS' z
    pn = dn (1 - n^2) ; pz = dz z (1 - z) ; pr = pn gh_n r (1 - r) ; pq = pn r
    dgi = [pr, pz, pn] ; dgh = [pr, pz, pq] ; dS += dgh W_hh
    per channel c: dM_c = dgi W_ih[:, cD:(c+1)D] ('avg': then divided by deg_c[a] + FLT_EPSILON) ;
                   dR_c = dM_c W2_c ; act_c[a, b, h] = edge (a, b, c) and Q_c[a, h] + P_c[b, h] > 0 ;
                   dQ_c[a, h] = dR_c[a, h] #{b: act_c[a, b, h]} ; dP_c[b, h] = sum_a act_c[a, b, h] dR_c[a, h] ;
                   dS += dP_c W1n_c + dQ_c W1s_c
    dW_ih = dgi^T cat_c M_c, db_ih = sum dgi ; dW_hh = dgh^T S, db_hh = sum dgh ; dW2_c = dM_c^T R_c,
    db2_c = sum_a deg_c[a] dM_c[a] ; dW1_c = [dP_c^T S | dQ_c^T S], db1_c = sum dQ_c          (sums over all rows)

The ReLU kinks: the gradient jumps where an edge pre-activation Q_c[a, h] + P_c[b, h] crosses zero, and a
float32 evaluation that lands on the other side of zero from float64 is off by a whole term — in the kernel and
in the CPU float32 reference alike.  So every kernel-level case is kink-free (`kink_free`, from `kink_figures`): in float64,
over every step, the smallest |pre-activation| on an edge is at least 4 x the largest |pre32 - pre64| of the
eight float32 evaluations of `permutations`.  The seeds (and, for the wide cases, the low edge densities) of
STEP_CASES and of the other draws below were chosen so that the float64 reference alone meets this; each case
stays at or below about 130 k edge pre-activations (edges x 64 x steps) — larger draws do not come close."""
import numpy as np
import torch

import mpnn_mirror as M

HIDDEN = M.HIDDEN
EPS = M.EPS
STEP_NAMES = ('dS', 'dW1', 'db1', 'dW2', 'db2', 'dWih', 'dbih', 'dWhh', 'dbhh')
KINK_RATIO = 4.0

# (N, C, D, B, steps, agg, row padding, how L reaches the kernel) -> (seed, edge density): the cases of
# tests/test_gpu_mpnn_train.py.  B = 14 at N = 5 gives tiles of 6, 6, 2 molecules, B = 7 at N = 11 tiles of
# 2, 2, 2, 1 (a tile holds floor(32 / N) molecules).  The seeds: the first of 7000, 7001, .. that meets
# KINK_RATIO with the density given (tools/mpnn_grad_reference_spread.py --seeds looks for them).
STEP_CASES = [
    (1, 1, 32, 1, 1, 'sum', 0, 'plain'),
    (5, 2, 32, 3, 2, 'avg', 0, 'plain'),
    (16, 7, 128, 3, 1, 'avg', 8, 'plain'),
    (17, 2, 64, 1, 3, 'sum', 0, 'sliced'),
    (31, 2, 32, 3, 2, 'avg', 4, 'expanded'),
    (32, 8, 128, 2, 1, 'avg', 0, 'plain'),
    (32, 1, 96, 2, 3, 'sum', 0, 'plain'),
    (5, 3, 96, 14, 3, 'avg', 4, 'plain'),
    (11, 2, 64, 7, 3, 'sum', 0, 'plain'),
]
CASE_DRAW = {
    (1, 1, 32, 1, 1, 'sum'): (7000, 0.3),
    (5, 2, 32, 3, 2, 'avg'): (7000, 0.3),
    (16, 7, 128, 3, 1, 'avg'): (7000, 0.2),
    (17, 2, 64, 1, 3, 'sum'): (7000, 0.3),
    (31, 2, 32, 3, 2, 'avg'): (7000, 0.12),
    (32, 8, 128, 2, 1, 'avg'): (7000, 0.04),
    (32, 1, 96, 2, 3, 'sum'): (7007, 0.25),
    (5, 3, 96, 14, 3, 'avg'): (7000, 0.3),
    (11, 2, 64, 7, 3, 'sum'): (7001, 0.3),
}
# the other kernel-level draws of the GPU tests: name -> (seed, N, C, D, B, steps, density)
SATURATED_DRAW, SATURATED_SCALE = (7121, 17, 2, 64, 3, 2, 0.3), 5.0
EDGE_DRAW = (7200, 9, 3, 32, 4, 2, 0.3)
REPEAT_DRAW = (7300, 13, 3, 64, 5, 1, 0.3)


def draw_operands(seed, B, N, C, D, scale=1.0, density=0.3):
  """(state0, L, the eight operands): the draw of tests/test_gpu_mpnn.py — Xavier-bounded weights (times
  `scale`), biases +-0.1, a sparse ASYMMETRIC L with negative entries (only != 0 matters), a self loop, a row
  with all N bits set and (N > 1) a row without an edge"""
  g = torch.Generator().manual_seed(seed)
  u = lambda bound, *s: (torch.rand(*s, generator=g) * 2 - 1) * bound  # noqa: E731
  xav = lambda *s: u(scale * float(np.sqrt(6.0 / (s[-1] + s[-2]))), *s)  # noqa: E731
  S = 0.5 * torch.randn(B, N, D, generator=g)
  L = (torch.rand(B, N, N, C, generator=g) < density).float() * (torch.rand(B, N, N, C, generator=g) - 0.5)
  L[B - 1, N // 2, N // 2, C - 1] = 0.5       # a self loop
  L[0, 0, :, 0] = -0.25                       # all N bits of a row (32 at N = 32), its self loop among them
  if N > 1:
    L[0, N - 1] = 0.0                         # a row without an edge in every channel
  W = [xav(C, HIDDEN, 2 * D), u(0.1, C, HIDDEN), xav(C, D, HIDDEN), u(0.1, C, D), xav(3 * D, C * D),
       u(0.1, 3 * D), xav(3 * D, D), u(0.1, 3 * D)]
  return S, L, W


def step_case_inputs(N, C, D, B, steps, agg, lkind='plain'):
  """(S_0, L as the formulas see it, the eight operands, dS_T) of a case of STEP_CASES: fixed seeds, CPU"""
  seed, density = CASE_DRAW[(N, C, D, B, steps, agg)]
  S, L, W = draw_operands(seed, B, N, C, D, density=density)
  if lkind == 'expanded':   # one channel, seen C times through a zero stride
    L = L[..., :1].expand(B, N, N, C).contiguous()
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(11 + N))
  return S, L, W, dST


def edge_case():
  """(S_0, L with a negative and two NaN entries, what `L != 0` says of it as 0 / 1, the eight operands, dS_T):
  a row without an edge in every channel, a whole channel of a molecule without an edge"""
  seed, N, C, D, B, _, density = EDGE_DRAW
  S, L, W = draw_operands(seed, B, N, C, D, density=density)
  L[0, 2] = 0.0                                                # a row without an edge in every channel
  L[1, :, :, 1] = 0.0                                          # a whole channel without an edge
  L[2, 3, 4, 0], L[2, 4, 3, 2], L[3, 0, 0, 1] = -0.5, float('nan'), float('nan')
  ones = (torch.isnan(L) | (L != 0)).float()
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(13))
  return S, L, ones, W, dST


def saturated_case():
  """(S_0, L, the eight operands, dS_T, the gate pre-activations gi + gh [.., :2 D] and gi [.., 2 D:] of the first
  step in float64): the weights scaled until the gate pre-activations pass +-100"""
  seed, N, C, D, B, _, density = SATURATED_DRAW
  S, L, W = draw_operands(seed, B, N, C, D, scale=SATURATED_SCALE, density=density)
  S = 2.0 * S
  dST = torch.randn(B, N, D, generator=torch.Generator().manual_seed(12))
  Sd, Wd = S.double(), [w.double() for w in W]
  A, deg = M._edges(L.double(), torch.float64)
  gi = torch.cat([x[3] for x in _messages(Sd, A, deg, *Wd[:4], 'avg')], dim=2) @ Wd[4].t() + Wd[5]
  gh = Sd @ Wd[6].t() + Wd[7]
  return S, L, W, dST, (gi + gh)[..., :2 * D], gi[..., 2 * D:]


# --------------------------------------------------------------------------------------------- forward
def _messages(S, A, deg, W1, b1, W2, b2, agg):
  """-> per channel (P_c [B, N, 64], Q_c [B, N, 64], R_c [B, N, 64], M_c [B, N, D]) of the factored form"""
  D = S.shape[2]
  out = []
  for c in range(A.shape[1]):
    Pn = S @ W1[c][:, :D].t()
    Qs = S @ W1[c][:, D:].t() + b1[c]
    R = (torch.relu(Qs.unsqueeze(2) + Pn.unsqueeze(1)) * A[:, c].unsqueeze(3)).sum(dim=2)
    Mc = R @ W2[c].t() + deg[:, c] * b2[c]
    if agg == 'avg':
      Mc = Mc / (deg[:, c] + EPS)
    out.append((Pn, Qs, R, Mc))
  return out


def propagate(S, L, W1, b1, W2, b2, Wih, bih, Whh, bhh, num_prop, agg='avg', order=None, trajectory=False):
  """mpnn_mirror.propagate_factored with gi summed channel by channel in `order` (None: that function itself,
  one product with the concatenated message).  trajectory: the list S_0 .. S_T instead of S_T"""
  if order is None and not trajectory:
    return M.propagate_factored(S, L, W1, b1, W2, b2, Wih, bih, Whh, bhh, num_prop, agg=agg)
  A, deg = M._edges(L, S.dtype)
  traj = [S]
  for _ in range(num_prop):
    Ms = [x[3] for x in _messages(S, A, deg, W1, b1, W2, b2, agg)]
    if order is None:
      S = M._gru(torch.cat(Ms, dim=2), S, Wih, bih, Whh, bhh)
    else:
      S = M._gru_by_channel(Ms, order, S, Wih, bih, Whh, bhh)
    traj.append(S)
  return traj if trajectory else S


def edge_preactivations(S, L, W1, b1):
  """pre [B, C, N(a), N(b), 64] = Q_c[a] + P_c[b] of the state S and the edge mask [B, C, N, N] (bool)"""
  D = S.shape[2]
  A = (L != 0).permute(0, 3, 1, 2)
  pre = torch.stack([(S @ W1[c][:, D:].t() + b1[c]).unsqueeze(2) + (S @ W1[c][:, :D].t()).unsqueeze(1)
                     for c in range(L.shape[3])], dim=1)
  return pre, A


# -------------------------------------------------------------------------------------------- backward
def step_backward(S, dSn, L, W1, b1, W2, b2, Wih, bih, Whh, bhh, agg='avg', swap_halves=False, transpose_dP=True):
  """-> (dS [B, N, D], dW1 [C, 64, 2 D], db1 [C, 64], dW2 [C, D, 64], db2 [C, D], dWih [3 D, C D], dbih [3 D],
  dWhh [3 D, D], dbhh [3 D]) of one step, by the formulas above.  swap_halves=True takes the own half of W1 for
  the neighbour and the other way round in the data gradient, transpose_dP=False sums dP over the row's own
  edges instead of the edges into it: the mistakes the asymmetric draw exists to catch
  (tests/test_mpnn_train_cpu.py)"""
  B, N, D = S.shape
  C = L.shape[3]
  A, deg = M._edges(L, S.dtype)
  msgs = _messages(S, A, deg, W1, b1, W2, b2, agg)
  Mcat = torch.cat([x[3] for x in msgs], dim=2)
  gi = Mcat @ Wih.t() + bih
  gh = S @ Whh.t() + bhh
  r = torch.sigmoid(gi[..., :D] + gh[..., :D])
  z = torch.sigmoid(gi[..., D:2 * D] + gh[..., D:2 * D])
  ghn = gh[..., 2 * D:]
  n = torch.tanh(gi[..., 2 * D:] + r * ghn)
  dn, dz, dS = dSn * (1 - z), dSn * (S - n), dSn * z
  pn = dn * (1 - n * n)
  pz = dz * (z * (1 - z))
  pr = (pn * ghn) * (r * (1 - r))
  dgi = torch.cat((pr, pz, pn), dim=2)
  dgh = torch.cat((pr, pz, pn * r), dim=2)
  dS = dS + dgh @ Whh
  dW1, db1, dW2, db2 = torch.zeros_like(W1), torch.zeros_like(b1), torch.zeros_like(W2), torch.zeros_like(b2)
  rows = lambda x: x.reshape(B * N, -1)  # noqa: E731
  for c in range(C):
    Pn, Qs, R, _ = msgs[c]
    dM = dgi @ Wih[:, c * D:(c + 1) * D]
    if agg == 'avg':
      dM = dM / (deg[:, c] + EPS)
    dR = dM @ W2[c]                                                             # [B, N, 64]
    act = ((Qs.unsqueeze(2) + Pn.unsqueeze(1)) > 0).to(S.dtype) * A[:, c].unsqueeze(3)   # [B, a, b, 64]
    dQ = dR * act.sum(dim=2)
    if transpose_dP:
      dP = (act * dR.unsqueeze(2)).sum(dim=1)                                   # over a, for every b
    else:
      dP = (act * dR.unsqueeze(2)).sum(dim=2)
    Wn, Ws = W1[c][:, :D], W1[c][:, D:]
    dS = dS + (dP @ Ws + dQ @ Wn if swap_halves else dP @ Wn + dQ @ Ws)
    dW2[c], db2[c] = rows(dM).t() @ rows(R), (rows(deg[:, c]) * rows(dM)).sum(dim=0)
    dW1[c] = torch.cat((rows(dP).t() @ rows(S), rows(dQ).t() @ rows(S)), dim=1)
    db1[c] = rows(dQ).sum(dim=0)
  dWih = rows(dgi).t() @ rows(Mcat)
  dWhh = rows(dgh).t() @ rows(S)
  return dS, dW1, db1, dW2, db2, dWih, rows(dgi).sum(dim=0), dWhh, rows(dgh).sum(dim=0)


def propagate_backward(S0, dST, L, W8, num_prop, agg='avg'):
  """backpropagation through num_prop steps from the trajectory: -> the nine of step_backward, dS = dL/dS_0 and
  the weight gradients summed over the steps (zeros with num_prop = 0)"""
  traj = propagate(S0, L, *W8, num_prop, agg=agg, trajectory=True)
  dS = dST
  acc = [torch.zeros_like(w) for w in W8]
  for t in range(num_prop - 1, -1, -1):
    out = step_backward(traj[t], dS, L, *W8, agg=agg)
    dS = out[0]
    acc = [a + x for a, x in zip(acc, out[1:])]
  return (dS,) + tuple(acc)


def propagate_autograd(S0, dST, L, W8, num_prop, agg='avg', order=None):
  """the same nine gradients by autograd through mpnn_mirror.propagate_factored (order: `propagate`), in the
  operands' dtype (a weight that is never read, num_prop = 0: zeros)"""
  ops = [x.detach().clone().requires_grad_(True) for x in [S0] + list(W8)]
  out = propagate(ops[0], L, *ops[1:], num_prop, agg=agg, order=order)
  gr = torch.autograd.grad(out, ops, dST, allow_unused=True)
  return tuple(torch.zeros_like(x) if v is None else v for v, x in zip(gr, ops))


def permutations(B, N, C, count=8, seed=5):
  """`count` (molecule permutation, node permutation, channel order) triples, the identity first"""
  g = torch.Generator().manual_seed(seed)
  out = [(torch.arange(B), torch.arange(N), list(range(C)))]
  while len(out) < count:
    out.append((torch.randperm(B, generator=g), torch.randperm(N, generator=g),
                torch.randperm(C, generator=g).tolist()))
  return out


def _unpermute(x, pb, pn):
  back = torch.empty_like(x)
  back[pb.unsqueeze(1), pn.unsqueeze(0)] = x
  return back


def propagate_e32(S0, dST, L, W8, truth, num_prop, agg, every=False):
  """per gradient of propagate_autograd: the largest error over eight evaluations of the CPU float32 autograd —
  the operands as given and seven with the molecules, the nodes (rows of S_0 / dS_T, rows and columns of L)
  and the channel order of the gi sum consistently permuted, the gradients un-permuted —, in units of
  max|truth|.  every=True: the list of the eight per gradient instead (what the spread is measured on)"""
  B, N = S0.shape[:2]
  runs = [[] for _ in truth]
  for i, (pb, pn, order) in enumerate(permutations(B, N, L.shape[3])):
    gr = list(propagate_autograd(S0[pb][:, pn], dST[pb][:, pn], L[pb][:, pn][:, :, pn], W8, num_prop, agg,
                                 None if i == 0 else order))
    gr[0] = _unpermute(gr[0], pb, pn)
    for k in range(len(truth)):
      scale = float(truth[k].abs().max())
      runs[k].append(float((gr[k].double() - truth[k]).abs().max()) / scale if scale > 0 else 0.0)
  return runs if every else [max(r) for r in runs]


def kink_figures(S0, L, W8, num_prop, agg):
  """-> (smallest, widest, count): in float64, over every step, the smallest |pre-activation| on an edge; the
  largest |pre32 - pre64| on an edge over the eight float32 evaluations of `permutations` (each against float64
  on the same permuted operands) and every step; the number of edge pre-activations (edges x 64 x steps)"""
  B, N = S0.shape[:2]
  d = lambda x: x.double()  # noqa: E731
  W64 = [d(w) for w in W8]
  smallest, widest, count = float('inf'), 0.0, 0
  for i, (pb, pn, order) in enumerate(permutations(B, N, L.shape[3])):
    Sp, Lp = S0[pb][:, pn], L[pb][:, pn][:, :, pn]
    order = None if i == 0 else order
    t64 = propagate(d(Sp), d(Lp), *W64, num_prop, agg=agg, order=order, trajectory=True)
    t32 = propagate(Sp, Lp, *W8, num_prop, agg=agg, order=order, trajectory=True)
    for t in range(num_prop):
      p64, A = edge_preactivations(t64[t], d(Lp), W64[0], W64[1])
      p32, _ = edge_preactivations(t32[t], Lp, W8[0], W8[1])
      on = A.unsqueeze(4).expand_as(p64)
      if not bool(on.any()):
        continue
      smallest = min(smallest, float(p64[on].abs().min()))
      widest = max(widest, float((p32.double() - p64)[on].abs().max()))
      if i == 0:
        count += int(on.sum())
  return smallest, widest, count


def kink_free(S0, L, W8, num_prop, agg):
  smallest, widest, _ = kink_figures(S0, L, W8, num_prop, agg)
  return smallest >= KINK_RATIO * widest


# ------------------------------------------------------------------------------------------ whole net
def net_forward(Q, cfg, node_feat, L, mask, order=None):
  """mpnn_mirror.forward (factored) on a dict of TENSORS (name -> tensor, any dtype, requires_grad allowed),
  without the detach: differentiable with respect to every entry that is read."""
  m = cfg.model
  C = cfg.dataset.num_bond_type + 1
  dtype = Q['node_embedding.weight'].dtype
  W1 = torch.stack([Q['edge_func.%d.0.weight' % c] for c in range(C)])
  b1 = torch.stack([Q['edge_func.%d.0.bias' % c] for c in range(C)])
  W2 = torch.stack([Q['edge_func.%d.2.weight' % c] for c in range(C)])
  b2 = torch.stack([Q['edge_func.%d.2.bias' % c] for c in range(C)])
  S = Q['node_embedding.weight'][node_feat] @ Q['input_func.0.weight'].t() + Q['input_func.0.bias']
  S = propagate(S, L.to(dtype), W1, b1, W2, b2, Q['update_func.weight_ih'], Q['update_func.bias_ih'],
                Q['update_func.weight_hh'], Q['update_func.bias_hh'], m.num_prop, agg=m.aggregate_type, order=order)
  gates = ('forget_gate', 'input_gate', 'output_gate', 'memory_gate')
  Wg = torch.stack([Q['att_func.LSTM.%s.0.weight' % k] for k in gates])
  bg = torch.stack([Q['att_func.LSTM.%s.0.bias' % k] for k in gates])
  return M.set2vec(S, mask, Wg, bg, Q['att_func.W_1'], Q['att_func.W_2'], Q['output_func.0.weight'],
                   Q['output_func.0.bias'], m.num_step_set2vec)


def net_gradients(P, cfg, batch, dtype, use_mask=True, perm=None):
  """Gradients of the MSE loss with respect to every parameter, as a dict name -> tensor (None where the
  parameter is never read), by autograd through net_forward in `dtype`, and the loss.  perm = (molecules,
  nodes, channel order): the batch consistently permuted (parameter gradients need no un-permuting)."""
  Q = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in P.items()}
  nf = torch.from_numpy(np.asarray(batch['node_feat'])).long()
  L = torch.from_numpy(np.asarray(batch['L']))
  mask = torch.from_numpy(np.asarray(batch['node_mask'])) if use_mask else None
  label = torch.from_numpy(np.asarray(batch['label'])).to(dtype)
  order = None
  if perm is not None:
    pb, pn, order = perm
    nf, L, label = nf[pb][:, pn], L[pb][:, pn][:, :, pn], label[pb]
    mask = None if mask is None else mask[pb][:, pn]
  score = net_forward(Q, cfg, nf, L, mask, order=order)
  loss = torch.nn.functional.mse_loss(score, label)
  names = list(Q)
  gr = torch.autograd.grad(loss, [Q[k] for k in names], allow_unused=True)
  return dict(zip(names, gr)), float(loss.detach())


def net_e32(P, cfg, batch, truth, use_mask=True):
  """per parameter: the largest error of the CPU float32 net_gradients over the eight permutations, in units
  of max|truth| (0 where the truth is None or identically zero)"""
  B, N = np.asarray(batch['node_feat']).shape
  worst = {k: 0.0 for k in truth}
  for i, perm in enumerate(permutations(B, N, cfg.dataset.num_bond_type + 1)):
    gr, _ = net_gradients(P, cfg, batch, torch.float32, use_mask, None if i == 0 else perm)
    for k, t in truth.items():
      if t is None or gr[k] is None:
        continue
      scale = float(t.abs().max())
      if scale > 0:
        worst[k] = max(worst[k], float((gr[k].double() - t).abs().max()) / scale)
  return worst
