"""Helper of the GGNN training tests (not a test): the backward formulas of csrc/ggnn_grad.hip written out
in torch, in the dtype of their operands, next to the float64 autograd through tests/ggnn_mirror.py that
they are held to, and the differentiable restatement of the whole net the module tests differentiate.

One step, from S = S_t and dS' = dL/dS_{t+1} (H_c, M_c, A_c, gi, gh, r, z, n recomputed as the forward does):
    dn = dS' (1 - z) ; dz = dS' (S - n) ; dS = dS' z
    dn_pre = dn (1 - n^2) ; dz_pre = dz z (1 - z) ; dr_pre = dn_pre gh_n r (1 - r)
    dgi = [dr_pre, dz_pre, dn_pre] ; dgh = [dr_pre, dz_pre, dn_pre r] ; dS += dgh W_hh
    per channel c: dA_c = dgi W_ih[:, cD:(c+1)D] ; dM_c = Â_c^T dA_c per molecule ;
                   dHpre_c = (dM_c W2_c) [H_c > 0] ; dS += dHpre_c W1_c
    dW_hh = dgh^T S, db_hh = sum dgh ; dW_ih = dgi^T cat_c A_c, db_ih = sum dgi ;
    dW2_c = dM_c^T H_c, db2_c = sum dM_c ; dW1_c = dHpre_c^T S, db1_c = sum dHpre_c      (sums over all rows)
Readout, per row i of the mask (cnt of them):
    dy = dscore / cnt ; do = dy g ; dzg = (sum_p dy[p] o[p]) g (1 - g) ; dS_T[i] = Wo^T do + wg dzg"""
import numpy as np
import torch

import ggnn_mirror as G

STEP_NAMES = ('dS', 'dW1', 'db1', 'dW2', 'db2', 'dWih', 'dbih', 'dWhh', 'dbhh')
RO_NAMES = ('dS', 'dWo', 'dbo', 'dwg', 'dbg')


def draw_operands(seed, B, N, C, D, P=16, scale=1.0, density=0.3):
  """(state0, L, the twelve operands): the draw of tests/test_gpu_ggnn.py — Xavier-bounded weights, biases
  +-0.1, a sparse ASYMMETRIC L with negative entries (only != 0 matters)"""
  g = torch.Generator().manual_seed(seed)
  u = lambda bound, *s: (torch.rand(*s, generator=g) * 2 - 1) * bound  # noqa: E731
  xav = lambda *s: u(scale * float(np.sqrt(6.0 / (s[-1] + s[-2]))), *s)  # noqa: E731
  S = 0.5 * torch.randn(B, N, D, generator=g)
  L = (torch.rand(B, N, N, C, generator=g) < density).float() * (torch.rand(B, N, N, C, generator=g) - 0.5)
  W = [xav(C, G.HIDDEN, D), u(0.1, C, G.HIDDEN), xav(C, D, G.HIDDEN), u(0.1, C, D), xav(3 * D, C * D), u(0.1, 3 * D),
       xav(3 * D, D), u(0.1, 3 * D), xav(P, D), u(0.1, P), xav(1, D), u(0.1, 1)]
  return S, L, W


def step_backward(S, dSn, L, W1, b1, W2, b2, Wih, bih, Whh, bhh, agg='avg', transpose_dM=True):
  """-> (dS [B, N, D], dW1 [C, 128, D], db1 [C, 128], dW2 [C, D, 128], db2 [C, D], dWih [3 D, C D], dbih [3 D],
  dWhh [3 D, D], dbhh [3 D]) of one GRU step, by the formulas above.  transpose_dM=False leaves the transpose
  of the aggregate out: the mistake the asymmetric draw exists to catch (tests/test_ggnn_train_cpu.py)"""
  B, N, D = S.shape
  C = L.shape[3]
  A = G.adjacency(L, agg, S.dtype)
  H = [torch.relu(S @ W1[c].t() + b1[c]) for c in range(C)]
  Ac = [A[:, c] @ (H[c] @ W2[c].t() + b2[c]) for c in range(C)]
  gi = None
  for c in range(C):
    part = Ac[c] @ Wih[:, c * D:(c + 1) * D].t()
    gi = part if gi is None else gi + part
  gi = gi + bih
  gh = S @ Whh.t() + bhh
  r = torch.sigmoid(gi[..., :D] + gh[..., :D])
  z = torch.sigmoid(gi[..., D:2 * D] + gh[..., D:2 * D])
  ghn = gh[..., 2 * D:]
  n = torch.tanh(gi[..., 2 * D:] + r * ghn)
  dn, dz, dS = dSn * (1 - z), dSn * (S - n), dSn * z
  dnp = dn * (1 - n * n)
  dzp = dz * (z * (1 - z))
  drp = (dnp * ghn) * (r * (1 - r))
  dgi = torch.cat((drp, dzp, dnp), dim=2)
  dgh = torch.cat((drp, dzp, dnp * r), dim=2)
  dS = dS + dgh @ Whh
  dW1, db1, dW2, db2 = torch.zeros_like(W1), torch.zeros_like(b1), torch.zeros_like(W2), torch.zeros_like(b2)
  rows = lambda x: x.reshape(B * N, -1)  # noqa: E731
  for c in range(C):
    dA = dgi @ Wih[:, c * D:(c + 1) * D]
    dM = (A[:, c].transpose(1, 2) if transpose_dM else A[:, c]) @ dA
    dHpre = (dM @ W2[c]) * (H[c] > 0).to(S.dtype)
    dS = dS + dHpre @ W1[c]
    dW2[c], db2[c] = rows(dM).t() @ rows(H[c]), rows(dM).sum(dim=0)
    dW1[c], db1[c] = rows(dHpre).t() @ rows(S), rows(dHpre).sum(dim=0)
  dWih = rows(dgi).t() @ rows(torch.cat(Ac, dim=2))
  dWhh = rows(dgh).t() @ rows(S)
  return dS, dW1, db1, dW2, db2, dWih, rows(dgi).sum(dim=0), dWhh, rows(dgh).sum(dim=0)


def propagate_backward(S0, dST, L, W8, num_prop, agg='avg'):
  """backpropagation through num_prop steps from the trajectory: -> the nine of step_backward, dS = dL/dS_0 and
  the weight gradients summed over the steps (zeros with num_prop = 0)"""
  traj = [S0]
  for _ in range(num_prop):
    traj.append(G.propagate(traj[-1], L, *W8, 1, agg=agg))
  dS = dST
  acc = [torch.zeros_like(w) for w in W8]
  for t in range(num_prop - 1, -1, -1):
    out = step_backward(traj[t], dS, L, *W8, agg=agg)
    dS = out[0]
    acc = [a + x for a, x in zip(acc, out[1:])]
  return (dS,) + tuple(acc)


def readout_backward(S, mask, Wo, bo, wg, bg, dscore):
  """-> (dS [B, N, D], dWo [P, D], dbo [P], dwg [D], dbg [1])"""
  B, N, D = S.shape
  o = S @ Wo.t() + bo
  g = torch.sigmoid(S @ wg.reshape(-1, 1) + bg)               # [B, N, 1]
  mk = torch.ones(B, N, 1, dtype=S.dtype) if mask is None else (mask != 0).to(S.dtype).unsqueeze(2)
  dy = (dscore / mk.sum(dim=1)).unsqueeze(1) * mk              # [B, N, P], zero outside the mask
  do = dy * g
  dzg = (dy * o).sum(dim=2, keepdim=True) * g * (1 - g)
  dS = do @ Wo + dzg * wg.reshape(1, 1, -1)
  return (dS, torch.einsum('bip,bid->pd', do, S), do.sum(dim=(0, 1)), (dzg * S).sum(dim=(0, 1)), dzg.sum().reshape(1))


def propagate_autograd(S0, dST, L, W8, num_prop, agg='avg', order=None):
  """the same nine gradients by autograd through ggnn_mirror.propagate, in the operands' dtype (a weight that
  is never read, num_prop = 0: zeros)"""
  ops = [x.detach().clone().requires_grad_(True) for x in [S0] + list(W8)]
  out = G.propagate(ops[0], L, *ops[1:], num_prop, agg=agg, order=order)
  gr = torch.autograd.grad(out, ops, dST, allow_unused=True)
  return tuple(torch.zeros_like(x) if v is None else v for v, x in zip(gr, ops))


def readout_autograd(S, mask, Wo, bo, wg, bg, dscore):
  ops = [x.detach().clone().requires_grad_(True) for x in (S, Wo, bo, wg, bg)]
  s = G.readout(ops[0], mask, ops[1], ops[2], ops[3], ops[4])
  gr = torch.autograd.grad(s, ops, dscore)
  return gr[0], gr[1], gr[2], gr[3].reshape(-1), gr[4]


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
  for pb, pn, order in permutations(B, N, L.shape[3]):
    gr = list(propagate_autograd(S0[pb][:, pn], dST[pb][:, pn], L[pb][:, pn][:, :, pn], W8, num_prop, agg, order))
    gr[0] = _unpermute(gr[0], pb, pn)
    for k in range(len(truth)):
      scale = float(truth[k].abs().max())
      runs[k].append(float((gr[k].double() - truth[k]).abs().max()) / scale if scale > 0 else 0.0)
  return runs if every else [max(r) for r in runs]


def readout_e32(S, mask, Wo, bo, wg, bg, dscore, truth):
  B, N = S.shape[:2]
  worst = [0.0] * 5
  for pb, pn, _ in permutations(B, N, 1):
    gr = list(readout_autograd(S[pb][:, pn], None if mask is None else mask[pb][:, pn], Wo, bo, wg, bg, dscore[pb]))
    gr[0] = _unpermute(gr[0], pb, pn)
    for k in range(5):
      scale = float(truth[k].abs().max())
      if scale > 0:
        worst[k] = max(worst[k], float((gr[k].double() - truth[k]).abs().max()) / scale)
  return worst


# ------------------------------------------------------------------------------------------ whole net
def net_forward(Q, cfg, node_feat, L, mask, order=None):
  """ggnn_mirror.forward on a dict of TENSORS (name -> tensor, any dtype, requires_grad allowed), without the
  detach: differentiable with respect to every entry that is read."""
  m = cfg.model
  C = cfg.dataset.num_bond_type + 1
  dtype = Q['embedding.weight'].dtype
  W1 = torch.stack([Q['msg_func.%d.0.weight' % c] for c in range(C)])
  b1 = torch.stack([Q['msg_func.%d.0.bias' % c] for c in range(C)])
  W2 = torch.stack([Q['msg_func.%d.2.weight' % c] for c in range(C)])
  b2 = torch.stack([Q['msg_func.%d.2.bias' % c] for c in range(C)])
  S = Q['embedding.weight'][node_feat] @ Q['input_func.0.weight'].t() + Q['input_func.0.bias']
  S = G.propagate(S, L.to(dtype), W1, b1, W2, b2, Q['update_func.weight_ih'], Q['update_func.bias_ih'],
                  Q['update_func.weight_hh'], Q['update_func.bias_hh'], m.num_prop, agg=m.aggregate_type,
                  update=m.update_func, order=order)
  return G.readout(S, mask, Q['output_func.0.weight'], Q['output_func.0.bias'], Q['att_func.0.weight'],
                   Q['att_func.0.bias'])


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
