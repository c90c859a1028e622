"""Helper of the GAT training tests (not a test): the backward formulas of csrc/gat_grad.hip written
out in torch, in the dtype of their operands, next to the autograd of tests/gat_mirror.py that they
are held to, and the differentiable restatement of the whole net the module tests differentiate.

Per (molecule, block k = c H + h), P the attention block of the forward (softmax over the ROW index):
    dO = dOut * elu'(.) ; dP[i][j] = dO[i] . Wh[j] ; t[j] = sum_i P dP ; dE = P (dP - t)
    dZ = dE * (s1[i] + s2[j] > 0 ? 1 : 0.2) ; ds1[i] = sum_j dZ ; ds2[j] = sum_i dZ
    dWh[j] = sum_i P[i][j] dO[i] + ds1[j] a1 + ds2[j] a2
    da1 = sum ds1[i] Wh[i] ; da2 = sum ds2[i] Wh[i] ; db1 = sum ds1 ; db2 = sum ds2 ; dbias = sum dO
Readout, per row i of the mask (cnt of them):
    dy = dscore / cnt ; do = dy g ; dzg = (sum_p dy[p] o[p]) g (1 - g) ; dx = Wo^T do + wg dzg
    dHlast[i, every block] = dx / CH"""
import numpy as np
import torch

import gat_mirror as G

ATT_NAMES = ('dWh', 'da1', 'db1', 'da2', 'db2', 'dbias')
RO_NAMES = ('dHlast', 'dWo', 'dbo', 'dwg', 'dbg')


def attention_backward(Wh, L, a1, b1, a2, b2, out, dOut, H, elu=True):
  """-> (dWh [B, N, C H Dh], da1 [C H, Dh], db1 [C H], da2, db2, dbias [C H, Dh]); `out` (the layer's
  forward output) is read for the ELU derivative only."""
  B, N, width = Wh.shape
  CH, Dh = a1.shape
  dWh = torch.zeros_like(Wh)
  da1, da2, dbias = torch.zeros_like(a1), torch.zeros_like(a2), torch.zeros_like(a1)
  db1, db2 = torch.zeros_like(b1), torch.zeros_like(b2)
  for k in range(CH):
    c = k // H
    sl = slice(k * Dh, (k + 1) * Dh)
    w = Wh[:, :, sl]
    s1 = w @ a1[k] + b1[k]
    s2 = w @ a2[k] + b2[k]
    z = s1.unsqueeze(2) + s2.unsqueeze(1)
    P = torch.softmax(torch.nn.functional.leaky_relu(z, 0.2) + L[:, :, :, c], dim=1)
    dO = dOut[:, :, sl]
    if elu:
      o = out[:, :, sl]
      dO = dO * torch.where(o > 0, torch.ones_like(o), o + 1)
    dP = dO @ w.transpose(1, 2)                               # [B, i, j]
    t = (P * dP).sum(dim=1, keepdim=True)
    dE = P * (dP - t)
    dZ = dE * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.2))
    ds1, ds2 = dZ.sum(dim=2), dZ.sum(dim=1)                   # [B, N] each
    dWh[:, :, sl] = P.transpose(1, 2) @ dO + ds1.unsqueeze(2) * a1[k] + ds2.unsqueeze(2) * a2[k]
    da1[k] = torch.einsum('bi,bid->d', ds1, w)
    da2[k] = torch.einsum('bi,bid->d', ds2, w)
    db1[k], db2[k] = ds1.sum(), ds2.sum()
    dbias[k] = dO.sum(dim=(0, 1))
  return dWh, da1, db1, da2, db2, dbias


def readout_backward(Hlast, mask, Wo, bo, wg, bg, CH, dscore):
  """-> (dHlast [B, N, CH Dh], dWo [P, Dh], dbo [P], dwg [Dh], dbg [1])"""
  B, N, width = Hlast.shape
  Dh = width // CH
  x = Hlast.reshape(B, N, CH, Dh).mean(dim=2)
  o = x @ Wo.t() + bo
  g = torch.sigmoid(x @ wg.reshape(-1, 1) + bg)              # [B, N, 1]
  mk = torch.ones(B, N, 1, dtype=Hlast.dtype) if mask is None else (mask != 0).to(Hlast.dtype).unsqueeze(2)
  dy = (dscore / mk.sum(dim=1)).unsqueeze(1) * mk             # [B, N, P], zero outside the mask
  do = dy * g
  dzg = (dy * o).sum(dim=2, keepdim=True) * g * (1 - g)
  dx = do @ Wo + dzg * wg.reshape(1, 1, -1)
  dHlast = (dx / CH).unsqueeze(2).expand(B, N, CH, Dh).reshape(B, N, width)
  return (dHlast, torch.einsum('bip,bid->pd', do, x), do.sum(dim=(0, 1)), (dzg * x).sum(dim=(0, 1)),
          dzg.sum().reshape(1))


def attention_autograd(Wh, L, a1, b1, a2, b2, bias, dOut, H, elu=True):
  """the same six gradients by autograd through gat_mirror.attention, in the operands' dtype"""
  ops = [x.detach().clone().requires_grad_(True) for x in (Wh, a1, b1, a2, b2, bias)]
  out = G.attention(ops[0], L, ops[1], ops[2], ops[3], ops[4], ops[5], H, elu)
  return torch.autograd.grad(out, ops, dOut)


def readout_autograd(Hlast, mask, Wo, bo, wg, bg, CH, dscore):
  ops = [x.detach().clone().requires_grad_(True) for x in (Hlast, Wo, bo, wg, bg)]
  s = G.readout(ops[0], mask, ops[1], ops[2], ops[3], ops[4], CH)
  gr = torch.autograd.grad(s, ops, dscore)
  return gr[0], gr[1], gr[2], gr[3].reshape(-1), gr[4]


def permutations(B, N, count=8, seed=5):
  """`count` (molecule permutation, node permutation) pairs, the identity first"""
  g = torch.Generator().manual_seed(seed)
  out = [(torch.arange(B), torch.arange(N))]
  while len(out) < count:
    out.append((torch.randperm(B, generator=g), torch.randperm(N, generator=g)))
  return out


def attention_e32(ops32, truth, H, elu):
  """per gradient: the largest error over eight evaluations of the CPU float32 autograd — the operands as
  given and seven with the molecules and the nodes consistently permuted (rows of Wh / dOut, rows and
  columns of L; the gradients un-permuted) —, in units of max|truth|"""
  Wh, L, a1, b1, a2, b2, bias, dOut = ops32
  B, N = Wh.shape[:2]
  worst = [0.0] * 6
  for pb, pn in permutations(B, N):
    gr = list(attention_autograd(Wh[pb][:, pn], L[pb][:, pn][:, :, pn], a1, b1, a2, b2, bias, dOut[pb][:, pn], H, elu))
    back = torch.empty_like(gr[0])
    back[pb.unsqueeze(1), pn.unsqueeze(0)] = gr[0]
    gr[0] = back
    for k in range(6):
      scale = float(truth[k].abs().max())
      if scale > 0:
        worst[k] = max(worst[k], float((gr[k].double() - truth[k]).abs().max()) / scale)
  return worst


def readout_e32(ops32, truth, CH):
  Hl, mask, Wo, bo, wg, bg, dscore = ops32
  B, N = Hl.shape[:2]
  worst = [0.0] * 5
  for pb, pn in permutations(B, N):
    gr = list(readout_autograd(Hl[pb][:, pn], None if mask is None else mask[pb][:, pn], Wo, bo, wg, bg, CH,
                               dscore[pb]))
    back = torch.empty_like(gr[0])
    back[pb.unsqueeze(1), pn.unsqueeze(0)] = gr[0]
    gr[0] = back
    for k in range(5):
      scale = float(truth[k].abs().max())
      if scale > 0:
        worst[k] = max(worst[k], float((gr[k].double() - truth[k]).abs().max()) / scale)
  return worst


# ------------------------------------------------------------------------------------------ whole net
def net_forward(Q, cfg, node_feat, L, mask):
  """gat_mirror.forward on a dict of TENSORS (name -> tensor, any dtype, requires_grad allowed), without
  the detach: differentiable with respect to every entry that is read."""
  m = cfg.model
  C, T = cfg.dataset.num_bond_type + 1, m.num_layer
  dtype = Q['embedding.weight'].dtype
  state = Q['embedding.weight'][node_feat]
  B, N = node_feat.shape
  Lt = L.to(dtype)
  for t in range(T):
    H = m.num_heads[t]
    blocks = [(c, h) for c in range(C) for h in range(H)]
    W = torch.cat([Q['filter.%d.%d.%d.weight' % (t, c, h)] for c, h in blocks], dim=0)
    a1 = torch.cat([Q['att_net_1.%d.%d.%d.weight' % (t, c, h)] for c, h in blocks], dim=0)
    b1 = torch.cat([Q['att_net_1.%d.%d.%d.bias' % (t, c, h)] for c, h in blocks], dim=0)
    a2 = torch.cat([Q['att_net_2.%d.%d.%d.weight' % (t, c, h)] for c, h in blocks], dim=0)
    b2 = torch.cat([Q['att_net_2.%d.%d.%d.bias' % (t, c, h)] for c, h in blocks], dim=0)
    bias = torch.stack([Q['bias_%d_%d_%d' % (h, C - 1, t)] for c, h in blocks], dim=0)
    Wh = (state.reshape(B * N, -1) @ W.t()).reshape(B, N, -1)
    state = G.attention(Wh, Lt, a1, b1, a2, b2, bias, H, elu=t < T - 1)
  return G.readout(state, mask, Q['output_func.0.weight'], Q['output_func.0.bias'], Q['att_func.0.weight'],
                   Q['att_func.0.bias'], C * m.num_heads[T - 1])


def net_gradients(P, cfg, batch, dtype, perm=None):
  """Gradients of the MSE loss with respect to every parameter, as a dict name -> tensor (None where the
  parameter is never read), by autograd through net_forward in `dtype`.  perm = (molecules, nodes): the
  batch consistently permuted (the gradients of the parameters need no un-permuting)."""
  Q = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in P.items()}
  nf = torch.from_numpy(np.asarray(batch['node_feat'])).long()
  L = torch.from_numpy(np.asarray(batch['L']))
  mask = torch.from_numpy(np.asarray(batch['node_mask']))
  label = torch.from_numpy(np.asarray(batch['label'])).to(dtype)
  if perm is not None:
    pb, pn = perm
    nf, L, mask, label = nf[pb][:, pn], L[pb][:, pn][:, :, pn], mask[pb][:, pn], label[pb]
  score = net_forward(Q, cfg, nf, L, mask)
  loss = torch.nn.functional.mse_loss(score, label)
  names = list(Q)
  gr = torch.autograd.grad(loss, [Q[k] for k in names], allow_unused=True)
  return dict(zip(names, gr)), float(loss.detach())


def param_groups(names, cfg):
  """The groups the module tests compare: per layer the stacked filter, att_net_1 / att_net_2 weight and
  bias and the read bias_*; the embedding; output_func; att_func.  -> list of (group name, [names])"""
  C, T = cfg.dataset.num_bond_type + 1, cfg.model.num_layer
  names = list(names)
  groups = []
  for t in range(T):
    for stem in ('filter', 'att_net_1', 'att_net_2'):
      for leaf in (('weight',) if stem == 'filter' else ('weight', 'bias')):
        sel = [k for k in names if k.startswith('%s.%d.' % (stem, t)) and k.endswith('.' + leaf)]
        groups.append(('%s.%d.%s' % (stem, t, leaf), sel))
    groups.append(('bias.%d' % t, [k for k in names if k.startswith('bias_') and k.endswith('_%d_%d' % (C - 1, t))]))
  groups.append(('embedding', ['embedding.weight']))
  groups.append(('output_func', ['output_func.0.weight', 'output_func.0.bias']))
  groups.append(('att_func', ['att_func.0.weight', 'att_func.0.bias']))
  return groups
