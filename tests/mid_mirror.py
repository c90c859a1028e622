"""A plain torch restatement of the four launches for graphs of 33..128 nodes (csrc/conv_mid.hip:
lnz_midgraph_forward; csrc/conv_mid_grad.hip: lnz_midgraph_head_grad, lnz_midgraph_input_grad,
lnz_midgraph_project), dtype generic: every function computes in the dtype of its first operand, so
the same code is the float64 truth and the fp32 conditioning run (tests/test_gpu_mid_edges.py).

Operands are the raw ops' (ops.midgraph_forward and its neighbours), on N rows (never NR):
  X0 [B,N,din0]   L [B,N,N,C]   V [B,N,K]   G [num_layer,B,S,K] or None   mask [B,N]
  W: a list, per layer [128, S + C, din_l] (long scales first, then the operator channels)
  bias [num_layer,128]   Whead [dout + 1,128] (head rows, then the gate row)   bhead [dout + 1]
Non-finite entries of V are read as 0 (finite_or_zero of csrc/conv_tiles.hpp).

`pack_weights` gives the two flat fp32 forms the launches take: the forward's and the transposed one
of lnz_midgraph_input_grad ([128 in][S + C][128 out], layer 0 zero-padded to 128 input rows)."""
import torch


def _clean(V):
  return torch.where(torch.isfinite(V), V, torch.zeros_like(V))


def _cast(dtype, *ts):
  return [None if t is None else ([u.to(dtype) for u in t] if isinstance(t, (list, tuple)) else t.to(dtype))
          for t in ts]


def pack_weights(W):
  """(W flat, Wt flat), fp32: W = the layers' [128][S + C][din_l] blocks behind each other;
  Wt[l][i][c][o] = W[l][o][c][i], rows i >= din_l zero."""
  flat = torch.cat([w.float().reshape(-1) for w in W]).contiguous()
  Wt = []
  for w in W:
    t = torch.zeros((128, w.shape[1], 128), dtype=torch.float32)
    t[:w.shape[2]] = w.float().permute(2, 1, 0)
    Wt.append(t.reshape(-1))
  return flat, torch.cat(Wt).contiguous()


def conv_layer(X, L, V, g, W, bias):
  """relu(sum_s V diag(g_s) V^T X W_s^T + sum_c L_c X W_c^T + b) on all rows.  g [B,S,K] or None."""
  S = 0 if g is None else g.shape[1]
  out = bias.view(1, 1, -1).expand(X.shape[0], X.shape[1], -1)
  if S:
    Y = V.transpose(1, 2) @ X
    for s in range(S):
      out = out + V @ (g[:, s, :, None] * (Y @ W[:, s].t()))
  for c in range(L.shape[3]):
    out = out + L[..., c] @ (X @ W[:, S + c].t())
  return torch.relu(out)


def readout(X, mask, Whead, bhead):
  """The gated masked mean: mean over the masked rows of (W_h x + b_h) sigmoid(w_g x + b_g)."""
  z = X @ Whead.t() + bhead
  m = (mask != 0).to(X.dtype).unsqueeze(2)
  return (z[..., :-1] * torch.sigmoid(z[..., -1:]) * m).sum(dim=1) / m.sum(dim=1)


def forward(X0, L, V, G, mask, W, bias, Whead, bhead):
  """-> (states [num_layer,B,N,128], score [B,dout])."""
  dt = X0.dtype
  L, V, G, W, bias, Whead, bhead = _cast(dt, L, V, G, W, bias, Whead, bhead)
  V = _clean(V)
  X, states = X0, []
  for l in range(len(W)):
    X = conv_layer(X, L, V, None if G is None else G[l], W[l], bias[l])
    states.append(X)
  return torch.stack(states), readout(X, mask, Whead, bhead)


def head_grad(X_last, mask, gscore, Whead, bhead):
  """The readout's backward on a given last state [B,N,128] -> (dOut_last [B,N,128] = dLoss/dX masked
  by [X_last > 0], per-graph dWhead [B,dout + 1,128], per-graph dbhead [B,dout + 1])."""
  dt = X_last.dtype
  gscore, Whead, bhead = _cast(dt, gscore, Whead, bhead)
  m = (mask != 0).to(dt).unsqueeze(2)
  z = X_last @ Whead.t() + bhead
  sg = torch.sigmoid(z[..., -1:])
  dy = gscore.unsqueeze(1) / m.sum(dim=1, keepdim=True)
  dz = torch.cat([dy * sg, (dy * z[..., :-1]).sum(dim=2, keepdim=True) * sg * (1 - sg)], dim=2) * m
  dOut = (dz @ Whead) * (X_last > 0).to(dt)
  return dOut, dz.transpose(1, 2) @ X_last, dz.sum(dim=1)


def input_grad(dOut_last, states, L, V, G, W, din0):
  """The recurrence in the header of csrc/conv_mid_grad.hip from a given dOut of the last layer and
  GIVEN stored states [num_layer,B,N,128] (the ReLU mask of layer l is states[l - 1] > 0):
    dX_l = sum_s V diag(g_s) V^T dOut_l W_s + sum_c L_c^T dOut_l W_c,  dOut_{l-1} = dX_l [X_l > 0]
  -> (dOut [num_layer,B,N,128], dX0 [B,N,din0])."""
  dt = dOut_last.dtype
  L, V, G, W = _cast(dt, L, V, G, W)
  V = _clean(V)
  num_layer = len(W)
  S = 0 if G is None else G.shape[2]
  assert W[0].shape[2] == din0
  d, dOut = dOut_last, [None] * num_layer
  for l in range(num_layer - 1, -1, -1):
    dOut[l] = d
    dX = 0
    if S:
      A = V.transpose(1, 2) @ d
      for s in range(S):
        dX = dX + V @ (G[l, :, s, :, None] * (A @ W[l][:, s]))
    for c in range(L.shape[3]):
      dX = dX + L[..., c].transpose(1, 2) @ (d @ W[l][:, S + c])
    if l > 0:
      d = dX * (states[l - 1] > 0).to(dt)
  return torch.stack(dOut), dX


def project(dOut, states, X0, L, V, G, W):
  """Per layer, on given dOut and states: A = V^T dOut_l [num_layer,B,K,128], Q = g_s . (V^T X_l)
  [num_layer,B,K,S,128], M = L_c X_l [num_layer,B,N,C,128], dG[l][b][k][s] = sum_o A[k][o] ((V^T X_l)
  W_s^T)[k][o] [num_layer,B,K,S], db = column sums of dOut_l [num_layer,B,128]; X_0 is the input state
  zero-padded to 128 columns.  A, Q and dG are None without long scales."""
  dt = dOut.dtype
  states, X0, L, V, G, W = _cast(dt, states, X0, L, V, G, W)
  V = _clean(V)
  S = 0 if G is None else G.shape[2]
  A, Q, M, dG = [], [], [], []
  for l in range(len(W)):
    X = states[l - 1] if l else torch.nn.functional.pad(X0, (0, 128 - X0.shape[2]))
    M.append(torch.stack([L[..., c] @ X for c in range(L.shape[3])], dim=2))
    if S:
      Al, Y = V.transpose(1, 2) @ dOut[l], V.transpose(1, 2) @ X
      Yl = Y[..., :W[l].shape[2]]
      A.append(Al)
      Q.append(G[l].transpose(1, 2)[..., None] * Y[:, :, None, :])
      dG.append(torch.stack([(Al * (Yl @ W[l][:, s].t())).sum(dim=2) for s in range(S)], dim=2))
  st = torch.stack
  return (st(A) if S else None, st(Q) if S else None, st(M), st(dG) if S else None, dOut.sum(dim=2))


def param_grads(dOut, A, Q, M, db, W):
  """The parameter gradients `_MidGraphFusedFunction.backward` assembles from the projections: per
  layer dW [128, S + C, din_l] = [sum_b A^T Q | sum_b dOut^T M] cut to the layer's input width, and
  db [128]."""
  num_layer, B, N, _ = dOut.shape
  C = M.shape[3]
  dWs = []
  for l in range(num_layer):
    dWe = dOut[l].reshape(B * N, 128).t() @ M[l].reshape(B * N, C * 128)
    dW = dWe.view(128, C, 128)
    if A is not None:
      K, S = Q.shape[2], Q.shape[3]
      dWl = A[l].reshape(B * K, 128).t() @ Q[l].reshape(B * K, S * 128)
      dW = torch.cat([dWl.view(128, S, 128), dW], dim=1)
    dWs.append(dW[:, :, :W[l].shape[2]])
  return dWs, db.sum(dim=1)
