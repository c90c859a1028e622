"""`GAT` (reference `model/gat.py:8-201`, `config/qm8_gat.yaml`) on the hand-written attention and
readout kernels (csrc/gat.hip).

Same constructor keys, `forward(node_feat, L, label=None, mask=None)`, `state_dict` keys and shapes,
`named_parameters()` order (the root module's `bias_*` first) and `_init_param` draws as the
reference, so `from model import *` picks the class up by name and a reference checkpoint loads
unchanged.  Four properties of the reference are reproduced, not fixed:
`L` is ADDED to the logits (every padded row and column takes part; the mask enters only the final
mean), the softmax runs over the ROW index per column, every channel of a layer reads the bias of
the LAST channel (`bias_{h}_{E}_{t}`; the others are registered, saved and never read), and the
parameter order above.

Route 'gat_hip' (inference, and training calls that need no gradient): per layer ONE `f32_linear`
launch on the weight stack [C H Dh, Din], then `gat_attention`; `gat_readout` after the last layer.
Everything else — gradients, dropout in training, shapes outside the kernels — takes 'gat_torch', a
device-side differentiable torch restatement, with one UserWarning per module that names the reason.
There is no CPU path.

Route 'gat_hip_train' (opt-in: `LANCZOSNET_GAT_BACKWARD=hip`, or `net.gat_backward_impl = 'hip'`;
default 'torch': nothing changes): a call that needs gradients runs the same three kernels forward
(the score's bits are route 'gat_hip's) inside one autograd Function on the stacked operands of every
layer, and backward `gat_readout_backward`, per layer `gat_attention_backward` + `f32_linear` (dstate) +
a library GEMM (dW), and `embedding_grad` (csrc/gat_grad.hip).  Autograd's own backward
of `torch.stack` / `torch.cat` hands the pieces to the parameters: the C copies of the aliased
`bias_{h}_{E}_{t}` are summed, the never-read biases keep `grad is None`.  Dropout in training and
every shape reason still take 'gat_torch'.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ._baseline import _Baseline
from ._common import _opt

__all__ = ['GAT']

# the envelope of route 'gat_hip' beyond the kernels' own (ops.GAT_MAX_*): lnz_f32_linear's K, and the
# widths one stacked launch was sized for
GAT_MAX_WIDTH = 1024        # C H Dh, a multiple of GAT_WIDTH_STEP
GAT_WIDTH_STEP = 32         # ... and of the input width (lnz_f32_linear: K a multiple of 32)


class _GatTrainFunction(torch.autograd.Function):
    """Route 'gat_hip_train': forward = `GAT._hip_forward`'s three kernels on the stacked operands,
    saving per layer the input state and Wh (the output of layer t is the state of layer t + 1);
    backward = readout backward, layers T-1 .. 0, the embedding table's gradient (all N rows take
    part, the padding id included, as in the reference).  Inputs after the five plain ones: the
    embedding table, Wo, bo, wg, bg, then per layer W [C H, Dh, Din], a1, b1, a2, b2, bias."""

    @staticmethod
    def forward(ctx, H, CH, node_feat, L, mask, emb, Wo, bo, wg, bg, *layer_ops):
        T = len(layer_ops) // 6
        f = lambda x: x.detach().float().contiguous()  # noqa: E731
        layers = []
        for t in range(T):
            W, a1, b1, a2, b2, bias = layer_ops[6 * t:6 * t + 6]
            layers.append((f(W.reshape(-1, W.shape[2])), f(a1), f(b1), f(a2), f(b2), f(bias)))
        head = (f(Wo), f(bo), f(wg), f(bg))
        B, N = node_feat.shape
        states, whs = [emb.detach()[node_feat]], []
        for t in range(T):
            W, a1, b1, a2, b2, bias = layers[t]
            Wh = ops.f32_linear(states[t].reshape(B * N, states[t].shape[2]), W).view(B, N, -1)
            whs.append(Wh)
            states.append(ops.gat_attention(Wh, L, a1, b1, a2, b2, bias, H, elu=t < T - 1))
        score = ops.gat_readout(states[T], mask, *head, CH)
        ctx.H, ctx.CH, ctx.T, ctx.num_atom = H, CH, T, emb.shape[0]
        ctx.layers, ctx.head = layers, head
        ctx.save_for_backward(node_feat, L, mask)
        ctx.states, ctx.whs = states, whs
        return score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dscore):
        T, H = ctx.T, ctx.H
        node_feat, L, mask = ctx.saved_tensors
        states, whs = ctx.states, ctx.whs
        dstate, dWo, dbo, dwg, dbg = ops.gat_readout_backward(states[T], mask, *ctx.head, ctx.CH,
                                                              dscore.contiguous())
        grads = [None] * (6 * T)
        for t in range(T - 1, -1, -1):
            W, a1, b1, a2, b2, _ = ctx.layers[t]
            elu = t < T - 1
            dstate, dW, da1, db1, da2, db2, dbias = ops.gat_layer_backward(
                states[t], dstate, whs[t], states[t + 1] if elu else None, L, W, a1, b1, a2, b2, H, elu=elu)
            grads[6 * t:6 * t + 6] = [dW.view(a1.shape[0], a1.shape[1], -1), da1, db1, da2, db2, dbias]
        demb = ops.embedding_grad(node_feat.contiguous(), dstate, dstate.shape[2], ctx.num_atom)
        return (None, None, None, None, None, demb, dWo, dbo, dwg.view(1, -1), dbg) + tuple(grads)


class GAT(_Baseline):
    """Graph Attention Networks (Velickovic et al., ICLR 2018) as the reference builds it for QM8."""
    _route_prefix = 'gat'
    _hip_kernels = 'kernels'
    # 'torch': a call that needs gradients takes route 'gat_torch'; 'hip': route 'gat_hip_train'
    gat_backward_impl = os.environ.get('LANCZOSNET_GAT_BACKWARD', 'torch')

    def __init__(self, config):
        super().__init__()
        m = config.model
        self.input_dim = m.input_dim
        self.hidden_dim = list(m.hidden_dim)
        self.output_dim = m.output_dim
        self.num_layer = m.num_layer
        self.num_heads = list(m.num_heads)
        self.dropout = _opt(m, 'dropout', 0.0)
        self.num_atom = config.dataset.num_atom
        self.num_edgetype = config.dataset.num_bond_type
        C, T = self.num_edgetype + 1, self.num_layer

        # creation order == reference (RNG parity and named_parameters order): model/gat.py:28-75
        self.embedding = nn.Embedding(self.num_atom, self.input_dim)
        dims = [self.input_dim] + self.hidden_dim + [self.output_dim]

        def per_head(make):
            return nn.ModuleList([nn.ModuleList([nn.ModuleList([make(t) for _ in range(self.num_heads[t])])
                                                 for _ in range(C)]) for t in range(T)])
        self.filter = per_head(lambda t: nn.Linear(dims[t] * (1 if t == 0 else self.num_heads[t] * C),
                                                   dims[t + 1], bias=False))
        self.att_net_1 = per_head(lambda t: nn.Linear(dims[t + 1], 1))
        self.att_net_2 = per_head(lambda t: nn.Linear(dims[t + 1], 1))
        for t in range(T):
            for c in range(C):
                for h in range(self.num_heads[t]):
                    self.register_parameter('bias_%d_%d_%d' % (h, c, t), nn.Parameter(torch.zeros(dims[t + 1])))
        self.att_func = nn.Sequential(nn.Linear(dims[-2], 1), nn.Sigmoid())
        self.output_func = nn.Sequential(nn.Linear(dims[-2], dims[-1]))

        self._finish_init(m.loss)

    def _init_param(self):
        # model/gat.py:88-123: Xavier-uniform weights, zero biases, in this order
        heads = lambda nets: [l for per_t in nets for per_c in per_t for l in per_c]  # noqa: E731
        for group in (self.att_func, self.output_func, heads(self.filter), heads(self.att_net_1),
                      heads(self.att_net_2)):
            self._init_linears(group)

    # -- the parameters of one layer as stacked operands, block order c H + h ------------------------
    def _used_bias(self, h, t):
        """model/gat.py:62-70: the list of lists repeats ONE inner list, so every channel of layer t,
        head h reads the parameter of the last channel.  Resolved by name at forward time (a replica
        under nn.DataParallel reads its own copy)."""
        return getattr(self, 'bias_%d_%d_%d' % (h, self.num_edgetype, t))

    def _layer_operands(self, t):
        """(W [C H, Dh, Din], a1 [C H, Dh], b1 [C H], a2, b2, bias [C H, Dh]) of the live parameters."""
        blocks = [(c, h) for c in range(self.num_edgetype + 1) for h in range(self.num_heads[t])]
        W = torch.stack([self.filter[t][c][h].weight for c, h in blocks])
        a1 = torch.cat([self.att_net_1[t][c][h].weight for c, h in blocks])
        b1 = torch.cat([self.att_net_1[t][c][h].bias for c, h in blocks])
        a2 = torch.cat([self.att_net_2[t][c][h].weight for c, h in blocks])
        b2 = torch.cat([self.att_net_2[t][c][h].bias for c, h in blocks])
        bias = torch.stack([self._used_bias(h, t) for c, h in blocks])
        return W, a1, b1, a2, b2, bias

    def _packs(self):
        """(per layer the six stacked operands of ops.gat_layer, the four of ops.gat_readout), once per weight
        version"""
        def build():
            layers = []
            for t in range(self.num_layer):
                W, a1, b1, a2, b2, bias = self._layer_operands(t)
                layers.append(tuple(x.detach().float().contiguous()
                                    for x in (W.reshape(-1, W.shape[2]), a1, b1, a2, b2, bias)))
            head = tuple(x.detach().float().contiguous() for x in (
                self.output_func[0].weight, self.output_func[0].bias, self.att_func[0].weight, self.att_func[0].bias))
            return layers, head
        return self._cached('_pack_cache', build)

    # -- which route serves a call ----------------------------------------------------------------
    def _why_not_hip(self, N, L, needs_grad, drop):
        """None when route 'gat_hip' serves the call, else the reason in words.  No GPU needed to ask."""
        C, T = self.num_edgetype + 1, self.num_layer
        if needs_grad and self.gat_backward_impl != 'hip':
            return 'gradients are required (the HIP backward is opt-in: LANCZOSNET_GAT_BACKWARD=hip)'
        if drop:
            return 'dropout=%r in training' % self.dropout
        if N > ops.GAT_MAX_NODES:
            return '%d nodes > %d' % (N, ops.GAT_MAX_NODES)
        Dh, H = self.hidden_dim[0], self.num_heads[0]
        if set(self.hidden_dim[:T]) != {Dh} or set(self.num_heads[:T]) != {H}:
            return 'hidden_dim=%r / num_heads=%r are not uniform' % (self.hidden_dim, self.num_heads)
        if (C > ops.GAT_MAX_CHANNELS or H > ops.GAT_MAX_HEADS or Dh > ops.GAT_MAX_HEAD_WIDTH or Dh % 4
                or (C * H * Dh) % GAT_WIDTH_STEP or C * H * Dh > GAT_MAX_WIDTH):
            return ('%d channels x %d heads of width %d (kernel: <= %d x <= %d of a width that is a multiple of 4 '
                    'and <= %d, %d | C H Dh <= %d)' % (C, H, Dh, ops.GAT_MAX_CHANNELS, ops.GAT_MAX_HEADS,
                                                      ops.GAT_MAX_HEAD_WIDTH, GAT_WIDTH_STEP, GAT_MAX_WIDTH))
        if self.input_dim % GAT_WIDTH_STEP:
            return 'input_dim=%d is not a multiple of %d' % (self.input_dim, GAT_WIDTH_STEP)
        if self.output_dim > ops.GAT_MAX_OUTPUTS:
            return 'output_dim=%d > %d' % (self.output_dim, ops.GAT_MAX_OUTPUTS)
        return self._why_not_hip_operands(L, C)

    def forward(self, node_feat, L, label=None, mask=None):
        """node_feat [B, N] long, L [B, N, N, E + 1] float, label [B, P], mask [B, N] (None: the mean
        runs over all N rows, model/gat.py:192-194) -> score [B, P], or (score, loss) with a label."""
        return self._dispatch(node_feat=node_feat, L=L, label=label, mask=mask)

    @torch.no_grad()
    def _hip_forward(self, node_feat, L, mask):
        layers, head = self._packs()
        H, T = self.num_heads[0], self.num_layer
        state = self.embedding.weight.detach()[node_feat]
        for t in range(T):
            state = ops.gat_layer(state, L, *layers[t], H, elu=t < T - 1)
        return ops.gat_readout(state, mask, *head, (self.num_edgetype + 1) * H)

    def _hip_train_forward(self, node_feat, L, mask):
        """The kernels of `_hip_forward` under autograd: the stacked operands come from the live
        parameters (`_layer_operands`, not the detached `_packs` cache), so that the backward of
        torch.stack / torch.cat distributes the gradients."""
        layer_ops = [x for t in range(self.num_layer) for x in self._layer_operands(t)]
        return _GatTrainFunction.apply(
            self.num_heads[0], (self.num_edgetype + 1) * self.num_heads[0], node_feat, L, mask,
            self.embedding.weight, self.output_func[0].weight, self.output_func[0].bias,
            self.att_func[0].weight, self.att_func[0].bias, *layer_ops)

    def _torch_forward(self, node_feat, L, mask, dropout=False):
        """Differentiable torch restatement of model/gat.py:142-196 on device tensors, all C H heads of
        a layer batched.  dropout=True draws what the reference draws per head: the head's copy of the
        state, its attention block and its Wh (model/gat.py:149,161-163)."""
        p = self.dropout
        B, N = node_feat.shape
        C, T = self.num_edgetype + 1, self.num_layer
        state = self.embedding(node_feat)
        Lc = L.to(state.dtype).permute(0, 3, 1, 2)                       # [B, C, N, N]
        for t in range(T):
            H = self.num_heads[t]
            W, a1, b1, a2, b2, bias = self._layer_operands(t)
            CH, Dh, Din = W.shape
            if dropout:
                xh = F.dropout(state.unsqueeze(1).expand(B, CH, N, Din), p, True)
                Wh = torch.einsum('bknd,kod->bkno', xh, W)
            else:
                Wh = (state.reshape(B * N, Din) @ W.reshape(CH * Dh, Din).t()).view(B, N, CH, Dh).permute(0, 2, 1, 3)
            s1 = torch.einsum('bknd,kd->bkn', Wh, a1) + b1.view(1, CH, 1)
            s2 = torch.einsum('bknd,kd->bkn', Wh, a2) + b2.view(1, CH, 1)
            e = F.leaky_relu(s1.unsqueeze(3) + s2.unsqueeze(2), 0.2) + Lc.repeat_interleave(H, dim=1)
            att = torch.softmax(e, dim=2)                                # over the ROW index, per column
            if dropout:
                att, Wh = F.dropout(att, p, True), F.dropout(Wh, p, True)
            out = att @ Wh + bias.view(1, CH, 1, Dh)
            if t == T - 1:
                state = out.mean(dim=1)
            else:
                state = F.elu(out).permute(0, 2, 1, 3).reshape(B, N, CH * Dh)
        y = self.output_func(state) * self.att_func(state)
        if mask is None:
            return y.mean(dim=1)
        mk = (mask != 0).to(y.dtype).unsqueeze(2)
        return (y * mk).sum(dim=1) / mk.sum(dim=1)
