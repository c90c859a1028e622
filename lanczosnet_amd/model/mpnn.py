"""`MPNN` (reference `model/mpnn.py:14-212`, `model/set2set.py`, `config/qm8_mpnn.yaml`) on the fused
edge-network propagation kernel and the Set2Vec readout kernel (csrc/mpnn.hip).

Same constructor keys, `forward(node_feat, L, label=None, mask=None)`, `state_dict` keys and shapes,
`named_parameters()` order and module creation order (`node_embedding`, `input_func`, `update_func`,
`edge_embedding` or `edge_func`, `att_func`, `output_func`: the RNG draws line up) as the reference, so
`from model import *` picks the class up by name and a reference checkpoint loads unchanged.
Reproduced, not fixed: `_init_param` passes over `att_func` (a Set2Vec, neither an
nn.Sequential nor an nn.Linear: it keeps its own constructor init) and over `edge_func` (a ModuleList:
torch's default init stays, the biases are NOT zero), and draws the cell's `weight_hh` before
`weight_ih`; every one of the N rows propagates (a padded row evolves under GRU(0, h)); `mask=None`
reads all N rows; an unknown `msg_func` raises ValueError at construction.  Documented deviations: the
caller's `L` is never written (the reference does `L[L != 0] = 1.0`, model/mpnn.py:125; both routes read
`L != 0`); B = 1 with 'sum' is served (the reference's `.squeeze()`, model/mpnn.py:170, drops the batch
dimension and the concatenation fails); the mask is read as `!= 0` whatever its dtype (the reference
indexes with it, so a uint8 mask is a deprecated byte index and a float mask an error).

Route 'mpnn_hip' (any call that needs no gradient, `msg_func: MLP`, no dropout in training, float32,
inside the kernels' envelope): `state_0 = input_func(node_embedding(node_feat))` has only `num_atom`
distinct rows — the [num_atom, D] table is ONE `f32_linear` launch per weight version, gathered per
call — then ONE `mpnn_forward` launch for all `num_prop` steps and ONE `set2vec_readout` launch for the
Set2Vec steps and `output_func`.  Everything else — gradients, dropout in training, `msg_func:
embedding`, shapes outside the envelope — takes 'mpnn_torch', a device-side differentiable torch
restatement in the factored form of the kernel (the first Linear of the edge network split over the
concatenation; `M_c = Â_c (S E_c)` for 'embedding'), with one UserWarning per module that names the
reason.  There is no CPU path.

Route 'mpnn_hip_train' (opt-in: `LANCZOSNET_MPNN_BACKWARD=hip`, or `net.mpnn_backward_impl = 'hip'`; a call
that needs gradients inside the same envelope): the propagation is one `torch.autograd.Function` — the
[num_atom, D] table and its gather, ONE `mpnn_forward_states` launch (route 'mpnn_hip''s kernel body and bits,
plus the state trajectory [num_prop + 1, B, N, D]: nothing else is saved, against one [B, N, N, 64] tensor per
channel and step on 'mpnn_torch'), and under `loss.backward()` one `mpnn_backward_step` launch per step
t = T-1 .. 0 (the step is recomputed on chip from S_t) with the step's weight gradients by the library GEMM,
`embedding_grad` into the table and the tiny input gradients in torch (csrc/mpnn_grad.hip).  Set2Vec and
`output_func` stay ordinary autograd on S_T (`set2vec_batched`): there is no Set2Vec backward kernel.  Dropout
in training, `msg_func: embedding` and every shape reason still take 'mpnn_torch'.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ._baseline import _Baseline
from ._common import _opt
from .set2set import Set2Vec, set2vec_batched

__all__ = ['MPNN']

EPS = float(np.finfo(np.float32).eps)
MPNN_INPUT_STEP = 32   # lnz_f32_linear: K (= input_dim) a multiple of 32


class _MpnnTrainFunction(torch.autograd.Function):
    """The propagation of route 'mpnn_hip_train': forward = `MPNN._hip_forward`'s table, gather and kernel body,
    leaving the state trajectory and returning S_T; backward = the steps T-1 .. 0 (each recomputed from its S_t,
    its weight gradients accumulated by the library GEMM), the table's gradient by atom id (all N rows take
    part, the padding id included, as in the reference), the input layer and the embedding in torch.  Inputs
    after the five plain ones: node_embedding.weight, input_func W, b, the stacked W1, b1, W2, b2, the cell's
    W_ih, b_ih, W_hh, b_hh."""

    @staticmethod
    def forward(ctx, avg, num_prop, transposes, node_feat, L, emb, Win, bin_, *operands):
        f = lambda x: x.detach().float().contiguous()  # noqa: E731
        emb, Win, bin_ = f(emb), f(Win), f(bin_)
        operands = tuple(f(x) for x in operands)
        table = ops.f32_linear(emb, Win, bias=bin_)
        states = ops.mpnn_forward_states(table[node_feat], L, *operands, num_prop, avg=avg)
        ctx.avg, ctx.transposes, ctx.operands, ctx.input = avg, transposes, operands, (emb, Win)
        ctx.save_for_backward(node_feat, L)
        ctx.states = states
        return states[states.shape[0] - 1].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dST):
        node_feat, L = ctx.saved_tensors
        states, prop = ctx.states, ctx.operands
        emb, Win = ctx.input
        T, B, N, D = states.shape[0] - 1, states.shape[1], states.shape[2], states.shape[3]
        C = L.shape[3]
        dS = dST.float().contiguous()
        grads = None
        if T > 0:
            spare, bufs = torch.empty_like(dS), ops.mpnn_step_buffers(B, N, C, D, dS.device)
            deg = ops.mpnn_edge_degrees(L)
            for t in range(T - 1, -1, -1):
                spare, _ = ops.mpnn_backward_step(states[t], dS, L, *prop, transposes=ctx.transposes, avg=ctx.avg,
                                                  dS=spare, buffers=bufs)
                dS, spare = spare, dS
                grads = ops.mpnn_step_weight_grads(states[t], bufs, C, deg, grads)
        dtable = ops.embedding_grad(node_feat.contiguous(), dS, D, emb.shape[0])
        dWin, dbin, demb = dtable.t() @ emb, dtable.sum(dim=0), dtable @ Win
        return (None,) * 5 + (demb, dWin, dbin) + (tuple(grads) if grads is not None else (None,) * 8)


class MPNN(_Baseline):
    """Message Passing Neural Networks (Gilmer et al., ICML 2017) as the reference builds it for QM8."""
    _route_prefix = 'mpnn'
    _hip_kernels = 'kernels'
    _cache_slots = ('_pack_cache', '_transpose_cache')
    # 'torch': a call that needs gradients takes route 'mpnn_torch'; 'hip': route 'mpnn_hip_train'
    mpnn_backward_impl = os.environ.get('LANCZOSNET_MPNN_BACKWARD', 'torch')

    def __init__(self, config):
        super().__init__()
        m = config.model
        self.config = config
        self.input_dim = m.input_dim
        self.hidden_dim = m.hidden_dim
        self.output_dim = m.output_dim
        self.num_layer = m.num_layer
        self.num_prop = m.num_prop
        self.msg_func_name = m.msg_func
        self.num_step_set2vec = m.num_step_set2vec
        self.dropout = _opt(m, 'dropout', 0.0)
        self.num_atom = config.dataset.num_atom
        self.num_edgetype = config.dataset.num_bond_type
        self.aggregate_type = m.aggregate_type
        assert self.num_layer == 1, 'not implemented'
        assert self.aggregate_type in ['avg', 'sum'], 'not implemented'
        C, D = self.num_edgetype + 1, self.hidden_dim

        # creation order == reference (RNG parity and named_parameters order): model/mpnn.py:40-72
        self.node_embedding = nn.Embedding(self.num_atom, self.input_dim)
        self.input_func = nn.Sequential(nn.Linear(self.input_dim, D))
        self.update_func = nn.GRUCell(input_size=D * C, hidden_size=D)
        if m.msg_func == 'embedding':
            self.edge_embedding = nn.Embedding(C, D ** 2)
        elif m.msg_func == 'MLP':
            self.edge_func = nn.ModuleList([nn.Sequential(nn.Linear(2 * D, ops.MPNN_MSG_HIDDEN), nn.ReLU(),
                                                          nn.Linear(ops.MPNN_MSG_HIDDEN, D)) for _ in range(C)])
        else:
            raise ValueError('Non-supported message function')
        self.att_func = Set2Vec(D, self.num_step_set2vec)
        self.output_func = nn.Sequential(nn.Linear(2 * D, self.output_dim))

        self._finish_init(m.loss)

    def _init_param(self):
        # model/mpnn.py:85-108.  The loop runs over input_func, output_func and att_func; att_func is a
        # Set2Vec, neither an nn.Sequential nor an nn.Linear, and is passed over; edge_func is not in the
        # list at all: its Linears keep torch's default init and nonzero biases
        self._init_sequentials((self.input_func, self.output_func, self.att_func))
        self._init_cell(self.update_func)

    # -- the packed operands of route 'mpnn_hip' -------------------------------------------------------
    def _msg_operands(self):
        """(W1 [C, 64, 2 D], b1 [C, 64], W2 [C, D, 64], b2 [C, D]) of the live parameters."""
        W1 = torch.stack([f[0].weight for f in self.edge_func])
        b1 = torch.stack([f[0].bias for f in self.edge_func])
        W2 = torch.stack([f[2].weight for f in self.edge_func])
        b2 = torch.stack([f[2].bias for f in self.edge_func])
        return W1, b1, W2, b2

    def _embedding_weight(self):
        return self.node_embedding.weight

    def _packs(self):
        """(table [num_atom, D] = input_func(node_embedding.weight), the eight operands of ops.mpnn_forward,
        the six of ops.set2vec_readout), once per weight version"""
        def build():
            f = lambda x: x.detach().float().contiguous()  # noqa: E731
            cell, att = self.update_func, self.att_func
            prop = tuple(f(x) for x in self._msg_operands() + (cell.weight_ih, cell.bias_ih, cell.weight_hh,
                                                               cell.bias_hh))
            Wg, bg, W1T = ops.set2vec_pack([(g[0].weight.detach(), g[0].bias.detach()) for g in att.LSTM.gates()],
                                           att.W_1.detach())
            read = (Wg, bg, W1T, f(att.W_2).reshape(-1), f(self.output_func[0].weight), f(self.output_func[0].bias))
            table = ops.f32_linear(f(self.node_embedding.weight), f(self.input_func[0].weight),
                                   bias=f(self.input_func[0].bias))
            return table, prop, read
        return self._cached('_pack_cache', build)

    def _transposes(self):
        """(W1T, W2T, WihT, WhhT) of ops.mpnn_backward_step, once per weight version like `_packs`."""
        def build():
            W1, _, W2, _ = self._msg_operands()
            return ops.mpnn_pack_transposes(W1, W2, self.update_func.weight_ih, self.update_func.weight_hh)
        return self._cached('_transpose_cache', build)

    # -- which route serves a call ----------------------------------------------------------------
    def _why_not_hip(self, N, L, needs_grad, drop):
        """None when route 'mpnn_hip' (or, for a call that needs gradients with the switch on, route
        'mpnn_hip_train') serves the call, else the reason in words.  No GPU needed to ask."""
        C, D = self.num_edgetype + 1, self.hidden_dim
        if needs_grad and self.mpnn_backward_impl != 'hip':
            return 'gradients are required (the HIP backward is opt-in: LANCZOSNET_MPNN_BACKWARD=hip)'
        if drop:
            return 'dropout=%r in training' % self.dropout
        if self.msg_func_name != 'MLP':
            return "msg_func=%r: the kernel holds the edge-network MLP, not the edge embedding" % self.msg_func_name
        if N > ops.MPNN_MAX_NODES:
            return '%d nodes > %d' % (N, ops.MPNN_MAX_NODES)
        if D % ops.MPNN_WIDTH_STEP or D > ops.MPNN_MAX_WIDTH or C > ops.MPNN_MAX_CHANNELS:
            return ('hidden_dim D = %d, %d channels (kernel: D a multiple of %d and <= %d, <= %d channels)'
                    % (D, C, ops.MPNN_WIDTH_STEP, ops.MPNN_MAX_WIDTH, ops.MPNN_MAX_CHANNELS))
        if self.input_dim % MPNN_INPUT_STEP:
            return 'input_dim=%d is not a multiple of %d' % (self.input_dim, MPNN_INPUT_STEP)
        if self.output_dim > ops.MPNN_MAX_OUTPUTS:
            return 'output_dim=%d > %d' % (self.output_dim, ops.MPNN_MAX_OUTPUTS)
        if self.num_prop < 0 or self.num_step_set2vec < 0:
            return 'num_prop=%d, num_step_set2vec=%d' % (self.num_prop, self.num_step_set2vec)
        return self._why_not_hip_operands(L, C)

    def forward(self, node_feat, L, label=None, mask=None):
        """node_feat [B, N] long, L [B, N, N, E + 1] float (read as L != 0, never written), label [B, P],
        mask [B, N] (read as != 0; None: Set2Vec reads all N rows, model/mpnn.py:203-205) -> score [B, P],
        or (score, loss) with a label."""
        return self._dispatch(node_feat=node_feat, L=L, label=label, mask=mask)

    @torch.no_grad()
    def _hip_forward(self, node_feat, L, mask):
        table, prop, read = self._packs()
        state = ops.mpnn_forward(table[node_feat], L, *prop, self.num_prop, avg=self.aggregate_type == 'avg')
        return ops.set2vec_readout(state, mask, *read, self.num_step_set2vec)

    def _hip_train_forward(self, node_feat, L, mask):
        """The propagation on the HIP kernels (`_MpnnTrainFunction`), Set2Vec and output_func by autograd on S_T."""
        cell = self.update_func
        state = _MpnnTrainFunction.apply(
            self.aggregate_type == 'avg', self.num_prop, self._transposes(), node_feat, L,
            self.node_embedding.weight, self.input_func[0].weight, self.input_func[0].bias, *self._msg_operands(),
            cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh)
        return self.output_func(set2vec_batched(self.att_func, state, mask))

    def _torch_forward(self, node_feat, L, mask, dropout=False):
        """Differentiable torch restatement of model/mpnn.py:126-207 on device tensors, in the factored
        form of the kernel.  `L` is read, never written."""
        B, N = node_feat.shape
        C, D = self.num_edgetype + 1, self.hidden_dim
        state = self.input_func(self.node_embedding(node_feat))               # [B, N, D]
        A = (L != 0).to(state.dtype).permute(0, 3, 1, 2)                        # [B, C, N, N]
        deg = A.sum(dim=3, keepdim=True)                                        # [B, C, N, 1]
        for _ in range(self.num_prop):
            x = state.reshape(B * N, D)
            msg = []
            for c in range(C):
                if self.msg_func_name == 'MLP':
                    lin1, lin2 = self.edge_func[c][0], self.edge_func[c][2]
                    Pn = (x @ lin1.weight[:, :D].t()).view(B, 1, N, -1)          # the neighbour b
                    Qs = (x @ lin1.weight[:, D:].t() + lin1.bias).view(B, N, 1, -1)   # the row a
                    R = (F.relu(Qs + Pn) * A[:, c].unsqueeze(3)).sum(dim=2)       # [B, N, 64]
                    M = R @ lin2.weight.t() + deg[:, c] * lin2.bias
                    if self.aggregate_type == 'avg':
                        M = M / (deg[:, c] + EPS)
                else:
                    E = self.edge_embedding.weight[c].view(D, D)
                    Ac = A[:, c] / (deg[:, c] + EPS) if self.aggregate_type == 'avg' else A[:, c]
                    M = torch.bmm(Ac, (x @ E).view(B, N, D))
                msg.append(M)
            state = self.update_func(torch.cat(msg, dim=2).view(B * N, C * D), x).view(B, N, D)
            state = F.dropout(state, self.dropout, training=dropout)
        return self.output_func(set2vec_batched(self.att_func, state, mask))
