"""`GGNN` (reference `model/ggnn.py:10-197`, `config/qm8_ggnn.yaml`) on the fused gated-propagation
kernel (csrc/ggnn.hip).

Same constructor keys, `forward(node_feat, L, label=None, mask=None)`, `state_dict` keys and shapes,
`named_parameters()` order and module creation order (`embedding`, `update_func`, `msg_func`,
`att_func`, `input_func`, `output_func`: the RNG draws line up) as the reference, so `from model import *`
picks the class up by name and a reference checkpoint loads unchanged.  Reproduced, not fixed
(INTEGRATION.md §5): `_init_param` skips `msg_func` (a ModuleList: its Linears keep torch's default
init and their biases are NOT zeroed) and draws the cell's `weight_hh` before `weight_ih`; every one
of the N rows takes part in the propagation (a padded row evolves under GRU(0, h)), the mask enters
only the final mean, `mask=None` averages all N rows, a molecule with no masked node scores NaN.
Two configurations the reference constructs and cannot run are constructed here too and refused by
`forward` with a NotImplementedError naming the reference line: `msg_func` other than 'MLP'
(model/ggnn.py:154,157 read an unbound `tmp_msg`) and `update_func: 'MLP'` (model/ggnn.py:168 calls an
nn.Sequential with two arguments).  One documented deviation: the reference overwrites the caller's
tensor (`L[L != 0] = 1.0`, model/ggnn.py:137); the port never writes to `L`, both routes read `L != 0`.

Route 'ggnn_hip' (inference, and any call that needs no gradient, inside the kernel's envelope):
`state_0 = input_func(embedding(node_feat))` has only `num_atom` distinct rows — the [num_atom, D]
table is ONE `f32_linear` launch per weight version, gathered per call — then ONE `ggnn_forward`
launch for all `num_prop` steps and the readout.  Everything else — gradients, dropout in training,
`update_func: 'RNN'`, shapes outside the envelope — takes 'ggnn_torch', a device-side differentiable
torch restatement, with one UserWarning per module that names the reason.  There is no CPU path.

Route 'ggnn_hip_train' (opt-in: `LANCZOSNET_GGNN_BACKWARD=hip`, or `net.ggnn_backward_impl = 'hip'`; a
call that needs gradients inside the same envelope): the same table and gather, ONE `ggnn_forward_states`
launch (route 'ggnn_hip''s kernel and bits, plus the state trajectory [num_prop + 1, B, N, D] — nothing else
is saved), and under `loss.backward()` the readout backward, one `ggnn_backward_step` launch per step
t = T-1 .. 0 (the step is recomputed on chip from S_t) with the step's weight gradients by the library
GEMM, `embedding_grad` into the table and the tiny input gradients in torch (csrc/ggnn_grad.hip).  Dropout
in training, the RNN update and every shape reason still take 'ggnn_torch'.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ._baseline import _Baseline
from ._common import _opt

__all__ = ['GGNN']

EPS = float(np.finfo(np.float32).eps)
GGNN_INPUT_STEP = 32   # lnz_f32_linear: K (= input_dim) a multiple of 32


class _GgnnTrainFunction(torch.autograd.Function):
    """Route 'ggnn_hip_train': forward = `GGNN._hip_forward`'s table, gather and kernel, leaving the state
    trajectory; backward = readout backward, the steps T-1 .. 0 (each recomputed from its S_t, its weight
    gradients accumulated by the library GEMM), the table's gradient by atom id (all N rows take part, the
    padding id included, as in the reference), the input layer and the embedding in torch.  Inputs after
    the six plain ones: embedding.weight, input_func W, b, the stacked W1, b1, W2, b2, the cell's W_ih,
    b_ih, W_hh, b_hh, Wo, bo, wg, bg."""

    @staticmethod
    def forward(ctx, avg, num_prop, transposes, node_feat, L, mask, emb, Win, bin_, *operands):
        f = lambda x: x.detach().float().contiguous()  # noqa: E731
        emb, Win, bin_ = f(emb), f(Win), f(bin_)
        operands = tuple(f(x) for x in operands)
        table = ops.f32_linear(emb, Win, bias=bin_)
        score, states = ops.ggnn_forward_states(table[node_feat], L, mask, *operands, num_prop, avg=avg)
        ctx.avg, ctx.transposes, ctx.operands, ctx.input = avg, transposes, operands, (emb, Win)
        ctx.save_for_backward(node_feat, L, mask)
        ctx.states = states
        return score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dscore):
        node_feat, L, mask = ctx.saved_tensors
        states, prop, head = ctx.states, ctx.operands[:8], ctx.operands[8:]
        emb, Win = ctx.input
        T, B, N, D = states.shape[0] - 1, states.shape[1], states.shape[2], states.shape[3]
        C = L.shape[3]
        dS, dWo, dbo, dwg, dbg = ops.ggnn_readout_backward(states[T], mask, *head, dscore.contiguous())
        grads = None
        if T > 0:
            spare, bufs = torch.empty_like(dS), ops.ggnn_step_buffers(B, N, C, D, dS.device)
            for t in range(T - 1, -1, -1):
                spare, _ = ops.ggnn_backward_step(states[t], dS, L, *prop, transposes=ctx.transposes, avg=ctx.avg,
                                                  dS=spare, buffers=bufs)
                dS, spare = spare, dS
                grads = ops.ggnn_step_weight_grads(states[t], bufs, C, grads)
        dtable = ops.embedding_grad(node_feat.contiguous(), dS, D, emb.shape[0])
        dWin, dbin, demb = dtable.t() @ emb, dtable.sum(dim=0), dtable @ Win
        return ((None,) * 6 + (demb, dWin, dbin) + (tuple(grads) if grads is not None else (None,) * 8)
                + (dWo, dbo, dwg.view(1, -1), dbg))


class GGNN(_Baseline):
    """Gated Graph Sequence Neural Networks (Li et al., ICLR 2016) as the reference builds it for QM8."""
    _route_prefix = 'ggnn'
    _cache_slots = ('_pack_cache', '_transpose_cache')
    # 'torch': a call that needs gradients takes route 'ggnn_torch'; 'hip': route 'ggnn_hip_train'
    ggnn_backward_impl = os.environ.get('LANCZOSNET_GGNN_BACKWARD', 'torch')

    def __init__(self, config):
        super().__init__()
        m = config.model
        self.config = config
        self.input_dim = m.input_dim
        self.hidden_dim = m.hidden_dim
        self.output_dim = m.output_dim
        self.num_layer = m.num_layer
        self.num_prop = m.num_prop
        self.dropout = _opt(m, 'dropout', 0.0)
        self.num_atom = config.dataset.num_atom
        self.num_edgetype = config.dataset.num_bond_type
        self.aggregate_type = m.aggregate_type
        self.update_kind = m.update_func
        self.msg_kind = m.msg_func
        assert self.num_layer == 1, "not implemented"
        assert self.aggregate_type in ['avg', 'sum'], 'not implemented'
        C, D = self.num_edgetype + 1, self.hidden_dim

        # creation order == reference (RNG parity and named_parameters order): model/ggnn.py:36-75
        self.embedding = nn.Embedding(self.num_atom, self.input_dim)
        if m.update_func == 'RNN':
            self.update_func = nn.RNNCell(input_size=D * C, hidden_size=D, nonlinearity='relu')
        elif m.update_func == 'GRU':
            self.update_func = nn.GRUCell(input_size=D * C, hidden_size=D)
        elif m.update_func == 'MLP':
            self.update_func = nn.Sequential(nn.Linear(D * C, D), nn.Tanh())
        if m.msg_func == 'MLP':
            self.msg_func = nn.ModuleList([nn.Sequential(nn.Linear(D, ops.GGNN_MSG_HIDDEN), nn.ReLU(),
                                                         nn.Linear(ops.GGNN_MSG_HIDDEN, D)) for _ in range(C)])
        else:
            self.msg_func = None
        self.att_func = nn.Sequential(nn.Linear(D, 1), nn.Sigmoid())
        self.input_func = nn.Sequential(nn.Linear(self.input_dim, D))
        self.output_func = nn.Sequential(nn.Linear(D, self.output_dim))

        self._finish_init(m.loss)

    def _init_param(self):
        # model/ggnn.py:88-120.  msg_func is a ModuleList, neither an nn.Sequential nor an nn.Linear: the
        # reference's loop passes over it, its Linears keep torch's default init and nonzero biases
        self._init_sequentials((self.input_func, self.msg_func, self.att_func, self.output_func))
        if self.update_kind in ('GRU', 'RNN'):
            self._init_cell(self.update_func)
        elif self.update_kind == 'MLP':
            self._init_linears(self.update_func)

    # -- the packed operands of route 'ggnn_hip' -------------------------------------------------------
    def _msg_operands(self):
        """(W1 [C, 128, D], b1 [C, 128], W2 [C, D, 128], b2 [C, D]) of the live parameters."""
        W1 = torch.stack([f[0].weight for f in self.msg_func])
        b1 = torch.stack([f[0].bias for f in self.msg_func])
        W2 = torch.stack([f[2].weight for f in self.msg_func])
        b2 = torch.stack([f[2].bias for f in self.msg_func])
        return W1, b1, W2, b2

    def _packs(self):
        """(table [num_atom, D] = input_func(embedding.weight), the twelve operands of ops.ggnn_forward), once per
        weight version"""
        def build():
            f = lambda x: x.detach().float().contiguous()  # noqa: E731
            cell = self.update_func
            operands = tuple(f(x) for x in self._msg_operands() + (
                cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, self.output_func[0].weight,
                self.output_func[0].bias, self.att_func[0].weight, self.att_func[0].bias))
            table = ops.f32_linear(f(self.embedding.weight), f(self.input_func[0].weight),
                                   bias=f(self.input_func[0].bias))
            return table, operands
        return self._cached('_pack_cache', build)

    def _transposes(self):
        """(W1T, W2T, WihT, WhhT) of ops.ggnn_backward_step, once per weight version like `_packs`."""
        def build():
            W1, _, W2, _ = self._msg_operands()
            return ops.ggnn_pack_transposes(W1, W2, self.update_func.weight_ih, self.update_func.weight_hh)
        return self._cached('_transpose_cache', build)

    # -- which route serves a call ----------------------------------------------------------------
    def _why_not_hip(self, N, L, needs_grad, drop):
        """None when route 'ggnn_hip' (or, for a call that needs gradients with the switch on, route
        'ggnn_hip_train') serves the call, else the reason in words.  No GPU needed to ask."""
        C, D = self.num_edgetype + 1, self.hidden_dim
        if needs_grad and self.ggnn_backward_impl != 'hip':
            return 'gradients are required (the HIP backward is opt-in: LANCZOSNET_GGNN_BACKWARD=hip)'
        if drop:
            return 'dropout=%r in training' % self.dropout
        if self.update_kind != 'GRU':
            return "update_func=%r: the kernel holds the GRU update, not the RNN update" % self.update_kind
        if not getattr(self.update_func, 'bias', True):
            return 'the GRU cell has no biases'
        if N > ops.GGNN_MAX_NODES:
            return '%d nodes > %d' % (N, ops.GGNN_MAX_NODES)
        if D % ops.GGNN_WIDTH_STEP or D > ops.GGNN_MAX_WIDTH or C > ops.GGNN_MAX_CHANNELS:
            return ('hidden_dim D = %d, %d channels (kernel: D a multiple of %d and <= %d, <= %d channels)'
                    % (D, C, ops.GGNN_WIDTH_STEP, ops.GGNN_MAX_WIDTH, ops.GGNN_MAX_CHANNELS))
        if self.input_dim % GGNN_INPUT_STEP:
            return 'input_dim=%d is not a multiple of %d' % (self.input_dim, GGNN_INPUT_STEP)
        if self.output_dim > ops.GGNN_MAX_OUTPUTS:
            return 'output_dim=%d > %d' % (self.output_dim, ops.GGNN_MAX_OUTPUTS)
        if self.num_prop < 0:
            return 'num_prop=%d' % self.num_prop
        return self._why_not_hip_operands(L, C)

    def forward(self, node_feat, L, label=None, mask=None):
        """node_feat [B, N] long, L [B, N, N, E + 1] float (read as L != 0, never written), label [B, P],
        mask [B, N] (None: the mean runs over all N rows, model/ggnn.py:188-190) -> score [B, P], or
        (score, loss) with a label."""
        if self.msg_kind != 'MLP':
            raise NotImplementedError('GGNN: msg_func=%r: the reference reads an unbound tmp_msg '
                                      '(model/ggnn.py:154,157); only msg_func: MLP runs' % (self.msg_kind,))
        if self.update_kind not in ('GRU', 'RNN'):
            raise NotImplementedError('GGNN: update_func=%r: the reference calls an nn.Sequential with two '
                                      'arguments (model/ggnn.py:168); only GRU and RNN run' % (self.update_kind,))
        return self._dispatch(node_feat=node_feat, L=L, label=label, mask=mask)

    @torch.no_grad()
    def _hip_forward(self, node_feat, L, mask):
        table, operands = self._packs()
        return ops.ggnn_forward(table[node_feat], L, mask, *operands, self.num_prop,
                                avg=self.aggregate_type == 'avg')

    def _hip_train_forward(self, node_feat, L, mask):
        cell = self.update_func
        return _GgnnTrainFunction.apply(
            self.aggregate_type == 'avg', self.num_prop, self._transposes(), node_feat, L, mask,
            self.embedding.weight, self.input_func[0].weight, self.input_func[0].bias, *self._msg_operands(),
            cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh, self.output_func[0].weight,
            self.output_func[0].bias, self.att_func[0].weight, self.att_func[0].bias)

    def _torch_forward(self, node_feat, L, mask, dropout=False):
        """Differentiable torch restatement of model/ggnn.py:138-192 on device tensors, the C message
        MLPs batched.  `L` is read, never written."""
        B, N = node_feat.shape
        C, D = self.num_edgetype + 1, self.hidden_dim
        state = self.input_func(self.embedding(node_feat))                    # [B, N, D]
        A = (L != 0).to(state.dtype).permute(0, 3, 1, 2)                        # [B, C, N, N]
        if self.aggregate_type == 'avg':
            A = A / (A.sum(dim=3, keepdim=True) + EPS)
        W1, b1, W2, b2 = self._msg_operands()
        Hd = W1.shape[1]
        for _ in range(self.num_prop):
            x = state.reshape(B * N, D)
            H = F.relu(x @ W1.reshape(C * Hd, D).t() + b1.reshape(-1)).view(B * N, C, Hd)
            M = torch.einsum('rch,cdh->rcd', H, W2) + b2                        # [B N, C, D]
            msg = torch.einsum('bcij,bjcd->bicd', A, M.view(B, N, C, D)).reshape(B * N, C * D)
            state = self.update_func(msg, x).view(B, N, D)
            state = F.dropout(state, self.dropout, training=dropout)
        y = self.output_func(state) * self.att_func(state)
        if mask is None:
            return y.mean(dim=1)
        mk = (mask != 0).to(y.dtype).unsqueeze(2)
        return (y * mk).sum(dim=1) / mk.sum(dim=1)
