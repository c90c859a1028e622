"""`GPNN` (reference `model/gpnn.py:10-251`, `config/qm8_gpnn.yaml`) on the fused partition-propagation
kernel (csrc/gpnn.hip).

Same constructor keys, `forward(node_feat, L, L_cluster, L_cut, label=None, mask=None)`, `state_dict` keys
and shapes, `named_parameters()` order and module creation order (`embedding`, `update_func`,
`update_func_partition`, `state_func`, `msg_func`, `att_func`, `input_func`, `output_func`: the RNG draws
line up) as the reference, so a reference checkpoint loads unchanged.  Reproduced, not fixed (INTEGRATION.md
§5): `_init_param` passes over `msg_func` (a ModuleList: its Linears keep torch's default init and nonzero
biases), Xavier-inits `state_func`, `input_func`, `att_func` and `output_func`, draws both cells'
`weight_hh` before `weight_ih`, and with `update_func: 'MLP'` initialises nothing (the two Sequentials are
not `nn.Linear`); every one of the N rows takes part in every propagation, the mask enters only the final
mean, `mask=None` averages all N rows, a molecule with no masked node scores NaN; `L_cluster` and `L_cut`
enter by value.  Two configurations the reference constructs and cannot run are constructed here too and
refused by `forward` with a NotImplementedError naming the reference line: `msg_func` other than 'MLP'
(model/gpnn.py:168-182 and :193-205 read an unbound `tmp_msg` / `msg`) and `update_func: 'MLP'`
(model/gpnn.py:187 and :210 call an nn.Sequential with two arguments).  One documented deviation: the
reference overwrites the caller's tensor (`L[L != 0] = 1.0`, model/gpnn.py:158); the port writes to none of
`L`, `L_cluster`, `L_cut`, both routes read `L != 0`.

Route 'gpnn_hip' (any call that needs no gradient, inside the kernel's envelope): the [num_atom, D] table
`input_func(embedding.weight)` is ONE `f32_linear` launch per weight version, gathered per call, then ONE
`gpnn_forward` launch for all `num_prop` outer steps and the readout.  Everything else — gradients (a HIP
backward does not exist yet), dropout in training, `update_func: 'RNN'`, shapes outside the envelope —
takes 'gpnn_torch', a device-side differentiable torch restatement, with one UserWarning per module that
names the reason.  There is no CPU path.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ._baseline import _Baseline
from ._common import _opt

__all__ = ['GPNN']

EPS = float(np.finfo(np.float32).eps)
GPNN_INPUT_STEP = 32   # lnz_f32_linear: K (= input_dim) a multiple of 32


class GPNN(_Baseline):
    """Graph Partition Neural Networks (Liao et al., 2018) as the reference builds it for QM8."""
    _route_prefix = 'gpnn'

    def __init__(self, config):
        super().__init__()
        m = config.model
        self.config = config
        self.input_dim = m.input_dim
        self.hidden_dim = m.hidden_dim
        self.output_dim = m.output_dim
        self.num_layer = m.num_layer
        self.num_prop = m.num_prop
        self.num_partition = m.num_partition
        self.num_prop_cluster = m.num_prop_cluster
        self.num_prop_cut = m.num_prop_cut
        self.dropout = _opt(m, 'dropout', 0.0)
        self.num_atom = config.dataset.num_atom
        self.num_edgetype = config.dataset.num_bond_type
        self.aggregate_type = m.aggregate_type
        self.update_kind = m.update_func
        self.msg_kind = m.msg_func
        assert self.num_layer == 1, "not implemented"
        assert self.aggregate_type in ['avg', 'sum'], 'not implemented'
        C, D = self.num_edgetype + 1, self.hidden_dim

        # creation order == reference (RNG parity and named_parameters order): model/gpnn.py:40-94
        self.embedding = nn.Embedding(self.num_atom, self.input_dim)
        if m.update_func == 'RNN':
            self.update_func = nn.RNNCell(input_size=D * C, hidden_size=D, nonlinearity='relu')
            self.update_func_partition = nn.RNNCell(input_size=D, hidden_size=D, nonlinearity='relu')
        elif m.update_func == 'GRU':
            self.update_func = nn.GRUCell(input_size=D * C, hidden_size=D)
            self.update_func_partition = nn.GRUCell(input_size=D, hidden_size=D)
        elif m.update_func == 'MLP':
            self.update_func = nn.Sequential(nn.Linear(D * C, D), nn.Tanh())
            self.update_func_partition = nn.Sequential(nn.Linear(D, D), nn.Tanh())
        self.state_func = nn.Sequential(nn.Linear(3 * D, ops.GPNN_STATE_HIDDEN), nn.ReLU(),
                                        nn.Linear(ops.GPNN_STATE_HIDDEN, D))
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
        # model/gpnn.py:107-139.  msg_func is a ModuleList, neither an nn.Sequential nor an nn.Linear: the
        # reference's loop passes over it, its Linears keep torch's default init and nonzero biases
        self._init_sequentials((self.input_func, self.state_func, self.msg_func, self.att_func, self.output_func))
        if self.update_kind in ('GRU', 'RNN'):
            self._init_cell(self.update_func)
            self._init_cell(self.update_func_partition)
        # update_func 'MLP': model/gpnn.py:134-139 tests the two Sequentials themselves for nn.Linear, which
        # they are not: nothing is initialised, torch's default init stays

    # -- the packed operands of route 'gpnn_hip' -------------------------------------------------------
    def _msg_operands(self):
        """(W1 [C, 128, D], b1 [C, 128], W2 [C, D, 128], b2 [C, D]) of the live parameters."""
        W1 = torch.stack([f[0].weight for f in self.msg_func])
        b1 = torch.stack([f[0].bias for f in self.msg_func])
        W2 = torch.stack([f[2].weight for f in self.msg_func])
        b2 = torch.stack([f[2].bias for f in self.msg_func])
        return W1, b1, W2, b2

    def _packs(self):
        """(table [num_atom, D] = input_func(embedding.weight), the twenty operands of ops.gpnn_forward), once per
        weight version"""
        def build():
            f = lambda x: x.detach().float().contiguous()  # noqa: E731
            cell, part, st = self.update_func, self.update_func_partition, self.state_func
            operands = tuple(f(x) for x in self._msg_operands() + (
                cell.weight_ih, cell.bias_ih, cell.weight_hh, cell.bias_hh,
                part.weight_ih, part.bias_ih, part.weight_hh, part.bias_hh,
                st[0].weight, st[0].bias, st[2].weight, st[2].bias,
                self.output_func[0].weight, self.output_func[0].bias, self.att_func[0].weight, self.att_func[0].bias))
            table = ops.f32_linear(f(self.embedding.weight), f(self.input_func[0].weight),
                                   bias=f(self.input_func[0].bias))
            return table, operands
        return self._cached('_pack_cache', build)

    # -- which route serves a call ----------------------------------------------------------------
    def _why_not_hip(self, N, L, L_cluster, L_cut, needs_grad, drop):
        """None when route 'gpnn_hip' serves the call, else the reason in words.  No GPU needed to ask."""
        C, D = self.num_edgetype + 1, self.hidden_dim
        if needs_grad:
            return 'gradients are required (the kernel has no HIP backward yet)'
        if drop:
            return 'dropout=%r in training' % self.dropout
        if self.update_kind != 'GRU':
            return "update_func=%r: the kernel holds the GRU update, not the RNN update" % self.update_kind
        if not (getattr(self.update_func, 'bias', True) and getattr(self.update_func_partition, 'bias', True)):
            return 'a GRU cell has no biases'
        if N > ops.GGNN_MAX_NODES:
            return '%d nodes > %d' % (N, ops.GGNN_MAX_NODES)
        if D % ops.GGNN_WIDTH_STEP or D > ops.GGNN_MAX_WIDTH or C > ops.GGNN_MAX_CHANNELS:
            return ('hidden_dim D = %d, %d channels (kernel: D a multiple of %d and <= %d, <= %d channels)'
                    % (D, C, ops.GGNN_WIDTH_STEP, ops.GGNN_MAX_WIDTH, ops.GGNN_MAX_CHANNELS))
        if self.input_dim % GPNN_INPUT_STEP:
            return 'input_dim=%d is not a multiple of %d' % (self.input_dim, GPNN_INPUT_STEP)
        if self.output_dim > ops.GGNN_MAX_OUTPUTS:
            return 'output_dim=%d > %d' % (self.output_dim, ops.GGNN_MAX_OUTPUTS)
        if self.num_prop < 0 or self.num_prop_cluster < 0 or self.num_prop_cut < 0:
            return 'num_prop=%d, num_prop_cluster=%d, num_prop_cut=%d' % (self.num_prop, self.num_prop_cluster,
                                                                         self.num_prop_cut)
        return self._why_not_hip_operands(L, C, graphs=(('L_cluster', L_cluster), ('L_cut', L_cut)))

    def forward(self, node_feat, L, L_cluster, L_cut, label=None, mask=None):
        """node_feat [B, N] long, L [B, N, N, E + 1] float (read as L != 0), L_cluster / L_cut [B, N, N] float
        (read by value), none of the three written; label [B, P], mask [B, N] (None: the mean runs over all N
        rows, model/gpnn.py:242-244) -> score [B, P], or (score, loss) with a label."""
        if self.msg_kind != 'MLP':
            raise NotImplementedError('GPNN: msg_func=%r: the reference reads an unbound tmp_msg / msg '
                                      '(model/gpnn.py:168-182, :193-205); only msg_func: MLP runs' % (self.msg_kind,))
        if self.update_kind not in ('GRU', 'RNN'):
            raise NotImplementedError('GPNN: update_func=%r: the reference calls an nn.Sequential with two '
                                      'arguments (model/gpnn.py:187, :210); only GRU and RNN run'
                                      % (self.update_kind,))
        return self._dispatch(node_feat=node_feat, L=L, L_cluster=L_cluster, L_cut=L_cut, label=label, mask=mask)

    @torch.no_grad()
    def _hip_forward(self, node_feat, L, L_cluster, L_cut, mask):
        table, operands = self._packs()
        return ops.gpnn_forward(table[node_feat], L, L_cluster, L_cut, mask, *operands, self.num_prop,
                                self.num_prop_cluster, self.num_prop_cut, avg=self.aggregate_type == 'avg')

    def _torch_forward(self, node_feat, L, L_cluster, L_cut, mask, dropout=False):
        """Differentiable torch restatement of model/gpnn.py:159-246 on device tensors, the C message MLPs
        of the GGNN step batched.  `L`, `L_cluster` and `L_cut` are read, never written."""
        B, N = node_feat.shape
        C, D = self.num_edgetype + 1, self.hidden_dim
        state = self.input_func(self.embedding(node_feat))                    # [B, N, D]
        A = (L != 0).to(state.dtype).permute(0, 3, 1, 2)                        # [B, C, N, N]
        Wcl, Wct = L_cluster.to(state.dtype), L_cut.to(state.dtype)
        if self.aggregate_type == 'avg':
            A = A / (A.sum(dim=3, keepdim=True) + EPS)
            Wcl = Wcl / (Wcl.sum(dim=2, keepdim=True) + EPS)
            Wct = Wct / (Wct.sum(dim=2, keepdim=True) + EPS)
        W1, b1, W2, b2 = self._msg_operands()
        Hd = W1.shape[1]

        def part(x, W):
            msg = torch.bmm(W, self.msg_func[0](x))
            return self.update_func_partition(msg.reshape(B * N, D), x.reshape(B * N, D)).view(B, N, D)

        for _ in range(self.num_prop):
            sc, sx = state, state
            for _i in range(self.num_prop_cluster):
                sc = part(sc, Wcl)
            for _i in range(self.num_prop_cut):
                sx = part(sx, Wct)
            state = self.state_func(torch.cat([state, sc, sx], dim=2))
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
