"""`LanczosNet` / `LanczosNetGeneral` nn.Modules backed by the gfx950 HIP path.

Drop-in surface of reference `model/lanczos_net.py:13-199` and
`model/lanczos_net_general.py:13-201`: same constructor config keys, same
`forward(node_feat, L, D, V, label=None, mask=None)` signature and return convention, same
`state_dict` keys (`filter.*`, `embedding.weight`, `spectral_filter.*.{0,2,4,6}.*`,
`att_func.0.*`), same parameter creation and init order, so `torch.manual_seed(s)` yields
the reference's weights and `utils/train_helper.py:28-32` checkpoints load unchanged.

The forward itself is three HIP launches (Laplacian pack + tile plan, spectral gains, fused
network) on the current torch stream; parameters are re-packed into MFMA fragment order only
when they change.  Training through `loss.backward()` (runner/qm8_runner.py:247): for LanczosNet /
LanczosNetGeneral at hidden width 128 the backward is HIP too (`_LanczosNetFusedFunction`:
input-gradient, message and gain-gradient kernels in the forward's tile structure + library GEMMs
for dW).  Architectures outside the fused kernels (other widths, N > 32, dropout
> 0 in training, AdaLanczosNet's backward) differentiate a device-side torch restatement of the
same math (`_torch_forward`) — still GPU only; there is no CPU path.  Graphs of 33..128 nodes have
a HIP backward of their own (`_MidGraphFusedFunction`, csrc/conv_mid_grad.hip),
opt-in through `mid_backward_impl`; beyond that ONE Function (`_LargeSparseFusedFunction`,
csrc/conv_sparse_grad.hip) trains on the sparse image(s) of symmetric operators (`_SparseOperators`): edge-list
batches (an untyped `ops.SparseLaplacian`), opt-in through `large_backward_impl`; typed ones (two
or more edge types: one image per operator channel; §4.9d) through `large_typed_backward_impl`; a DENSE collated
`L` beyond 128 nodes whose operators are symmetric, on the image(s) of the tensor, through
`large_dense_backward_impl` (§4.9e).

One regime per module: `_small` (<= 32 nodes, the fused kernels), `_mid` (33..128 nodes, one launch),
`_large` (beyond: streamed and sparse kernels, library GEMMs), `_ada` (AdaLanczosNet); `_common`
holds what they share.  This module composes them into `_LanczosNetBase`, which reads the
configuration, creates the parameters and picks the regime of a call (`_route`).
"""
import os
import warnings

import torch
import torch.nn as nn

from .. import ops
from ..utils.data_helper import check_dist
from ._common import (FUSED_MAX_NODES, FUSED_WIDTHS, LARGE_MAX_OPERATORS, MAX_CHANNELS, MAX_INPUT_DIM,
                      MAX_SHORT_SCALES, MID_MAX_NODES, STRIP_MAX_LONG_SCALES, STRIP_WIDTH, _CallPlumbing, _opt, input_state,
                      masked_readout)
from ._large import _LargeMixin, _LargeSparseFusedFunction, _SparseOperators
from ._mid import _MidGraphFusedFunction, _MidMixin
from ._small import _LanczosNetFunction, _LanczosNetFusedFunction, _SmallMixin

__all__ = ['LanczosNet', 'LanczosNetGeneral', 'AdaLanczosNet']

# the routes of `_LanczosNetBase._route` that train through an autograd.Function of their own
_TRAIN_FUNCTIONS = {'fused_train_hip': _LanczosNetFusedFunction, 'fused_train_torch': _LanczosNetFunction,
                    'mid_train_hip': _MidGraphFusedFunction, 'large_train_hip': _LargeSparseFusedFunction,
                    'large_typed_train_hip': _LargeSparseFusedFunction,
                    'large_dense_train_hip': _LargeSparseFusedFunction,
                    'large_dense_channels_train_hip': _LargeSparseFusedFunction}


class _LanczosNetBase(_SmallMixin, _MidMixin, _LargeMixin, _CallPlumbing, nn.Module):
    general = False
    filter_kind = 0                      # 0: diagonal gains on Ritz vectors, 1: dense (Ada)
    # 'fp32' (default): exact fp32 MFMA.  'f16x3': opt-in split precision inside the strip kernel (x_hi
    # w_hi + x_lo w_hi + x_hi w_lo on fp16 MFMA, fp32 accumulate, for GEMM1 and the block products;
    # 1e-6 .. 2e-6 vs fp64, parity bar 1e-5) — see DESIGN.md §4.7
    gemm_mode = os.environ.get('LANCZOSNET_GEMM', 'fp32')
    # spectral-filter MLP gradients in the HIP backward: 'hip' = lnz_spectral_mlp_grad (one launch),
    # 'torch' = autograd through batched library GEMMs (the oracle that kernel is tested against)
    mlp_grad_impl = os.environ.get('LANCZOSNET_MLP_GRAD', 'hip')
    # readout-head gradients in the HIP backward: 'hip' = lnz_head_backward (one launch), 'torch' =
    # autograd on the stored last state (the oracle that kernel is tested against)
    head_grad_impl = os.environ.get('LANCZOSNET_HEAD_GRAD', 'hip')
    # 'hip' = HIP backward kernels where built (LanczosNet, width 128); 'torch' = autograd through
    # the torch recomputation everywhere (the gradient oracle the HIP backward is tested against)
    backward_impl = os.environ.get('LANCZOSNET_BACKWARD', 'hip')
    _spectral_hidden = 128               # model/lanczos_net.py:50-56
    last_route = None                    # the `_route` name of the latest forward

    def _spectral_io(self):
        return self.num_scale_long

    def __init__(self, config):
        super().__init__()
        m = config.model
        self.config = config
        self.input_dim = m.input_dim
        self.hidden_dim = list(m.hidden_dim)
        self.output_dim = m.output_dim
        self.num_layer = m.num_layer
        self._read_dataset(config.dataset)
        self.dropout = _opt(m, 'dropout', 0.0)
        short, long_, num_eig, kind = self._diffusion_conf(m)
        self.short_diffusion_dist = check_dist(short)
        self.long_diffusion_dist = check_dist(long_)
        self.max_short_diffusion_dist = max(self.short_diffusion_dist, default=None)
        self.max_long_diffusion_dist = max(self.long_diffusion_dist, default=None)
        self.num_scale_short = len(self.short_diffusion_dist)
        self.num_scale_long = len(self.long_diffusion_dist)
        self.num_eig_vec = num_eig
        self.spectral_filter_kind = kind

        self._override_dims()
        widths = [self.input_dim] + self.hidden_dim + [self.output_dim]
        n_chan = self.num_scale_short + self.num_scale_long + self.num_edgetype + 1
        # creation order == reference (RNG parity): conv mixes, head, [embedding], spectral MLPs, gate
        mixes = [nn.Linear(widths[t] * n_chan, widths[t + 1]) for t in range(self.num_layer)]
        self.filter = nn.ModuleList(mixes + [nn.Linear(widths[-2], widths[-1])])
        self._make_input_layer()
        if self._has_mlp():
            fin, H = self._spectral_io(), self._spectral_hidden
            self.spectral_filter = nn.ModuleList([
                nn.Sequential(nn.Linear(fin, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(),
                              nn.Linear(H, H), nn.ReLU(), nn.Linear(H, fin))
                for _ in range(self.num_layer)])
        self.att_func = nn.Sequential(nn.Linear(widths[-2], 1), nn.Sigmoid())

        losses = {'CrossEntropy': nn.CrossEntropyLoss, 'MSE': nn.MSELoss, 'L1': nn.L1Loss}
        if m.loss not in losses:
            raise ValueError("Non-supported loss function!")
        self.loss_func = losses[m.loss]()
        self._init_param()
        self._plan_cache = None

    # -- configuration hooks ------------------------------------------------------------
    def _override_dims(self):
        pass

    def _channel_order(self):
        """Reference column-block index of each KERNEL message channel (kernel order: short, long,
        edge types) — None when the reference concatenates in that order (model/lanczos_net.py:
        164-180); the DCNN baseline puts the edge types first (model/dcnn.py:90-97)."""
        return None

    def _mix_weight(self, t):
        """Weight of conv layer t with its column blocks in kernel channel order (differentiable)."""
        w = self.filter[t].weight
        order = self._channel_order()
        if order is None:
            return w
        d = w.shape[1] // len(order)
        return w.view(w.shape[0], len(order), d)[:, order, :].reshape(w.shape[0], -1)

    def _to_reference_channel_order(self, dW):
        order = self._channel_order()
        if order is None:
            return dW
        d = dW.shape[1] // len(order)
        inv = [order.index(i) for i in range(len(order))]
        return dW.view(dW.shape[0], len(order), d)[:, inv, :].reshape(dW.shape[0], -1)

    def _diffusion_conf(self, m):
        """(short distances, long distances, K, spectral filter kind) from the model config."""
        return (list(m.short_diffusion_dist), list(m.long_diffusion_dist), m.num_eig_vec,
                m.spectral_filter_kind)

    def _guard_forward(self, L, mask):
        if mask is None:
            raise ValueError('forward needs `mask` (model/lanczos_net.py:192)')
        dev = self.filter[0].weight.device
        if dev.type != 'cuda':
            raise RuntimeError('lanczosnet_amd models run on the AMD GPU only: move the '
                               'module and its inputs to cuda (no CPU fallback)')
        return dev

    def invalidate_plan(self):
        """Drop the packed-parameter plans.  They are keyed on (data_ptr, tensor version) of every
        parameter, which in-place writes through `.data` (`p.data.clamp_()`, EMA copies, the
        reference's own `_init_param` idiom) do NOT bump: call this after such a write.
        `load_state_dict` and `.to()/.cuda()/.float()` call it themselves."""
        self._plan_cache = None
        self._plan_large_cache = None

    def _apply(self, fn, *a, **kw):
        self.invalidate_plan()
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self.invalidate_plan()
        return super().load_state_dict(*a, **kw)

    def _read_dataset(self, ds):
        self.num_atom = ds.num_atom
        self.num_edgetype = ds.num_bond_type

    def _make_input_layer(self):
        self.embedding = nn.Embedding(self.num_atom, self.input_dim)

    def _has_mlp(self):
        return self.spectral_filter_kind == 'MLP' and self.num_scale_long > 0

    def _init_param(self):
        # model/lanczos_net.py:74-93: Xavier-uniform weights, zero biases; embedding keeps N(0,1)
        groups = [list(self.filter), list(self.att_func)]
        if self._has_mlp():
            groups.append([f for seq in self.spectral_filter for f in seq])
        for group in groups:
            for layer in group:
                if isinstance(layer, nn.Linear):
                    nn.init.xavier_uniform_(layer.weight.data)
                    if layer.bias is not None:
                        layer.bias.data.zero_()

    # -- packed-parameter plan ------------------------------------------------------------
    def _param_signature(self):
        return (self.gemm_mode,) + tuple((p.data_ptr(), p._version, str(p.device))
                                         for p in self.parameters())

    # -- which regime serves a call ---------------------------------------------------------------
    def _strip_widths_ok(self):
        """Uniform hidden width 128, input width <= 128: the widths of every kernel but the 64-wide
        fused forward."""
        return (set(self.hidden_dim[:self.num_layer]) == {STRIP_WIDTH}
                and self.input_dim <= MAX_INPUT_DIM)

    def _route(self, N, K, channels, needs_grad, drop, capturing, sparse_one_operator=False,
               sparse_typed_operators=False, *, dense_one_operator=False, dense_channel_operators=False,
               inputs_grad=False):
        """The path `forward` takes for graphs of N nodes, K Ritz pairs and `channels` operator
        channels (needs_grad: `_needs_grad()`; drop: dropout > 0 in training; capturing: the
        current stream is being captured into a HIP graph; sparse_one_operator: L is an untyped
        SparseLaplacian — one operator as a sparse image with its fp32 values — and the image raised
        no flag; sparse_typed_operators: L is a typed SparseLaplacian — `channels` = 3 .. 8 distinct operators,
        one sparse image each with its fp32 values — and the images raised no flag; dense_one_operator: L is a dense
        float32 tensor on the device whose channels are ONE symmetric operator, its clean image with values riding
        on it; dense_channel_operators: ... whose 3 .. 8 channels are distinct symmetric operators under
        `large_sparse_channels == 'each'`, their images riding on it — `_dense_operators`; inputs_grad: autograd
        is on and a floating input of the call — node_feat, L, D or V — requires grad: the HIP backward passes
        treat the inputs as data, so such a call is 'torch' whatever else holds).  No GPU needed to ask.
          'fused'              <= 32 nodes: the fused MFMA kernels (`_hip_forward`)
          'fused_train_hip'    ... training, HIP backward (`_LanczosNetFusedFunction`)
          'fused_train_torch'  ... training, backward through `_torch_forward` (`_LanczosNetFunction`)
          'mid'                33..128 nodes in one launch (`_mid_graph_forward_hip`)
          'mid_train_hip'      ... training, opted in (`_MidGraphFusedFunction`)
          'large_hip'          > 32 nodes: the streamed / sparse kernels (`_large_graph_forward_hip`)
          'large_train_hip'    ... an edge-list batch in training, opted in (`_LargeSparseFusedFunction` on
                               the batch's image: one operator)
          'large_typed_train_hip'  ... a typed edge-list batch in training, opted in (the same Function on
                               the batch's images: one operator per channel)
          'large_dense_train_hip'  > 128 nodes: a dense L of one symmetric operator class in training, opted in
                               (the same Function on the tensor's image)
          'large_dense_channels_train_hip'  ... of 3 .. 8 distinct symmetric channels, opted in
                               (the same Function on the tensor's images)
          'library'            > 32 nodes or an architecture outside the fused kernels, inference:
                               hipBLASLt conv + HIP spectral gains (`_large_graph_forward`)
          'torch'              gradients or dropout outside the kernels, or gradients for an input:
                               `_torch_forward`"""
        if inputs_grad:
            return 'torch'
        if (N <= FUSED_MAX_NODES and not drop and self._fused_supported()
                and self._fused_channels_ok()):
            if not needs_grad:
                return 'fused'
            return 'fused_train_hip' if self._fused_backward_supported() else 'fused_train_torch'
        if needs_grad and not drop and not capturing and self._mid_backward_supported(N, K, channels):
            return 'mid_train_hip'
        if (needs_grad and not drop and not capturing and sparse_one_operator and N > FUSED_MAX_NODES
                and self._large_backward_supported(K, channels)):
            return 'large_train_hip'
        if (needs_grad and not drop and not capturing and sparse_typed_operators and N > FUSED_MAX_NODES
                and self._large_typed_backward_supported(K, channels)):
            return 'large_typed_train_hip'
        if (needs_grad and not drop and not capturing and N > MID_MAX_NODES
                and (dense_one_operator or dense_channel_operators)
                and self._large_dense_backward_supported(K, channels)):
            if dense_one_operator:
                return 'large_dense_train_hip'
            if self.large_sparse_channels == 'each' and 3 <= channels <= LARGE_MAX_OPERATORS:
                return 'large_dense_channels_train_hip'
        if needs_grad or drop:
            return 'torch'
        if self._mid_hip_supported(N, K, channels):
            return 'mid'
        if N > FUSED_MAX_NODES and self._large_hip_supported(K, channels):
            return 'large_hip'
        return 'library'

    def _warn_library_path(self, drop):
        """Once per module: a call of <= 32 nodes that the fused kernels do not serve."""
        if getattr(self, '_warned_library_path', False):
            return
        if drop:
            why = 'dropout=%r in training' % self.dropout
        elif not self._fused_supported():
            why = 'hidden_dim=%r / input_dim=%r' % (self.hidden_dim, self.input_dim)
        else:
            why = '%d short + %d long scales + %d operator channels' % (
                self.num_scale_short, self.num_scale_long, self.num_edgetype + 1)
        warnings.warn('lanczosnet_amd: %s is outside the fused MFMA kernel (uniform width %d '
                      'or %d, <= %d short and <= %d long scales, <= %d channels in all, no '
                      'training dropout): using the device library-GEMM path '
                      '(hipBLASLt conv + HIP spectral gains; differentiable torch ops when '
                      'gradients or dropout are needed), which is slower'
                      % ((why,) + FUSED_WIDTHS + (MAX_SHORT_SCALES, STRIP_MAX_LONG_SCALES, MAX_CHANNELS)))
        self._warned_library_path = True

    def _torch_forward(self, node_feat, L, D, V, mask, dropout=False):
        """Differentiable torch restatement of the same math (device tensors, channel-major L,
        `M_c (X W_c^T)` association).  Used inside backward to obtain parameter gradients where no
        HIP backward is built, and as the training forward of architectures outside the fused
        kernels (widths other than a uniform 64/128, N > 32, dropout > 0).  `dropout=True` applies
        `F.dropout(state, p)` after every conv layer exactly where the reference does
        (model/lanczos_net.py:182): same call, same shape, same order, so the device generator
        is consumed like the reference consumes it on this device."""
        B, N = L.shape[0], L.shape[1]
        Lc = L.float().permute(0, 3, 1, 2).contiguous()          # [B, E+1, N, N]
        Vf, Vt = V.float(), V.float().transpose(1, 2)
        state = input_state(self, node_feat)
        S = self.num_scale_long
        if S > 0:
            pows = torch.stack([torch.pow(D.float(), p) for p in self.long_diffusion_dist], dim=2)
        for t in range(self.num_layer):
            W, bias = self._mix_weight(t), self.filter[t].bias
            d_in = state.shape[2]
            Wc = W.view(W.shape[0], -1, d_in)                       # [dout, C, d_in]
            # X W_c^T per channel.  unbind, not `Z[:, c]`: the backward of a select allocates and adds a
            # zero tensor of the WHOLE [B, C, N, dout] block per channel (15 x 200 MB per layer at
            # B = 1024), the backward of unbind is one stack
            Z = torch.einsum('bnd,ocd->bcno', state, Wc).unbind(1)   # C x [B, N, dout]
            out = bias.view(1, 1, -1).expand(B, N, -1)
            c = 0
            if self.num_scale_short > 0:
                for p in self.short_diffusion_dist:
                    z = Z[c]
                    for _ in range(p):
                        z = torch.bmm(Lc[:, 0], z)
                    out = out + z
                    c += 1
            if S > 0:
                G = pows if self.spectral_filter_kind != 'MLP' else \
                    self.spectral_filter[t](pows.view(-1, S)).view(B, -1, S)   # [B, K, S]
                for s_ in range(S):
                    y = torch.bmm(Vt, Z[c])                                   # [B, K, dout]
                    out = out + torch.bmm(Vf, G[:, :, s_].unsqueeze(2) * y)
                    c += 1
            for e in range(self.num_edgetype + 1):
                out = out + torch.bmm(Lc[:, e], Z[c])
                c += 1
            state = torch.relu(out)
            if dropout:
                state = torch.nn.functional.dropout(state, self.dropout, training=True)
        return masked_readout(self, state, mask)

    def forward(self, node_feat, L, D, V, label=None, mask=None):
        """Shapes as the reference docstring (model/lanczos_net.py:125-141): node_feat B x N
        (long) [General: B x N x D float], L B x N x N x (E+1), D B x K, V B x N x K,
        label B x P, mask B x N.  Returns score, or (score, loss) when `label` is given."""
        dev = self._guard_forward(L, mask)
        t = self._to_module_device(dev, node_feat=node_feat, L=L, D=D, V=V, label=label, mask=mask)
        node_feat, L, D, V, label, mask = (t[k] for k in ('node_feat', 'L', 'D', 'V', 'label', 'mask'))
        if any(d == 'inf' for d in self.short_diffusion_dist + self.long_diffusion_dist):
            raise NotImplementedError("diffusion distance 'inf' is not built in the HIP path")
        drop = self.training and self.dropout > 0.0
        ops.forget_autograd_kernel()   # (last_kernel(): the previous step's backward is history)
        N = L.shape[1]
        capturing = torch.cuda.is_current_stream_capturing()
        # (a differentiable input: no route but 'torch' can answer, the batch's images are not examined)
        diff = self._differentiable_inputs(node_feat=node_feat, L=L, D=D, V=V)
        dense = None if diff else self._dense_operators(L, V.shape[2], drop, capturing)
        route = self._route(N, V.shape[2], L.shape[3], self._needs_grad(node_feat, L, D, V), drop, capturing,
                            sparse_one_operator=not diff and self._sparse_one_operator(L, drop, capturing),
                            sparse_typed_operators=not diff and self._sparse_typed_operators(L, drop, capturing),
                            dense_one_operator=dense == 'one', dense_channel_operators=dense == 'each',
                            inputs_grad=bool(diff))
        self.last_route = route
        if diff:
            self._warn_differentiable_inputs(diff)
        if isinstance(L, ops.SparseLaplacian):
            # the batch of dataset.collate_graph_edges: its image serves the sparse large-graph
            # layers; every other route reads the dense tensor
            if L.channels != self.num_edgetype + 1:
                raise ValueError('the SparseLaplacian batch has %d operator channels (num_edge_type = %d), the '
                                 'model num_edgetype + 1 = %d' % (L.channels, L.channels - 1, self.num_edgetype + 1))
            if L.device != dev:
                L = L.to(dev)
            if route not in ('large_hip', 'large_train_hip', 'large_typed_train_hip') or capturing:
                L = self._densify(L, "route '%s'" % route)
        if N <= FUSED_MAX_NODES and not route.startswith('fused') and not diff:
            self._warn_library_path(drop)
        if _TRAIN_FUNCTIONS.get(route) is _LargeSparseFusedFunction:
            # (the batch's own image(s), or those `_dense_operators` left riding on the tensor)
            L = _SparseOperators(L, each=route == 'large_dense_channels_train_hip')
        if route in _TRAIN_FUNCTIONS:
            # forward = HIP kernels keeping their states (runner/qm8_runner.py:216-248); backward =
            # HIP kernels + library GEMMs where built, else autograd through a torch recomputation
            score = _TRAIN_FUNCTIONS[route].apply(self, node_feat, L, D, V, mask, *self.parameters())
        elif route == 'torch':
            # the reference trains arbitrary widths / sizes: differentiate the device-side
            # torch restatement (same association as the kernels)
            score = self._torch_forward(node_feat, L, D, V, mask, dropout=drop)
        elif route == 'large_hip':
            # hand-written streaming kernels; 'bf16' = config 5's bf16-operand mode
            score = self._large_graph_forward_hip(
                node_feat, L, D, V, mask, planes=1 if self.gemm_mode == 'bf16' else self.large_split_planes)
        else:
            run = {'fused': self._hip_forward, 'mid': self._mid_graph_forward_hip,
                   'library': self._large_graph_forward}[route]
            score = run(node_feat, L, D, V, mask)
        if label is not None:
            return score, self.loss_func(score, label)
        return score


class LanczosNet(_LanczosNetBase):
    """QM8 model: integer atom ids through nn.Embedding (model/lanczos_net.py:44,154)."""


class LanczosNetGeneral(_LanczosNetBase):
    """Float node features, no embedding (model/lanczos_net_general.py:22-24,45-46,156)."""
    general = True

    def _read_dataset(self, ds):
        self.node_emb_dim = ds.node_emb_dim
        self.graph_emb_dim = ds.graph_emb_dim
        self.num_edgetype = ds.num_edge_type

    def _make_input_layer(self):
        assert self.input_dim == self.node_emb_dim
        assert self.output_dim == self.graph_emb_dim


from ._ada import AdaLanczosNet  # noqa: E402  (it derives from _LanczosNetBase above)
