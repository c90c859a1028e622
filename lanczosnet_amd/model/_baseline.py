"""What the four baseline modules (GAT, GGNN, MPNN, GPNN) share: the loss table, the reference's two init
idioms, the packed-operand caches keyed on the parameter versions, and the way a call finds its route.

A subclass keeps its constructor (module creation order is the reference's: the RNG draws and
`named_parameters()` line up), the quirks of its `_init_param`, its operands, the envelope checks of its
`_why_not_hip`, and its `_hip_forward`, `_hip_train_forward` (where a HIP backward exists) and
`_torch_forward`.  This class registers no module and no parameter."""
import warnings

import torch
import torch.nn as nn

from ._common import _CallPlumbing

LOSSES = {'CrossEntropy': nn.CrossEntropyLoss, 'MSE': nn.MSELoss, 'L1': nn.L1Loss}


class _Baseline(_CallPlumbing, nn.Module):
    _route_prefix = None              # the routes are '<prefix>_hip', '<prefix>_hip_train' and '<prefix>_torch'
    _hip_kernels = 'kernel'           # what the torch-route warning calls the HIP route's launches
    _cache_slots = ('_pack_cache',)   # what `invalidate_plan` drops, besides the parameter list

    def _finish_init(self, loss):
        """The tail of a constructor: the loss (registered last, as in the reference), the reference's init,
        empty caches."""
        if loss not in LOSSES:
            raise ValueError("Non-supported loss function!")
        self.loss_func = LOSSES[loss]()
        self._init_param()
        self.invalidate_plan()
        self.last_route = None

    # -- the reference's init idioms ----------------------------------------------------------------
    @staticmethod
    def _init_linears(layers):
        """Xavier-uniform weights, zero biases, for the nn.Linear among `layers`, in order"""
        for layer in layers:
            if isinstance(layer, nn.Linear):
                nn.init.xavier_uniform_(layer.weight.data)
                if layer.bias is not None:
                    layer.bias.data.zero_()

    @classmethod
    def _init_sequentials(cls, groups):
        """... for the nn.Sequential among `groups`: the reference's loop passes over everything else (a
        ModuleList, a Set2Vec, None), which keeps its own init"""
        for group in groups:
            if isinstance(group, nn.Sequential):
                cls._init_linears(group)

    @staticmethod
    def _init_cell(cell):
        nn.init.xavier_uniform_(cell.weight_hh.data)       # hh before ih, as in the reference
        nn.init.xavier_uniform_(cell.weight_ih.data)
        if cell.bias:
            cell.bias_hh.data.zero_()
            cell.bias_ih.data.zero_()

    # -- the packed operands, once per weight version -------------------------------------------------
    def _embedding_weight(self):
        return self.embedding.weight

    def _param_signature(self):
        """What the packed operands are keyed on: the tensor version of every parameter (an optimizer
        step or any other in-place update bumps it) and the device.  The parameter list is walked once per
        plan, not per call (GAT: 2,357 parameters at the yaml shape)."""
        if self._param_list is None:
            self._param_list = list(self.parameters())
        return (str(self._embedding_weight().device),) + tuple(p._version for p in self._param_list)

    def invalidate_plan(self):
        """Drop the packed operands (and, where the module has one, the [num_atom, D] table).  Writes that bump
        no tensor version (`p.data.clamp_()`, `p.data = x`, the reference's own `_init_param` idiom) and a
        parameter replaced by another object need this call.  `load_state_dict` and `.to()/.cuda()/.float()`
        call it themselves."""
        for slot in self._cache_slots:
            setattr(self, slot, None)
        self._param_list = None

    def _apply(self, fn, *a, **kw):
        self.invalidate_plan()
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self.invalidate_plan()
        return super().load_state_dict(*a, **kw)

    @torch.no_grad()
    def _cached(self, slot, build):
        """`build()` once per weight version, kept in the cache slot `slot`"""
        sig = self._param_signature()
        hit = getattr(self, slot)
        if hit is None or hit[0] != sig:
            hit = (sig, build())
            setattr(self, slot, hit)
        return hit[1]

    # -- which route serves a call ----------------------------------------------------------------
    def _why_not_hip_operands(self, L, C, graphs=()):
        """The tail of every `_why_not_hip`: L is float32 [B, N, N, C], each of `graphs` (name, tensor) float32
        [B, N, N], the parameters float32"""
        if L.dtype != torch.float32 or L.dim() != 4 or L.shape[3] != C:
            return 'L is %s %s, not float32 [B, N, N, %d]' % (L.dtype, tuple(L.shape), C)
        for name, t in graphs:
            if t.dtype != torch.float32 or t.dim() != 3:
                return '%s is %s %s, not float32 [B, N, N]' % (name, t.dtype, tuple(t.shape))
        if self._embedding_weight().dtype != torch.float32:
            return 'the parameters are %s, not float32' % self._embedding_weight().dtype
        return None

    def _guard_device(self):
        dev = self._embedding_weight().device
        if dev.type != 'cuda':
            raise RuntimeError('lanczosnet_amd models run on the AMD GPU only: move the '
                               'module and its inputs to cuda (no CPU fallback)')
        return dev

    def _dispatch(self, **inputs):
        """The tail of every `forward`.  inputs: node_feat, the graph tensors, `label`, mask last, in the order of
        the signature.  Everything goes to the module's device; `_why_not_hip(N, *graphs, needs_grad, drop)`
        picks the route, whose method gets (node_feat, *graphs, mask) -> score, or (score, loss) with a label."""
        dev = self._guard_device()
        inputs = self._to_module_device(dev, **inputs)
        label = inputs.pop('label')
        args = tuple(inputs.values())
        drop = self.training and self.dropout > 0
        needs_grad = self._needs_grad(*args)
        why = self._why_not_hip(args[0].shape[1], *args[1:-1], needs_grad, drop)
        # (the HIP backward returns no gradient for an input: the restatement differentiates through it, with
        # a warning of its own, once per module)
        diff = self._differentiable_inputs(**inputs) if why is None else []
        name, prefix = type(self).__name__, self._route_prefix
        if diff:
            self.last_route = prefix + '_torch'
            self._warn_differentiable_inputs(diff)
            score = self._torch_forward(*args, dropout=drop)
        elif why is None and needs_grad:
            self.last_route = prefix + '_hip_train'
            score = self._hip_train_forward(*args)
        elif why is None:
            self.last_route = prefix + '_hip'
            score = self._hip_forward(*args)
        else:
            self.last_route = prefix + '_torch'
            if not getattr(self, '_warned_torch_route', False):
                warnings.warn("lanczosnet_amd: %s takes the differentiable torch restatement (route '%s_torch', "
                              "slower than the HIP %s of route '%s_hip'): %s"
                              % (name, prefix, self._hip_kernels, prefix, why))
                self._warned_torch_route = True
            score = self._torch_forward(*args, dropout=drop)
        if label is not None:
            return score, self.loss_func(score, label)
        return score
