"""What the regime modules of LanczosNet share: the small tensor helpers of the backward passes and
the ONE implementation of each piece of arithmetic that the regimes have in common (layer-0 state,
stacked readout head, masked-mean readout, embedding gradient, the parameter-gradient tuple).

Several tests and benchmark fields compare bit for bit across the regimes' routes: where two
callers need different operands (a detached lookup, a cast, the live parameters) the helper takes
an explicit argument; it never picks one caller's behaviour for both."""
import warnings

import torch
import torch.nn as nn

from .. import ops


# -- the envelopes of the kernels ---------------------------------------------------------------
# Every numeric limit of a route predicate is written HERE and nowhere else: the predicates of the
# regime modules, `_LanczosNetBase._route` and the texts of the library-path warnings read these.
# (The sixteen long scales of the gains kernels are the class attribute `gains_kernel_max_scales`.)
FUSED_MAX_NODES = 32        # one 32-row MFMA tile of nodes: csrc/conv_forward.hip, conv_strip.hip
FUSED_WIDTHS = (64, 128)    # uniform hidden width of the fused forward
STRIP_WIDTH = 128           # ... of the strip kernels, the HIP backward and the > 32-node kernels
MAX_INPUT_DIM = 128
MAX_OUTPUT_DIM = 31         # head rows + the gate's row: one 32-row tile
MAX_SHORT_SCALES = 8        # csrc/conv_forward.hip launch_conv
STRIP_MAX_LONG_SCALES = 12  # csrc/conv_strip.hip strip_forward_eligible
MAX_CHANNELS = 32           # message channels in all
MID_MAX_NODES = 128         # csrc/conv_mid.hip
MID_MAX_K = 32
MID_MAX_OPERATORS = 2
LARGE_MAX_K = 64            # csrc/conv_large.hip
LARGE_MAX_OPERATORS = 8     # the pack kernel's channel map (`LargeChanMap`)


def _opt(node, key, default):
    return getattr(node, key) if hasattr(node, key) else default


# -- what every module of the package asks of a call --------------------------------------------
def _requires_grad(t):
    return isinstance(t, torch.Tensor) and t.is_floating_point() and t.requires_grad


class _CallPlumbing:
    """Mixed into LanczosNet and the baseline modules: does the call need gradients, and are its inputs
    where the module is."""

    def _needs_grad(self, *inputs):
        """A parameter requires grad, or one of the call's floating tensors `inputs` does (features from an
        upstream encoder, a learned operator): either way the score has to carry a graph."""
        if not torch.is_grad_enabled():
            return False
        return any(p.requires_grad for p in self.parameters()) or any(map(_requires_grad, inputs))

    @staticmethod
    def _differentiable_inputs(**tensors):
        """Names of the floating tensors among `tensors` that require grad ([] where autograd is off).  The
        hand-written backward passes treat every input as data, so a call with one of these is served by the
        differentiable torch restatement (the training switches)."""
        if not torch.is_grad_enabled():
            return []
        return [k for k, t in tensors.items() if _requires_grad(t)]

    def _warn_differentiable_inputs(self, names):
        """Once per module: the call left the HIP routes because an input requires grad."""
        if not getattr(self, '_warned_differentiable_inputs', False):
            self._warned_differentiable_inputs = True
            warnings.warn('lanczosnet_amd: input(s) %s require grad; the HIP training routes treat the inputs as '
                          'data, so this call takes the differentiable torch restatement, which is slower '
                          '(detach the inputs to stay on the HIP route)' % ', '.join(names))

    def _to_module_device(self, dev, **tensors):
        """`QM8Runner.test` moves only `D, V` to the GPU and hands over a HOST `L` (and, like every
        loop of the runner, host-side nothing else) — runner/qm8_runner.py:301-302; the reference
        model then fails inside `bmm`.  A drop-in should not: inputs that are not on the module's
        device are moved there, with one warning per module."""
        out, moved = {}, []
        for k, t in tensors.items():
            if isinstance(t, torch.Tensor) and t.device != dev:
                moved.append(k)
                t = t.to(dev, non_blocking=True)
            out[k] = t
        if moved and not getattr(self, '_warned_host_inputs', False):
            warnings.warn('lanczosnet_amd: input(s) %s were not on %s and were moved there '
                          '(reference runner/qm8_runner.py:301-302 leaves L on the host); keep the '
                          'batch resident on the GPU to avoid the copy' % (', '.join(moved), dev))
            self._warned_host_inputs = True
        return out


# -- layer-0 state ---------------------------------------------------------------------------
def input_state(m, node_feat, width=None, detached=False, as_float=False):
    """Node state entering conv layer 0: the float features (General) or the embedding rows.
    detached: index the detached table instead of calling the Embedding (no autograd node);
    as_float: cast the looked-up rows to fp32; width: zero-pad the columns to that many."""
    if m.general:
        x = node_feat.float()
    else:
        x = m.embedding.weight.detach()[node_feat] if detached else m.embedding(node_feat)
        if as_float:
            x = x.float()
    if width is not None and x.shape[2] != width:
        x = torch.nn.functional.pad(x, (0, width - x.shape[2]))
    return x


# -- readout head (model/lanczos_net.py:185-194) -----------------------------------------------
def head_parts(m):
    """(output weight, output bias, gate weight, gate bias): the live parameters of the readout."""
    return m.filter[-1].weight, m.filter[-1].bias, m.att_func[0].weight, m.att_func[0].bias


def head_params(m, live=False):
    """Output Linear and gate Linear as ONE operand: weight [P + 1, dh] (the gate's row last) and
    bias [P + 1].  live: stacked from the parameters themselves, so that autograd reaches them;
    else from detached fp32 copies (what the packed plans keep)."""
    Wo, bo, Wg, bg = head_parts(m)
    if live:
        return torch.cat([Wo, Wg], dim=0), torch.cat([bo, bg], dim=0)
    return (torch.cat([Wo.detach().float(), Wg.detach().float()]).contiguous(),
            torch.cat([bo.detach().float(), bg.detach().float()]).contiguous())


def masked_readout(m, state, mask, stacked=None):
    """score [B, P] = mean over the real nodes of head(state) * gate(state).  stacked = (W, b) of
    `head_params`: head and gate as one product Z = state W^T + b, y = Z[:P] * sigmoid(Z[P:])
    (three library GEMMs forward + backward instead of six thin ones; every output column is the
    same dot product either way) — the form the backward passes differentiate."""
    if stacked is None:
        y = m.filter[-1](state)
        y = y * m.att_func(state)
    else:
        P = m.output_dim
        Z = torch.nn.functional.linear(state, stacked[0], stacked[1])
        y = Z[..., :P] * torch.sigmoid(Z[..., P:])
    mk = (mask != 0).float().unsqueeze(2)
    return (y * mk).sum(dim=1) / mk.sum(dim=1)


def scatter_head_grads(m, grads, dWh, dbh):
    """Rows of the stacked head gradient (dWh [P + 1, dh], dbh [P + 1]) into `grads` by parameter."""
    P = m.output_dim
    Wo, bo, Wg, bg = head_parts(m)
    grads[id(Wo)], grads[id(bo)] = dWh[:P], dbh[:P]
    grads[id(Wg)], grads[id(bg)] = dWh[P:], dbh[P:]


# -- parameter gradients ---------------------------------------------------------------------
def embedding_grad(m, node_feat, dx0, N, din0):
    """Gradient of the embedding table from dX_0 [B, >= N, >= din0]: lnz_embedding_grad (rows of
    dX_0 added by atom id, no atomics) at the widths it is built for, else one-hot^T dX_0 as a GEMM
    (index_add's atomics are 10x slower here)."""
    if din0 in (16, 32, 64, 128):
        return ops.embedding_grad(node_feat.contiguous(), dx0, din0, m.num_atom)
    onehot = torch.nn.functional.one_hot(node_feat.reshape(-1), m.num_atom).to(torch.float32)
    return onehot.t() @ dx0[:, :N, :din0].reshape(-1, din0)


def param_grad_tuple(m, grads, n_leading):
    """What an autograd.Function's backward returns: None for the `n_leading` non-parameter inputs,
    then `grads` (by id(parameter)) in `m.parameters()` order."""
    out = [grads.get(id(p_)) if p_.requires_grad else None for p_ in m.parameters()]
    return (None,) * n_leading + tuple(out)


def torch_param_grads(m, score, grad_score):
    """-> grads by id(parameter): autograd of a torch restatement's `score`."""
    need = [p for p in m.parameters() if p.requires_grad]
    return dict(zip(map(id, need),
                    torch.autograd.grad(score, need, grad_score.contiguous(), allow_unused=True)))


# -- spectral-filter MLPs ----------------------------------------------------------------------
def spectral_mlp_operands(m):
    """Per conv layer the (weight, bias) of the four Linears of its filter MLP: the operand list
    of ops.pack_spectral_mlp_layers."""
    return [[(seq[i].weight, seq[i].bias) for i in (0, 2, 4, 6)] for seq in m.spectral_filter]


def is_reference_filter_mlp(seq):
    """The reference's filter MLP: Linear, ReLU, Linear, ReLU, Linear, ReLU, Linear."""
    return len(seq) == 7 and all(isinstance(seq[i], nn.Linear) for i in (0, 2, 4, 6))


def _linear_relu(x, w, b):
    """relu(x w^T + b) as ONE library launch where torch exposes the fused epilogue."""
    f = getattr(torch, '_addmm_activation', None)
    if f is not None and b is not None and x.dim() == 2:
        return f(b, x, w.t())
    return torch.relu_(torch.nn.functional.linear(x, w, b))


class _BatchedLinear(torch.autograd.Function):
    """y[l] = x[l] W[l]^T + b[l] for the stacked spectral-filter MLPs of all conv layers
    (x [L, R, i], W [L, o, i], b [L, o]).  torch's own backward of the broadcast bias is a
    reduction over the [L, R, o] block (88 us per Linear at R = 20 k, three of them per step);
    here the bias gradient is one thin batched GEMM, ones^T g."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        return torch.baddbmm(b.unsqueeze(1), x, W.transpose(1, 2))

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.bmm(g, W) if ctx.needs_input_grad[0] else None
        dW = torch.bmm(g.transpose(1, 2), x)
        ones = g.new_ones((g.shape[0], 1, g.shape[1]))
        db = torch.bmm(ones, g).squeeze(1)
        return dx, dW, db


def _tn_split_k(a, b, splits=4):
    """a^T b for tall operands a [R, m], b [R, n] (the conv weight gradient: m = 128, n = 1920,
    R = every node row of the batch).  One library GEMM tiles the small m x n output into ~60
    workgroups; as `splits` batched partial products over row slices it fills the chip
    (200 -> 125 us at R = 26.6 k on an MI355X), the partials are summed in a fixed order."""
    R = a.shape[0]
    if R < 8192:
        return a.t() @ b
    Rs = R // splits
    part = torch.bmm(a[:splits * Rs].view(splits, Rs, a.shape[1]).transpose(1, 2),
                     b[:splits * Rs].view(splits, Rs, b.shape[1]))
    out = part.sum(dim=0)
    if splits * Rs < R:  # the last R % splits rows
        out = out + a[splits * Rs:].t() @ b[splits * Rs:]
    return out


def _spectral_mlp_param_grads(m, grads, D, dG, live_rows=None, n_live=None, static_rows=True, rtot=None):
    """Gradients of the spectral-filter MLPs (model/lanczos_net.py:95-123) from dG [L, B*K, S] into
    `grads` (by id(parameter)): lnz_spectral_mlp_grad in one launch (S <= 8), else autograd through
    the batched MLP.  live_rows / n_live: the eigen rows the gains were evaluated on (None: all);
    rtot: the host's copy of the node-row total that bounds their number (static_rows: not read)."""
    B, K = D.shape
    S, Lnum, dev = m.num_scale_long, m.num_layer, D.device
    lin_idx = ([i for i, mod in enumerate(m.spectral_filter[0]) if isinstance(mod, nn.Linear)]
               if S > 0 and m._has_mlp() else [])
    if (S > 0 and m._has_mlp() and m.mlp_grad_impl == 'hip' and S <= 8 and len(lin_idx) == 4
            and dG.is_contiguous()):
        # one launch for every layer's MLP (csrc/spectral_gains_grad.hip): forward recomputation,
        # the chain of ReLU masks and all eight parameter gradients on chip, live rows only
        layers = [[(m.spectral_filter[t][i].weight, m.spectral_filter[t][i].bias) for i in lin_idx]
                  for t in range(Lnum)]
        rows_max = B * K
        if live_rows is not None and not static_rows:
            rows_max = min(int(rtot[0]), B * K)   # (sum of node extents >= live eigen rows)
        try:
            gl = ops.spectral_mlp_grad(D.float(), m.long_diffusion_dist, layers, dG,
                                       rows=(live_rows, n_live) if live_rows is not None else None,
                                       rows_max=rows_max)
        except ops.NotSupported:
            # (a part without 160 KiB of LDS per workgroup: lnz::set_dynamic_lds says so) —
            # the library-GEMM branch below serves it from now on
            gl = None
            m.mlp_grad_impl = 'torch'
        for li, i in enumerate(lin_idx if gl is not None else ()):
            for t in range(Lnum):
                grads[id(m.spectral_filter[t][i].weight)] = gl[li][0][t]
                grads[id(m.spectral_filter[t][i].bias)] = gl[li][1][t]
    if S > 0 and m._has_mlp() and id(m.spectral_filter[0][lin_idx[0]].weight) not in grads:
        # (a frozen MLP tensor gets no gradient: autograd.grad refuses one that does not require grad)
        mlp_params = [p_ for p_ in ([m.spectral_filter[t][i].weight for i in lin_idx for t in range(Lnum)] +
                                    [m.spectral_filter[t][i].bias for i in lin_idx for t in range(Lnum)])
                      if p_.requires_grad]
        if not mlp_params:
            return
        pows = torch.stack([torch.pow(D.float(), p) for p in m.long_diffusion_dist],
                           dim=2).view(B * K, S)
        if live_rows is not None and not static_rows:
            # only the eigen slots that carry a Ritz pair have a gradient (dG is zero elsewhere):
            # the first n_live entries of the plan's row list; the host knows an upper bound of
            # their number without a round trip (sum of node extents >= sum of min(n, K)) — the
            # tail of the gathered block is masked.  [S = 8 columns: the gathers are cheap; the
            # MLP forward + backward shrink from B K = 20.5 k to ~17 k rows]
            R_live = min(int(rtot[0]), B * K)
            idx = live_rows[:R_live].long().clamp_(0, B * K - 1)
            keep = (torch.arange(R_live, device=dev) < n_live.long()).to(dG.dtype)
            pows = pows.index_select(0, idx)
            dG = dG.index_select(1, idx) * keep.view(1, R_live, 1)
        pows = pows.unsqueeze(0).expand(Lnum, pows.shape[0], S)
        with torch.enable_grad():
            h = pows
            for li, i in enumerate(lin_idx):
                Wst = torch.stack([m.spectral_filter[t][i].weight for t in range(Lnum)])
                bst = torch.stack([m.spectral_filter[t][i].bias for t in range(Lnum)])
                h = _BatchedLinear.apply(h, Wst, bst)
                if li + 1 < len(lin_idx):
                    h = torch.relu(h)
            gg = torch.autograd.grad(h, mlp_params, dG)
        for p_, g_ in zip(mlp_params, gg):
            grads[id(p_)] = g_
