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
opt-in through `mid_backward_impl`.
"""
import os
import warnings

import torch
import torch.nn as nn

from .. import ops
from ..utils.data_helper import check_dist

__all__ = ['LanczosNet', 'LanczosNetGeneral', 'AdaLanczosNet']

_SPECTRAL_HIDDEN = 128  # model/lanczos_net.py:50-56


def _opt(node, key, default):
    return getattr(node, key) if hasattr(node, key) else default


class _LanczosNetBase(nn.Module):
    general = False
    filter_kind = 0                      # 0: diagonal gains on Ritz vectors, 1: dense (Ada)
    # 'fp32' (default): exact fp32 MFMA.  'f16x3': opt-in split precision inside the strip kernel (x_hi
    # w_hi + x_lo w_hi + x_hi w_lo on fp16 MFMA, fp32 accumulate, for GEMM1 and the block products;
    # 1e-6 .. 2e-6 vs fp64, parity bar 1e-5) — see DESIGN.md §4.7
    gemm_mode = os.environ.get('LANCZOSNET_GEMM', 'fp32')
    # graphs beyond 32 nodes, fp32-grade mode of the streamed kernels: 3 = three bf16 pieces per
    # operand (six products), 2 = two fp16 pieces (three products, 2/3 of the operand bytes)
    large_split_planes = int(os.environ.get('LANCZOSNET_LARGE_PLANES', '3'))
    # spectral-filter MLP gradients in the HIP backward: 'hip' = lnz_spectral_mlp_grad (one launch),
    # 'torch' = autograd through batched library GEMMs (the oracle that kernel is tested against)
    mlp_grad_impl = os.environ.get('LANCZOSNET_MLP_GRAD', 'hip')
    # readout-head gradients in the HIP backward: 'hip' = lnz_head_backward (one launch), 'torch' =
    # autograd on the stored last state (the oracle that kernel is tested against)
    head_grad_impl = os.environ.get('LANCZOSNET_HEAD_GRAD', 'hip')
    # 'hip' = HIP backward kernels where built (LanczosNet, width 128); 'torch' = autograd through
    # the torch recomputation everywhere (the gradient oracle the HIP backward is tested against)
    backward_impl = os.environ.get('LANCZOSNET_BACKWARD', 'hip')
    # graphs of 33..128 nodes in training: 'hip' = the backward of the one-launch kernel
    # (_MidGraphFusedFunction, csrc/conv_mid_grad.hip), 'torch' (default) = autograd through
    # `_torch_forward`.  Opt-in until its step time is recorded
    mid_backward_impl = os.environ.get('LANCZOSNET_MID_BACKWARD', 'torch')
    _spectral_hidden = _SPECTRAL_HIDDEN

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

    def _needs_grad(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

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

    def _fused_supported(self):
        """True when the fused MFMA kernel is built for this architecture (uniform hidden width
        64 or 128, input width <= 128, head width <= 31)."""
        hid = set(self.hidden_dim[:self.num_layer])
        return (len(hid) == 1 and next(iter(hid)) in (64, 128) and self.input_dim <= 128
                and self.output_dim <= 31)

    def _fused_channels_ok(self):
        """Scale and channel counts the fused forward kernels are built for (csrc/conv_forward.hip
        launch_conv, csrc/conv_strip.hip strip_forward_eligible): at most 8 short and 12 long
        diffusion scales, at most 32 message channels in all.  Beyond that the module takes the
        library path, like a width outside the kernels."""
        n_chan = self.num_scale_short + self.num_scale_long + self.num_edgetype + 1
        return self.num_scale_short <= 8 and self.num_scale_long <= 12 and n_chan <= 32

    def _check_supported(self):
        if any(d == 'inf' for d in self.short_diffusion_dist + self.long_diffusion_dist):
            raise NotImplementedError("diffusion distance 'inf' is not built in the HIP path")
        if not self._fused_supported():
            raise NotImplementedError(
                'fused kernel is built for a uniform hidden width of 64 or 128, input width <= 128, '
                'got hidden_dim=%r input_dim=%r' % (self.hidden_dim, self.input_dim))

    @torch.no_grad()
    def _plan(self):
        sig = self._param_signature()
        if self._plan_cache is not None and self._plan_cache['sig'] == sig:
            return self._plan_cache
        self._check_supported()
        dev = self.filter[0].weight.device
        dhid = self.hidden_dim[0]
        packs, biases, w_off, b_off, woff, boff = [], [], [], [], 0, 0
        # the kernels consume the input width in 32-column groups — 64-column groups for width-128
        # models, whose launches run on strips of 16-row subtiles (csrc/conv_strip.hip): zero-pad
        # layer-0 weight columns (per message channel) and the embedding / feature columns to match
        din0 = self.input_dim
        # gemm_mode 'f16x3' on the strip plan (csrc/conv_strip.hip, HALF): the same stream at the same
        # offsets, fp16 hi / lo pieces of the weights; every other operand is the exact kernel's
        split_strips = (self.gemm_mode == 'f16x3' and dhid == 128
                        and din0 <= 128 and self.filter_kind == 0 and self._tiles16_channels_ok()
                        and self.num_scale_short == 0 and self.output_dim <= 31)
        # (that kernel's weight ring is built for 128 input columns in every layer)
        group = 128 if split_strips else (64 if dhid == 128 else 32)
        din0p = (din0 + group - 1) // group * group
        n_chan = self.num_scale_short + self.num_scale_long + self.num_edgetype + 1
        # layer 0 has its own width; the other layers share a shape and are packed by one launch
        # (rows of the stacked matrix are whole 32-row tiles of each layer, so the pack of the
        # stack is the concatenation of the per-layer packs)
        w = self._mix_weight(0)
        if din0p != din0:
            w = torch.nn.functional.pad(w.view(dhid, n_chan, din0), (0, din0p - din0))
            w = w.reshape(dhid, n_chan * din0p)
        pack_conv = ops.pack_rows_k8_split if split_strips else ops.pack_rows_k8
        wp = pack_conv(w)
        packs.append(wp)
        w_off.append(0)
        woff = wp.numel()
        if self.num_layer > 1:
            stack = torch.cat([self._mix_weight(t) for t in range(1, self.num_layer)], dim=0)
            wps = pack_conv(stack)
            packs.append(wps)
            per = wps.numel() // (self.num_layer - 1)
            for t in range(1, self.num_layer):
                w_off.append(woff)
                woff += per
        for t in range(self.num_layer):
            biases.append(self.filter[t].bias.detach().float())
            b_off.append(boff)
            boff += dhid
        P = self.output_dim
        head = torch.zeros((32, dhid), dtype=torch.float32, device=dev)
        head[:P] = self.filter[-1].weight
        head[P] = self.att_func[0].weight[0]
        bias_head = torch.zeros((32,), dtype=torch.float32, device=dev)
        bias_head[:P] = self.filter[-1].bias
        bias_head[P] = self.att_func[0].bias[0]
        emb = None
        if not self.general:
            emb = torch.nn.functional.pad(self.embedding.weight.detach().float(),
                                          (0, din0p - din0)).contiguous()
        plan = dict(sig=sig, num_layer=self.num_layer, din0=din0p, din0_raw=din0, dhid=dhid,
                    dout=P, filter_kind=self.filter_kind,
                    short=list(self.short_diffusion_dist), n_long=self.num_scale_long,
                    n_edge=self.num_edgetype + 1,
                    # + slack: the kernel's weight prefetch ring over-reads up to 7 steps (7 KiB; the
                    # split-precision ring 8 slots per wave pair: 16 KiB)
                    Wp=torch.cat(packs + [torch.zeros(8192 if split_strips else 2048, dtype=torch.float32,
                                                      device=dev)]),
                    bias=torch.cat(biases).contiguous(),
                    w_off=w_off, b_off=b_off, Wp_head=ops.pack_rows_k8(head),
                    bias_head=bias_head,
                    embedding=emb)
        plan['gemm_mode'] = 1 if split_strips else 0
        if self.gemm_mode == 'f16x3' and not split_strips:
            raise NotImplementedError(
                "gemm_mode='f16x3' runs inside the strip kernel: LanczosNet / LanczosNetGeneral with "
                "hidden width 128, input width <= 128, no short-diffusion scales, <= 12 long scales, "
                "<= 32 channels in all, output width <= 31")
        if self.gemm_mode not in ('fp32', 'bf16', 'f16x3'):
            raise ValueError("gemm_mode must be 'fp32', 'f16x3' (N <= 32) or 'bf16' (N > 32)")
        if self._has_mlp() and self.filter_kind == 0:
            plan['mlp_pack'] = ops.pack_spectral_mlp_layers(
                [[(seq[i].weight, seq[i].bias) for i in (0, 2, 4, 6)]
                 for seq in self.spectral_filter], self.num_scale_long)
        else:
            plan['mlp_pack'] = None
        self._plan_cache = plan
        return plan

    # -- forward ----------------------------------------------------------------------------
    @torch.no_grad()
    def _hip_forward(self, node_feat, L, D, V, mask):
        plan = self._plan()
        mask_u8 = mask.to(torch.uint8).contiguous()
        Lp, tiles, rows = ops.pack_and_plan(plan, L, mask_u8, V.shape[2])
        G = None
        if self.num_scale_long > 0:
            G = ops.spectral_gains(D, self.long_diffusion_dist, self.num_layer, plan['mlp_pack'],
                                   rows=rows, zero_fill=not ops.pairing_supported(plan),
                                   split_pack=Lp if plan['gemm_mode'] == 1 else None)
            if plan['gemm_mode'] == 1:
                G, Lp = G   # (the gains and the pack's float16 form, written under the same launch)
        return ops.lanczosnet_forward(plan, node_feat, Lp, V, G, mask_u8, tiling=tiles)

    # lnz_spectral_gains / lnz_pack_spectral_mlp_layers: csrc/gains_body.hpp SMAX
    gains_kernel_max_scales = 16

    @torch.no_grad()
    def _torch_gains(self, D):
        """G [L,B,S,K] by library calls (model/lanczos_net.py:110-113,118-121,146-149): the gains
        of more long scales than the HIP gains kernel is built for."""
        S = self.num_scale_long
        B, K = D.shape
        pows = torch.stack([torch.pow(D.float(), p) for p in self.long_diffusion_dist], dim=2)
        if self._has_mlp():
            G = torch.stack([seq(pows.view(-1, S)).view(B, K, S) for seq in self.spectral_filter])
        else:
            G = pows.unsqueeze(0).expand(self.num_layer, B, K, S)
        return G.transpose(2, 3)

    @torch.no_grad()
    def _large_graph_forward(self, node_feat, L, D, V, mask, gemm_dtype=None):
        """Graphs beyond the 32-node MFMA tile (BASELINE config 5: N = 2048, K = 64).  The conv is
        then plain batched dense GEMMs (`L_e (X W_e^T)` with N x N operands), which go to
        hipBLASLt through torch.bmm; the spectral gains are the HIP kernel and the Ritz pairs come
        from `lnz_lanczos_ritz_large`.  `gemm_dtype=torch.bfloat16` runs the edge-type GEMMs with
        bf16 operands / fp32 accumulate (config 5's "bf16 MFMA filter GEMM"); default fp32."""
        B, N = L.shape[0], L.shape[1]
        S = self.num_scale_long
        G = None
        if S > self.gains_kernel_max_scales:
            G = self._torch_gains(D)                                  # [L,B,S,K]
        elif S > 0:
            plan_mlp = self._plan_large()['mlp_pack'] if self._has_mlp() else None
            G = ops.spectral_gains(D, self.long_diffusion_dist, self.num_layer, plan_mlp)  # [L,B,S,K]
        Lc = L.permute(0, 3, 1, 2)                                   # channel-major view
        if gemm_dtype is not None:
            Lc = Lc.to(gemm_dtype)
        Lc = Lc.contiguous()
        Vf = V.float()
        Vt = Vf.transpose(1, 2).contiguous()
        state = node_feat.float() if self.general else self.embedding(node_feat)
        for t in range(self.num_layer):
            W, bias = self._mix_weight(t), self.filter[t].bias
            d_in = state.shape[2]
            Wc = W.view(W.shape[0], -1, d_in)
            out = bias.view(1, 1, -1).expand(B, N, -1).clone()
            c = 0
            for p in self.short_diffusion_dist:
                z = torch.matmul(state, Wc[:, c].t())
                for _ in range(p):
                    z = torch.bmm(Lc[:, 0].float(), z)
                out += z
                c += 1
            if S > 0:
                # sum_s V diag(g_s) V^T X W_s^T = V [ sum_s (g_s * (V^T X)) W_s^T ]: project X to the
                # K eigen directions ONCE, mix the S channels there (K rows instead of N), lift
                # back once — 13x fewer FLOPs than S full-size GEMM chains at N = 2048, K = 64
                Y = torch.bmm(Vt, state)                              # V^T X        [B,K,d_in]
                Gt = G[t].transpose(1, 2)                             # [B,K,S]
                Ys = (Gt.unsqueeze(3) * Y.unsqueeze(2)).reshape(B, Y.shape[1], S * d_in)
                Wl = Wc[:, c:c + S].reshape(W.shape[0], S * d_in)     # [dout, S*d_in]
                out += torch.bmm(Vf, torch.matmul(Ys, Wl.t()))        # V T          [B,N,dout]
                c += S
            E1 = self.num_edgetype + 1
            dout = W.shape[0]
            # X W_e^T for all edge types in one GEMM, then one N x N batched GEMM per type
            Z = torch.matmul(state, Wc[:, c:c + E1].permute(1, 0, 2).reshape(E1 * dout, d_in).t())
            Z = Z.view(B, N, E1, dout)
            for e in range(E1):
                z = Z[:, :, e]
                if gemm_dtype is not None:
                    out += torch.bmm(Lc[:, e], z.to(gemm_dtype)).float()
                else:
                    out = torch.baddbmm(out, Lc[:, e], z)
            c += E1
            state = torch.relu_(out)
        y = self.filter[-1](state) * self.att_func(state)
        m = (mask != 0).float().unsqueeze(2)
        return (y * m).sum(dim=1) / m.sum(dim=1)

    @torch.no_grad()
    def _plan_large(self, planes=None, classes=None):
        """classes: the channel fold of `_large_fold_classes` (tuple: channel -> representative
        channel); the node-space weight blocks of a class are summed (sum_c L_c X W_c^T =
        L (X (sum_c W_c)^T) for equal operators) and only the representatives are kept."""
        sig = self._param_signature()
        cache = getattr(self, '_plan_large_cache', None)
        if cache is None or cache['sig'] != sig:
            buf = None
            if self._has_mlp() and self.num_scale_long <= self.gains_kernel_max_scales:
                buf = ops.pack_spectral_mlp_layers(
                    [[(seq[i].weight, seq[i].bias) for i in (0, 2, 4, 6)]
                     for seq in self.spectral_filter], self.num_scale_long)
            cache = self._plan_large_cache = dict(sig=sig, mlp_pack=buf, conv={})
        key = planes if classes is None else (planes, tuple(classes))
        if planes is not None and key not in cache['conv']:
            # per layer: the node-space (edge-type) column blocks of the mix weight as bf16 pieces
            # in MFMA fragment order (the Wf of lnz_large_gemm1) and the long-scale blocks
            # as their pack_rows_k8 image, fp32 (lnz_large_spectral)
            S, E1 = self.num_scale_long, self.num_edgetype + 1
            if classes is None:
                classes = tuple(range(E1))
            assert len(classes) == E1
            reps = sorted(set(classes))
            layers = []
            for t in range(self.num_layer):
                W = self._mix_weight(t).detach().float()
                dout = W.shape[0]
                d_in = W.shape[1] // (S + E1)
                dinp = (d_in + 15) // 16 * 16
                Wc = torch.nn.functional.pad(W.view(dout, S + E1, d_in), (0, dinp - d_in))
                Wn = Wc[:, S:]
                if len(reps) < E1:
                    Wn = torch.stack([sum(Wn[:, c] for c in range(E1) if classes[c] == r)
                                      for r in reps], dim=1)
                Wb = ops.large_weight_fragments(ops.split_bf16_planes(
                    Wn.permute(1, 0, 2).reshape(len(reps) * dout, dinp), planes))
                Wt = ops.pack_rows_k8(Wc[:, :S].reshape(dout, S * dinp).contiguous()) if S else None
                # one operator class: its summed fp32 block, columns padded to a multiple of 32
                # (lnz_f32_linear's K) — the exact-fp32 sparse form of the split-precision modes
                d32 = (d_in + 31) // 32 * 32
                Wn32 = torch.nn.functional.pad(Wn[:, 0, :d_in], (0, d32 - d_in)).contiguous() \
                    if len(reps) == 1 else None
                layers.append(dict(Wb=Wb, Wt=Wt, bias=self.filter[t].bias.detach().float().contiguous(),
                                   din=d_in, Wn32=Wn32))
            cache['conv'][key] = layers
        return cache

    # -- graphs of 33..128 nodes: one fused launch (csrc/conv_mid.hip) ---------------------------
    mid_graph_kernel = os.environ.get('LANCZOSNET_MID_KERNEL', '1') != '0'

    def _mid_hip_supported(self, N, K, channels):
        """lnz_midgraph_forward: exact fp32, uniform hidden width 128, input width <= 128, no
        short-diffusion powers, K <= 32, <= 16 long scales, <= 2 operator channels, 32 < N <= 128."""
        return (self.mid_graph_kernel and 32 < N <= 128 and K <= 32 and channels <= 2
                and self.gemm_mode == 'fp32' and self.filter_kind == 0
                and set(self.hidden_dim[:self.num_layer]) == {128} and self.input_dim <= 128
                and self.num_scale_short == 0 and self.num_scale_long <= 16 and self.output_dim <= 31
                and self._channel_order() is None)

    @torch.no_grad()
    def _plan_mid(self):
        """Weights of lnz_midgraph_forward: per layer the mix weight as [128][S + E + 1][dinp]
        (input width zero-padded to a multiple of 16), biases, head + gate rows."""
        cache = self._plan_large()
        if 'mid' not in cache:
            S, E1 = self.num_scale_long, self.num_edgetype + 1
            Ws, din0p = [], None
            for t in range(self.num_layer):
                W = self._mix_weight(t).detach().float()
                d_in = W.shape[1] // (S + E1)
                dinp = (d_in + 15) // 16 * 16
                if t == 0:
                    din0p = dinp
                Ws.append(torch.nn.functional.pad(W.view(W.shape[0], S + E1, d_in),
                                                  (0, dinp - d_in)).reshape(-1))
            cache['mid'] = dict(
                W=torch.cat(Ws).contiguous(), din0p=din0p,
                bias=torch.stack([self.filter[t].bias.detach().float() for t in range(self.num_layer)]).contiguous(),
                Whead=torch.cat([self.filter[-1].weight.detach().float(),
                                 self.att_func[0].weight.detach().float()]).contiguous(),
                bhead=torch.cat([self.filter[-1].bias.detach().float(),
                                 self.att_func[0].bias.detach().float()]).contiguous())
        return cache

    @torch.no_grad()
    def _mid_graph_forward_hip(self, node_feat, L, D, V, mask):
        plan = self._plan_mid()
        mid = plan['mid']
        X0 = node_feat.float() if self.general else self.embedding(node_feat).float()
        if X0.shape[2] != mid['din0p']:
            X0 = torch.nn.functional.pad(X0, (0, mid['din0p'] - X0.shape[2]))
        G = None
        if self.num_scale_long > 0:
            G = ops.spectral_gains(D, self.long_diffusion_dist, self.num_layer, plan['mlp_pack'])
        Lf = L if L.dtype == torch.float32 else L.float()
        return ops.midgraph_forward(X0.contiguous(), Lf, V.float().contiguous(), G,
                                    mask.to(torch.uint8).contiguous(), mid['W'], mid['bias'], mid['Whead'],
                                    mid['bhead'], self.num_layer)

    def _mid_backward_supported(self, N, K, channels):
        """The HIP backward of lnz_midgraph_forward (lnz_midgraph_head_grad / _input_grad / _project):
        the envelope of `_mid_hip_supported`, selected by `mid_backward_impl == 'hip'` where
        `backward_impl` asks for HIP at all."""
        return (self.mid_backward_impl == 'hip' and self.backward_impl == 'hip'
                and self._mid_hip_supported(N, K, channels))

    @torch.no_grad()
    def _plan_mid_backward(self):
        """`_plan_mid` + the transposed weight blocks of lnz_midgraph_input_grad: per layer
        Wt[i][c][o] = W[o][c][i] as [128][S + E + 1][128] (layer 0: rows beyond its input width zero)."""
        cache = self._plan_mid()
        mid = cache['mid']
        if 'Wt' not in mid:
            nch = self.num_scale_long + self.num_edgetype + 1
            Wts = []
            for t in range(self.num_layer):
                W = self._mix_weight(t).detach().float()
                Wt = W.view(128, nch, -1).permute(2, 1, 0)
                Wts.append(torch.nn.functional.pad(Wt, (0, 0, 0, 0, 0, 128 - Wt.shape[0])).reshape(-1))
            mid['Wt'] = torch.cat(Wts).contiguous()
        return cache

    def _large_hip_supported(self, K, channels=1):
        """lnz_large_*: uniform hidden width 128, input width <= 128, no short-diffusion powers,
        K <= 64, <= 16 long scales, at most 8 operator channels (the pack kernel's channel map,
        csrc/conv_large.hip: `LargeChanMap`; more edge types take the library path like any other
        unsupported shape)."""
        return (set(self.hidden_dim[:self.num_layer]) == {128} and self.input_dim <= 128
                and self.num_scale_short == 0 and K <= 64 and channels <= 8
                and self.num_scale_long <= self.gains_kernel_max_scales)

    # -- channel folding of the large-graph path ------------------------------------------------
    # With one edge type (config/graph_lanczos_net.yaml:14) the collated L carries the SAME operator
    # twice: channel 0 = L4 of the simple graph, channel 1 = L4 of the only bond type (reference
    # dataset/graph_data.py:225-262).  The conv is HBM bound on the operator stream, so streaming the
    # duplicate is half of its bytes for nothing.  Equality is a property of the DATA, and the check
    # is free where every entry of every channel is in registers anyway — the pack kernel:
    #   * a zero channel stride (an expanded view) proves equality without looking;
    #   * otherwise the pack kernel compares the packed channels pairwise while it converts them
    #     and reports "differs somewhere" bits; the bits come back through pinned memory and are
    #     read at the NEXT call (never a host sync): channels that were equal in the last batch are
    #     folded in this one — the claim is then verified by the same compare, and the only wait is
    #     for the pack launch itself while the layer launches behind it keep the GPU busy; a
    #     failed claim repacks unfolded (and drops the guess).
    # `large_fold = False` (or LANCZOSNET_LARGE_FOLD=0) packs every channel, no comparison.
    large_fold = os.environ.get('LANCZOSNET_LARGE_FOLD', '1') != '0'

    def _large_fold_classes(self, L):
        """-> (classes, proven): classes[c] = representative channel of channel c under the
        current claim; proven[c] = True when channel c needs no verification (its own
        representative, or structurally equal through a zero channel stride)."""
        Cn = L.shape[3]
        ident = tuple(range(Cn))
        if not self.large_fold or Cn == 1 or Cn > 8:
            return ident, (True,) * Cn
        if L.stride(3) == 0:
            return (0,) * Cn, (True,) * Cn
        st = self.__dict__.setdefault('_large_fold_state', {}).get((Cn, L.device.index))
        if st is None:
            return ident, (True,) * Cn
        if st.get('pending') is not None:
            ev, host, cls = st.pop('pending')
            st['pending'] = None
            ev.synchronize()   # the previous call's pack: long finished
            st['guess'] = self._classes_from_bits(int(host.item()), cls)
        guess = st.get('guess', ident)
        return guess, tuple(guess[c] == c for c in range(Cn))

    @staticmethod
    def _classes_from_bits(bits, packed_classes):
        """Refine the classes a pack ran with by its comparison bits: packed channels (the
        representatives) that never differed from an earlier packed channel join its class."""
        Cn = len(packed_classes)
        reps = sorted(set(packed_classes))
        new_rep = {}
        for r in reps:
            new_rep[r] = r
            for r2 in reps:
                if r2 >= r:
                    break
                if new_rep[r2] == r2 and not (bits >> (8 * r + r2)) & 1:
                    new_rep[r] = r2
                    break
        return tuple(new_rep[packed_classes[c]] for c in range(Cn))

    def _large_pack(self, Lf, Vf, planes):
        """Pack the operators under the current fold claim.  -> (Lb, Vb, classes, verify) where
        verify() (or None) must be called before the result is released: it waits for the pack
        launch and returns False when a folded channel turned out to differ."""
        Cn = Lf.shape[3]
        classes, proven = self._large_fold_classes(Lf)
        capturing = torch.cuda.is_current_stream_capturing()
        compare = self.large_fold and 1 < Cn <= 8 and not capturing and Lf.stride(3) != 0
        if capturing and not all(proven):
            classes, proven = tuple(range(Cn)), (True,) * Cn
        reps = sorted(set(classes))
        if not compare and len(reps) == Cn:
            Lb, Vb = ops.large_pack_operators(Lf, Vf, planes)
            return Lb, Vb, classes, None
        slot = {r: i for i, r in enumerate(reps)}
        neq = torch.zeros((1,), dtype=torch.int64, device=Lf.device) if compare else None
        Lb, Vb = ops.large_pack_operators(
            Lf, Vf, planes, chan_src=reps, chan_rep=[slot[classes[c]] for c in range(Cn)],
            chan_check=[0 if (classes[c] != c and proven[c]) else 1 for c in range(Cn)], neq=neq)
        if not compare:
            return Lb, Vb, classes, None
        # keyed per device: nn.DataParallel replicas are shallow copies that share this dict, and
        # each of them runs on a device (and thread) of its own
        st = self.__dict__.setdefault('_large_fold_state', {}).setdefault((Cn, Lf.device.index), {})
        host = st.get('host')
        if host is None:
            host = st['host'] = torch.zeros((1,), dtype=torch.int64).pin_memory()
        host.copy_(neq, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        claimed = [c for c in range(Cn) if classes[c] != c and not proven[c]]
        if not claimed:
            st['pending'] = (ev, host, classes)   # read at the next call
            return Lb, Vb, classes, None
        st['pending'] = None

        def verify():
            ev.synchronize()
            bits = int(host.item())
            ok = not any((bits >> (8 * c + classes[c])) & 1 for c in claimed)
            if ok:
                st['guess'] = self._classes_from_bits(bits, classes)
            else:
                st['guess'] = tuple(range(Cn))
            return ok
        return Lb, Vb, classes, verify

    # -- the node-space term on the nonzeros of L (csrc/conv_sparse.hip) -------------------------
    # The image kernel reads L once, keeps the nonzeros of channel 0
    # and reports (a) whether any other channel differs from channel 0 (the fold claim of
    # `_large_pack`, checked here for all channels at once) and (b) whether a row is too dense for
    # the gather to beat the stream (when the batch comes from `collate_graph_adjacency`, its K-step
    # Lanczos pass over L has left that image riding on the tensor: L is read once per batch).
    # The flags come back through pinned memory behind the layer
    # launches; a raised flag discards the result, the batch takes the streamed kernels, and the
    # next `large_sparse_backoff` calls on this device do not try again (twice as many after every
    # further failure in a row, up to 32 x).
    large_sparse = os.environ.get('LANCZOSNET_LARGE_SPARSE', '1') != '0'
    large_head_kernel = os.environ.get('LANCZOSNET_LARGE_HEAD', '1') != '0'
    large_sparse_backoff = 32

    def _large_sparse_layers(self, node_feat, Lf, Vf, G, planes=1):
        """-> the last conv layer's state [B,N,128], or None when the batch has to take the
        streamed kernels (disabled, capturing, N beyond 16-bit columns, or a raised image flag).
        planes = 1: bf16 values x bf16 features (the streamed bf16 form's products); planes = 2, 3
        (the split-precision modes): the node-space term in EXACT fp32 — fp32 values x fp32
        features of lnz_f32_linear — and the lift from `planes` pieces as in the streamed form."""
        B, N, _, Cn = Lf.shape
        if not self.large_sparse or N > 65536 or torch.cuda.is_current_stream_capturing():
            return None
        st = self.__dict__.setdefault('_large_sparse_state', {}).setdefault(Lf.device.index, {})
        if st.get('skip', 0) > 0:
            st['skip'] -= 1
            return None
        exact = planes != 1
        img = ops.attached_sparse_image(Lf)   # left by the collate's Lanczos pass over this very tensor
        if img is not None and exact and img.values is None:
            img = None                        # (an image without the unrounded values)
        st['image_from'] = 'collate' if img is not None else 'forward'
        if img is None:
            img = ops.large_sparse_image(Lf, values=exact)
        host = st.get('host')
        if host is None:
            host = st['host'] = torch.zeros((1,), dtype=torch.int32).pin_memory()
        host.copy_(img.flags, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        Vb = ops.large_pack_vectors(Vf, planes)
        classes = (0,) * Cn
        plan = self._plan_large(planes, classes)
        state = node_feat.float().contiguous() if self.general else \
            self.embedding(node_feat).float().contiguous()
        bufs = [None, None]
        if not exact:
            work = ops.large_sparse_work_buffers(B, N, Lf.device)
            for t, lay in enumerate(plan['conv'][(1, classes)]):
                state = ops.large_sparse_conv_layer(state, lay['din'], img, Vb, Vf, lay['Wb'], lay['Wt'],
                                                    G[t] if G is not None else None, lay['bias'], work,
                                                    relu=True, out=bufs[t & 1])
                bufs[t & 1] = state
        else:
            dev = Lf.device
            work = (torch.empty((B, N, 128), dtype=torch.float32, device=dev),
                    torch.zeros((planes, B, 128, 64), dtype=ops.large_plane_dtype(planes), device=dev),
                    torch.zeros((B, 64, 128), dtype=torch.float32, device=dev))
            d0 = state.shape[2]
            if d0 % 32:
                state = torch.nn.functional.pad(state, (0, (d0 + 31) // 32 * 32 - d0)).contiguous()
            for t, lay in enumerate(plan['conv'][(planes, classes)]):
                state = ops.large_sparse_conv_layer_f32(state, lay['din'], img, Vb, Vf, lay['Wn32'], lay['Wt'],
                                                        G[t] if G is not None else None, lay['bias'], work,
                                                        planes, relu=True, out=bufs[t & 1])
                bufs[t & 1] = state
        ev.synchronize()   # the image launch: long finished
        flags = int(host.item())
        st['last_flags'] = flags
        if flags:
            # (a data set of dense graphs raises it every time: the pause doubles, up to 32 x)
            st['streak'] = min(st.get('streak', 0) + 1, 6)
            st['skip'] = self.large_sparse_backoff << (st['streak'] - 1)
            return None
        st['streak'] = 0
        return state

    @torch.no_grad()
    def _large_graph_forward_hip(self, node_feat, L, D, V, mask, planes=3):
        """Graphs beyond the 32-node MFMA tile on the hand-written streaming kernels
        (csrc/conv_large.hip; BASELINE config 5: N = 2048, K = 64, batch 256): the operators are
        packed once (channel-major bf16 planes, equal channels once — see `_large_pack`), every
        layer is gemm1 + eigen-space spectral block + streamed conv.  planes = 3: fp32-grade split
        products (default, the 1e-5 parity mode); planes = 1: plain bf16 operands / fp32
        accumulate (`gemm_mode = 'bf16'`, config 5's mode)."""
        S = self.num_scale_long
        Lf = L if L.dtype == torch.float32 else L.float()
        Vf = V.float().contiguous()
        G = None
        if S > 0:
            G = ops.spectral_gains(D, self.long_diffusion_dist, self.num_layer,
                                   self._plan_large()['mlp_pack'])
        state = self._large_sparse_layers(node_feat, Lf, Vf, G, planes)
        for attempt in range(2 if state is None else 0):
            Lb, Vb, classes, verify = self._large_pack(Lf, Vf, planes)
            plan = self._plan_large(planes, classes)
            work = ops.large_work_buffers(Lb)
            state = node_feat.float().contiguous() if self.general else \
                self.embedding(node_feat).float().contiguous()
            bufs = [None, None]
            for t, lay in enumerate(plan['conv'][(planes, tuple(classes))]):
                state = ops.large_conv_layer(state, lay['din'], Lb, Vb, Vf, lay['Wb'], lay['Wt'],
                                             G[t] if G is not None else None, lay['bias'], work,
                                             relu=True, out=bufs[t & 1])
                bufs[t & 1] = state
            if verify is None or verify():
                break
            # a folded channel differed in this batch: the guess is dropped, pack every channel
        if self.large_head_kernel and self.output_dim <= 16 and state.shape[2] == 128:
            # the readout in one pass over the state (csrc/head_large.hip)
            Wh = torch.cat([self.filter[-1].weight.detach().float(), self.att_func[0].weight.detach().float()])
            bh = torch.cat([self.filter[-1].bias.detach().float(), self.att_func[0].bias.detach().float()])
            return ops.large_head(state, mask, Wh, bh)
        y = self.filter[-1](state) * self.att_func(state)
        m = (mask != 0).float().unsqueeze(2)
        return (y * m).sum(dim=1) / m.sum(dim=1)

    def _tiles16_channels_ok(self):
        """Channel counts of the strip kernels (csrc/conv_strip.hip strip_forward_eligible), the
        only home of the training forward and the input-gradient pass: at most 12 long-diffusion
        channels, at most 32 channels in all."""
        n_long, n_short = len(self.long_diffusion_dist), len(self.short_diffusion_dist)
        return n_long <= 12 and n_short + n_long + self.num_edgetype + 1 <= 32

    def _fused_backward_supported(self):
        """The HIP backward (lnz_lanczosnet_input_grad / _messages) is built for the exact-fp32
        LanczosNet kernel with hidden width 128."""
        return (self.filter_kind == 0 and self.gemm_mode == 'fp32' and self._fused_supported()
                and self.hidden_dim[0] == 128 and self.backward_impl == 'hip'
                and self._tiles16_channels_ok())

    @torch.no_grad()
    def _plan_backward(self):
        """Transposed packs for lnz_lanczosnet_input_grad: kernel layer t = conv layer L-1-t holds
        pack_rows_k8 of Wb[i][c*128 + o] = W_l[o][c*d_l + i]."""
        plan = self._plan()
        if 'Wp_t' in plan:
            return plan
        dev = self.filter[0].weight.device
        n_chan = self.num_scale_short + self.num_scale_long + self.num_edgetype + 1
        dhid, din0, din0p = plan['dhid'], plan['din0_raw'], plan['din0']
        packs, offs, off = [], [], 0
        # kernel layers 0 .. L-2 = conv layers L-1 .. 1 (one shape: packed by one launch), then
        # conv layer 0 with its own width
        if self.num_layer > 1:
            wbs = []
            for t in range(self.num_layer - 1):
                w = self._mix_weight(self.num_layer - 1 - t).detach().float().view(dhid, n_chan, dhid)
                wbs.append(w.permute(2, 1, 0).reshape(dhid, n_chan * dhid))
            pk = ops.pack_rows_k8(torch.cat(wbs, dim=0).contiguous())
            packs.append(pk)
            per = pk.numel() // (self.num_layer - 1)
            for t in range(self.num_layer - 1):
                offs.append(off)
                off += per
        w = self._mix_weight(0).detach().float().view(dhid, n_chan, din0)
        if din0p != din0:
            w = torch.nn.functional.pad(w, (0, din0p - din0))
        wb = w.permute(2, 1, 0).reshape(w.shape[2], n_chan * dhid).contiguous()
        pk = ops.pack_rows_k8(wb)
        packs.append(pk)
        offs.append(off)
        off += pk.numel()
        plan['Wp_t'] = torch.cat(packs + [torch.zeros(2048, dtype=torch.float32, device=dev)])
        plan['wt_off'] = offs
        return plan

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
        state = node_feat.float() if self.general else self.embedding(node_feat)
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
        y = self.filter[-1](state)
        att = self.att_func(state)
        y = att * y
        m = (mask != 0).float().unsqueeze(2)
        return (y * m).sum(dim=1) / m.sum(dim=1)

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
        fused = self._fused_supported() and self._fused_channels_ok()
        if L.shape[1] > 32 or not fused or drop:
            if L.shape[1] <= 32 and not getattr(self, '_warned_library_path', False):
                warnings.warn('lanczosnet_amd: %s is outside the fused MFMA kernel (uniform width 64 '
                              'or 128, <= 8 short and <= 12 long scales, <= 32 channels in all, no '
                              'training dropout): using the device library-GEMM path '
                              '(hipBLASLt conv + HIP spectral gains; differentiable torch ops when '
                              'gradients or dropout are needed), which is slower'
                              % ('dropout=%r in training' % self.dropout if drop else
                                 'hidden_dim=%r / input_dim=%r' % (self.hidden_dim, self.input_dim)
                                 if not self._fused_supported() else
                                 '%d short + %d long scales + %d operator channels'
                                 % (self.num_scale_short, self.num_scale_long, self.num_edgetype + 1)))
                self._warned_library_path = True
            if (not drop and self._needs_grad()
                    and self._mid_backward_supported(L.shape[1], V.shape[2], L.shape[3])
                    and not torch.cuda.is_current_stream_capturing()):
                # 33..128 nodes, opted in: the one-launch forward keeping its states + its HIP backward
                score = _MidGraphFusedFunction.apply(self, node_feat, L, D, V, mask,
                                                     *[p for p in self.parameters()])
            elif self._needs_grad() or drop:
                # the reference trains arbitrary widths / sizes: differentiate the device-side
                # torch restatement (same association as the kernels)
                score = self._torch_forward(node_feat, L, D, V, mask, dropout=drop)
            elif self._mid_hip_supported(L.shape[1], V.shape[2], L.shape[3]):
                # 33..128 nodes: every layer, the head and the readout in one launch
                score = self._mid_graph_forward_hip(node_feat, L, D, V, mask)
            elif L.shape[1] > 32 and self._large_hip_supported(V.shape[2], L.shape[3]):
                # hand-written streaming kernels; 'bf16' = config 5's bf16-operand mode
                score = self._large_graph_forward_hip(node_feat, L, D, V, mask,
                                                      planes=1 if self.gemm_mode == 'bf16'
                                                      else self.large_split_planes)
            else:
                score = self._large_graph_forward(node_feat, L, D, V, mask)
        elif self._needs_grad():
            # training (runner/qm8_runner.py:216-248): forward = HIP kernels; backward = the HIP
            # input-gradient and message kernels + library GEMMs (_LanczosNetFusedFunction) where
            # built, else autograd through a torch recomputation (_LanczosNetFunction)
            fn = _LanczosNetFusedFunction if self._fused_backward_supported() else _LanczosNetFunction
            score = fn.apply(self, node_feat, L, D, V, mask, *[p for p in self.parameters()])
        else:
            score = self._hip_forward(node_feat, L, D, V, mask)
        if label is not None:
            return score, self.loss_func(score, label)
        return score


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
            mlp_params = [m.spectral_filter[t][i].weight for i in lin_idx for t in range(Lnum)] + \
                         [m.spectral_filter[t][i].bias for i in lin_idx for t in range(Lnum)]
            gg = torch.autograd.grad(h, mlp_params, dG)
        for p_, g_ in zip(mlp_params, gg):
            grads[id(p_)] = g_


def _fused_conv_backward(m, plan, grad_score, node_feat, V, G, mask_u8, Lp, act, tiles, n_mol,
                         static_rows, rtot, rtot_ready):
    """The part of the HIP backward LanczosNet and AdaLanczosNet share: readout head by torch
    autograd on the stored last state, node-state gradients of the conv stack
    (lnz_lanczosnet_input_grad), conv weight / bias gradients (lnz_lanczosnet_messages + one
    library GEMM per layer).  V, G: the basis and the filters the forward ran with (Ritz vectors +
    diagonal gains, or Lanczos vectors + dense K x K filters).  Returns (grads by id(parameter),
    dy [L,B,32,dh] pre-activation gradients, dx0 [B,32,din0p], x0 [B,32,din0p])."""
    B, N, K = V.shape
    Lnum, dh = m.num_layer, plan['dhid']
    din0, din0p = plan['din0_raw'], plan['din0']
    S, n_short = m.num_scale_long, m.num_scale_short
    n_chan = n_short + S + m.num_edgetype + 1
    dev = V.device
    grads = {}
    # ---- head (model/lanczos_net.py:185-194) on the stored last state: lnz_head_backward (one
    #      launch; below, once the compact row numbering exists) or torch autograd
    P_out = m.filter[-1].weight.shape[0]
    hip_head = (m.head_grad_impl == 'hip' and dh == 128 and N <= 32 and P_out <= 31 and
                mask_u8.shape[1] == N)
    head_params = list(m.filter[-1].parameters()) + list(m.att_func.parameters())
    hg = None
    with torch.enable_grad():
        if not hip_head:
            XL = act[Lnum - 1][:, :N].detach().requires_grad_(True)
            # output Linear and gate Linear as ONE product (three library GEMMs forward + backward instead
            # of six thin ones; every output column is the same dot product either way)
            Z = torch.nn.functional.linear(XL, torch.cat([m.filter[-1].weight, m.att_func[0].weight], dim=0),
                                           torch.cat([m.filter[-1].bias, m.att_func[0].bias], dim=0))
            y = Z[..., :P_out] * torch.sigmoid(Z[..., P_out:])
            mk = (mask_u8 != 0).float().unsqueeze(2)
            score = (y * mk).sum(dim=1) / mk.sum(dim=1)
            hg = torch.autograd.grad(score, [XL] + head_params, grad_score.contiguous())
    dy = torch.zeros((Lnum, B, 32, dh), dtype=torch.float32, device=dev)
    if hg is not None:
        for p_, g_ in zip(head_params, hg[1:]):
            grads[id(p_)] = g_
        dy[Lnum - 1][:, :N] = hg[0] * (XL > 0).float()
    dx0 = torch.zeros((B, 32, din0p), dtype=torch.float32, device=dev)

    # ---- compact row numbering (real nodes only: half of the padded rows are empty) — the row
    #      order of the message matrix; node extent (last real node + 1) is what the kernels size
    #      a molecule by
    # (n_mol: the block lnz_node_extents wrote in the forward — extents | row offsets | total)
    n_mol, row_off, row_total = n_mol[:B], n_mol[B:2 * B], n_mol[2 * B:]
    if static_rows:
        R_tot = B * N   # graph capture: no host round trip; rows past the real count are masked
    else:
        rtot_ready.synchronize()   # recorded before the forward kernel: long complete
        R_tot = int(rtot[0])
    # ---- node-state gradients of the conv stack.  The kernel also leaves what the weight / bias
    #      gradients need: dY_l in the compact numbering (no gather per layer) and per-workgroup
    #      column sums of dY_l (no reduction over the [L, B * 32, dh] block)
    # (graph capture: rows past the real count are never written — zeros, they meet zero messages)
    dyc = (torch.zeros if static_rows else torch.empty)((Lnum, R_tot, dh), dtype=torch.float32,
                                                        device=dev)
    # (one entry per strip when the plan carries strips: the pass then runs on them)
    strips_ = getattr(tiles[0], 'strips', None)
    n_part = max(2 * tiles[1], (strips_.numel() - 1) // ops.STRIP_INTS if strips_ is not None else 0)
    dbp = torch.zeros((n_part, Lnum, dh), dtype=torch.float32, device=dev)
    db_last = None
    if hip_head:
        dWh, dbh, db_last = ops.head_backward(act[Lnum - 1], mask_u8, grad_score, m.filter[-1].weight.detach(),
                                              m.filter[-1].bias.detach(), N, dy[Lnum - 1], row_off=row_off,
                                              dY_compact=dyc[Lnum - 1], Wgate=m.att_func[0].weight.detach(),
                                              bgate=m.att_func[0].bias.detach())
        grads[id(m.filter[-1].weight)], grads[id(m.filter[-1].bias)] = dWh[:P_out], dbh[:P_out]
        grads[id(m.att_func[0].weight)], grads[id(m.att_func[0].bias)] = dWh[P_out:], dbh[P_out:]
    ops.lanczosnet_input_grad(plan, Lp, V, G, mask_u8, act, dy, dx0, tiles, row_off=row_off,
                              dy_compact=dyc, dbias_part=dbp)

    # ---- X_0
    x0 = torch.zeros((B, 32, din0p), dtype=torch.float32, device=dev)
    if m.general:
        x0[:, :N, :din0] = node_feat.float()
    else:
        x0[:, :N, :din0] = m.embedding.weight.detach()[node_feat]

    # ---- conv weights / biases: dW_l = dY_l^T cat_c(M_c X_l), db_l = column sums of dY_l, over
    #      the REAL node rows only
    if static_rows:
        # rows past the real count are never written by the kernels: zero-filled here
        msg_buf = torch.zeros((R_tot * n_chan * dh,), dtype=torch.float32, device=dev)
        msg_buf0 = msg_buf if din0p == dh else \
            torch.zeros((R_tot * n_chan * din0p,), dtype=torch.float32, device=dev)
    else:
        msg_buf = msg_buf0 = torch.empty((R_tot * n_chan * dh,), dtype=torch.float32, device=dev)
    if not hip_head:
        # the incoming gradient (slot L - 1) is the one layer the input-gradient kernel does not write
        # compactly (lnz_head_backward does): compact row r -> padded row (molecule * 32 + node),
        # without a data-dependent shape; under graph capture the rows past the real count are masked
        r = torch.arange(R_tot, device=dev)
        if static_rows:
            row_end = row_off + n_mol
            valid = (r < row_total).to(torch.float32).unsqueeze(1)
            mol_of_r = torch.searchsorted(row_end, r, right=True).clamp_(max=B - 1)
            real = mol_of_r * 32 + (r - row_off[mol_of_r]).clamp_(min=0, max=31)
            dyc[Lnum - 1] = dy[Lnum - 1].view(B * 32, dh).index_select(0, real) * valid
        else:
            mol_of_r = torch.searchsorted(row_off + n_mol, r, right=True)
            real = mol_of_r * 32 + (r - row_off[mol_of_r])
            dyc[Lnum - 1] = dy[Lnum - 1].view(B * 32, dh).index_select(0, real)
    for la in range(Lnum):
        d = din0p if la == 0 else dh
        msg = (msg_buf0 if la == 0 else msg_buf)[:R_tot * n_chan * d].view(R_tot, n_chan * d)
        ops.lanczosnet_messages(plan, Lp, V, G, mask_u8, act, x0, la, msg, tiles,
                                row_off=row_off)
        dW = _tn_split_k(dyc[la], msg)
        if la == 0 and din0p != din0:
            dW = dW.view(dh, n_chan, din0p)[:, :, :din0].reshape(dh, n_chan * din0)
        grads[id(m.filter[la].weight)] = m._to_reference_channel_order(dW)
    # bias gradients: the kernel's per-workgroup column sums added in a fixed order (one small
    # reduction over [2 * workgroups, L, dh] instead of one over the [L, B * 32, dh] block);
    # the last layer's from the incoming gradient
    db_all = dbp.sum(dim=0)
    db_all[Lnum - 1] = db_last if db_last is not None else dy[Lnum - 1].view(B * 32, dh).sum(dim=0)
    for la in range(Lnum):
        grads[id(m.filter[la].bias)] = db_all[la]
    return grads, dy, dx0, x0


class _LanczosNetFusedFunction(torch.autograd.Function):
    """Training through the HIP kernels.

    forward: the fused kernel, storing every layer's activations.
    backward: head by torch autograd on the stored last state; node-state gradients of the whole
    conv stack by lnz_lanczosnet_input_grad (the forward's two chained GEMMs run on dY with
    transposed weights); per layer the reference's message matrix by lnz_lanczosnet_messages and
    dW = dY^T msg as one library GEMM; spectral-MLP gradients from dG[b,k,s] =
    sum_i ((V^T dY) W_s)[b,k,i] (V^T X)[b,k,i] and torch autograd through the small MLP; embedding
    rows by index_add.  Inputs L, D, V, mask, node ids are data: no gradient."""

    @staticmethod
    def forward(ctx, module, node_feat, L, D, V, mask, *params):
        plan = module._plan()
        mask_u8 = mask.to(torch.uint8).contiguous()
        Vc = V.float().contiguous()
        B = Vc.shape[0]
        Lp, tiles, rows = ops.pack_and_plan(plan, L, mask_u8, Vc.shape[2])
        G = None
        if module.num_scale_long > 0:
            G = ops.spectral_gains(D, module.long_diffusion_dist, module.num_layer, plan['mlp_pack'],
                                   rows=rows)
        act = torch.zeros((module.num_layer, B, 32, plan['dhid']), dtype=torch.float32,
                          device=Vc.device)
        # node extents and their total: the backward sizes its compact message matrix by the
        # number of real node rows.  The count travels to the host asynchronously, under the
        # forward kernel, so the backward never has to drain the GPU to learn a shape.
        N = Vc.shape[1]
        # (one launch: extents, their exclusive prefix sums = the compact row numbering, the total)
        n_mol = ops.node_extents_block(mask_u8)
        # Under HIP-graph capture (train.GraphedTrainStep) nothing may touch the host: the backward
        # then sizes its message matrix by the padded row count B * N and masks the tail on the
        # device instead of reading the real row count.
        ctx.static_rows = (torch.cuda.is_current_stream_capturing()
                           or bool(getattr(module, 'train_static_rows', False)))
        rtot = ev = None
        if not ctx.static_rows:
            rtot = torch.empty((1,), dtype=torch.int64, pin_memory=True)
            rtot.copy_(n_mol[-1:], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        score = ops.lanczosnet_forward(plan, node_feat, Lp, Vc, G, mask_u8, tiling=tiles,
                                       act_out=act)
        ctx.module, ctx.cap = module, tiles[1]
        ctx.rtot, ctx.rtot_ready = rtot, ev
        # the live eigen rows (b * K + k, k < min(n_b, K)) the gains were evaluated on: the backward
        # runs the MLPs on those rows only
        live = rows if rows is not None else (None, None)
        ctx.has_rows = live[0] is not None
        ctx.save_for_backward(node_feat, D, Vc, mask_u8, Lp, G, act, tiles[0], n_mol,
                              *([live[0], live[1]] if ctx.has_rows else []))
        return score

    @staticmethod
    def backward(ctx, grad_score):
        m = ctx.module
        node_feat, D, V, mask_u8, Lp, G, act, tile_buf, n_mol = ctx.saved_tensors[:9]
        live_rows, n_live = ctx.saved_tensors[9:11] if ctx.has_rows else (None, None)
        tiles = (tile_buf, ctx.cap)
        plan = m._plan_backward()
        B, N, K = V.shape
        Lnum, dh = m.num_layer, plan['dhid']
        din0, din0p = plan['din0_raw'], plan['din0']
        S, n_short = m.num_scale_long, m.num_scale_short
        n_chan = n_short + S + m.num_edgetype + 1
        dev = V.device
        grads, dy, dx0, x0 = _fused_conv_backward(m, plan, grad_score, node_feat, V, G, mask_u8, Lp,
                                                  act, tiles, n_mol, ctx.static_rows, ctx.rtot,
                                                  ctx.rtot_ready)

        # ---- spectral filter MLPs (model/lanczos_net.py:95-123): dG, then autograd through the MLPs.
        #      All layers at once: one batched V^T [dY_0..dY_L-1 | X_0..X_L-1], one batched MLP.
        if S > 0 and m._has_mlp() and os.environ.get('LANCZOSNET_DGAINS', 'hip') == 'hip':
            # dG[l][b][k][s] = sum_o (V^T dY_l)[k][o] ((V^T X_l) W_{l,s}^T)[k][o]: one HIP launch in
            # the forward's tile structure (lnz_lanczosnet_gain_grad)
            dG = ops.lanczosnet_gain_grad(plan, Lp, V, G, mask_u8, act, x0, dy, tiles)
            dG = dG.view(Lnum, B * K, S)
        elif S > 0 and m._has_mlp():
            Vt = V.transpose(1, 2)
            cat = torch.cat([dy[:, :, :N].permute(1, 2, 0, 3).reshape(B, N, Lnum * dh),
                             x0[:, :N],
                             act[:Lnum - 1, :, :N].permute(1, 2, 0, 3).reshape(B, N, (Lnum - 1) * dh)],
                            dim=2)
            proj = torch.bmm(Vt, cat)                                   # [B,K,L*dh + din0p + (L-1)*dh]
            dYv = proj[:, :, :Lnum * dh].reshape(B * K, Lnum, dh)
            dG = []
            for la in range(Lnum):
                d = din0 if la == 0 else dh
                lo = Lnum * dh if la == 0 else Lnum * dh + din0p + (la - 1) * dh
                Xv = proj[:, :, lo:lo + d]                              # [B,K,d]
                Wl = m._mix_weight(la).detach().view(dh, n_chan, d)[:, n_short:n_short + S, :]
                R = torch.matmul(dYv[:, la], Wl.reshape(dh, S * d)).view(B, K, S, d)
                dG.append((R * Xv.unsqueeze(2)).sum(dim=3))             # [B,K,S]
            dG = torch.stack(dG).reshape(Lnum, B * K, S)               # [L, B*K, S]
        if S > 0 and m._has_mlp():
            _spectral_mlp_param_grads(m, grads, D, dG, live_rows, n_live, ctx.static_rows, ctx.rtot)

        # ---- embedding rows: one-hot^T dX_0 as a GEMM (index_add's atomics are 10x slower here)
        if not m.general:
            if din0 in (16, 32, 64, 128):   # (lnz_embedding_grad: rows of dX_0 added by atom id, no atomics)
                grads[id(m.embedding.weight)] = ops.embedding_grad(node_feat.contiguous(), dx0, din0, m.num_atom)
            else:
                onehot = torch.nn.functional.one_hot(node_feat.reshape(-1), m.num_atom).to(torch.float32)
                grads[id(m.embedding.weight)] = onehot.t() @ dx0[:, :N, :din0].reshape(-1, din0)

        out = [grads.get(id(p_)) if p_.requires_grad else None for p_ in m.parameters()]
        return (None, None, None, None, None, None) + tuple(out)


class _MidGraphFusedFunction(torch.autograd.Function):
    """Training graphs of 33..128 nodes through the HIP kernels (config/graph_lanczos_net.yaml under
    runner/graph_runner.py).

    forward: spectral gains + lnz_midgraph_forward, keeping its exchange buffer — every layer's
    output state.
    backward: lnz_midgraph_head_grad (the head on the stored last state), lnz_midgraph_input_grad
    (dOut of every layer, one launch), lnz_midgraph_project (the GEMM operands in eigen space, the
    gain gradients, the bias partials), two batched library GEMMs for all dW, lnz_spectral_mlp_grad,
    lnz_embedding_grad.  Inputs L, D, V, mask, node ids are data: no gradient."""

    @staticmethod
    def forward(ctx, module, node_feat, L, D, V, mask, *params):
        m = module
        plan = m._plan_mid_backward()
        mid = plan['mid']
        X0 = node_feat.float() if m.general else m.embedding.weight.detach()[node_feat].float()
        if X0.shape[2] != mid['din0p']:
            X0 = torch.nn.functional.pad(X0, (0, mid['din0p'] - X0.shape[2]))
        X0 = X0.contiguous()
        G = None
        if m.num_scale_long > 0:
            G = ops.spectral_gains(D, m.long_diffusion_dist, m.num_layer, plan['mlp_pack'])
        Lf = L if L.dtype == torch.float32 else L.float()
        Vc = V.float().contiguous()
        mask_u8 = mask.to(torch.uint8).contiguous()
        score, Xwork = ops.midgraph_forward(X0, Lf, Vc, G, mask_u8, mid['W'], mid['bias'], mid['Whead'],
                                            mid['bhead'], m.num_layer, return_work=True)
        ctx.module = m
        ctx.has_gains = G is not None
        ctx.save_for_backward(node_feat, X0, Lf, D, Vc, mask_u8, Xwork, *([G] if G is not None else []))
        return score

    @staticmethod
    def backward(ctx, grad_score):
        m = ctx.module
        node_feat, X0, L, D, V, mask_u8, Xwork = ctx.saved_tensors[:7]
        G = ctx.saved_tensors[7] if ctx.has_gains else None
        mid = m._plan_mid_backward()['mid']
        Lnum, B, NR, _ = Xwork.shape
        N, K = V.shape[1], V.shape[2]
        S, C = m.num_scale_long, L.shape[3]
        din0, din0p = m.input_dim, mid['din0p']
        grads = {}
        dOut = torch.empty_like(Xwork)
        # ---- head (model/lanczos_net.py:185-194): lnz_midgraph_head_grad, or (the oracle that kernel
        #      is tested against) autograd on the stored last state
        P_out = m.filter[-1].weight.shape[0]
        if m.head_grad_impl == 'hip':
            dWh, dbh = ops.midgraph_head_grad(Xwork, mask_u8, grad_score, mid['Whead'], mid['bhead'], dOut)
        else:
            with torch.enable_grad():
                XL = Xwork[-1][:, :N].detach().requires_grad_(True)
                Wh = mid['Whead'].detach().requires_grad_(True)
                bh = mid['bhead'].detach().requires_grad_(True)
                Z = torch.nn.functional.linear(XL, Wh, bh)
                y = Z[..., :P_out] * torch.sigmoid(Z[..., P_out:])
                mk = (mask_u8 != 0).float().unsqueeze(2)
                dXL, dWh, dbh = torch.autograd.grad((y * mk).sum(dim=1) / mk.sum(dim=1), [XL, Wh, bh],
                                                    grad_score.contiguous())
            dOut[-1].zero_()
            dOut[-1][:, :N] = dXL * (XL > 0).float()
        grads[id(m.filter[-1].weight)], grads[id(m.filter[-1].bias)] = dWh[:P_out], dbh[:P_out]
        grads[id(m.att_func[0].weight)], grads[id(m.att_func[0].bias)] = dWh[P_out:], dbh[P_out:]
        # ---- dOut of every layer; dX_0 for the embedding
        dx0, folded = ops.midgraph_input_grad(dOut, Xwork, L, V, G, mid['Wt'], N, din0p,
                                              want_dx0=not m.general)
        # ---- weights and biases: dW_l = [A_l^T Q_l | dOut_l^T M_l], every layer in one batched GEMM
        #      per operand (fixed summation order); the long scales contract over the B K eigen rows
        want_dg = S > 0 and m._has_mlp()
        A, Q, M, dG, dbp = ops.midgraph_project(dOut, Xwork, X0, L, V, G, mid['W'], want_dgains=want_dg)
        dWe = torch.bmm(dOut.view(Lnum, B * NR, 128).transpose(1, 2), M.view(Lnum, B * NR, C * 128))
        dWe = dWe.view(Lnum, 128, C, 128)
        if C > 1:
            # equal operator channels in every graph (one edge type: dataset/graph_data.py:225-262
            # collates the simple graph's Laplacian twice) have equal messages: one value for all blocks
            dWe = torch.where(folded.min() > 0, dWe[:, :, :1].expand_as(dWe), dWe)
        if S > 0:
            dWl = torch.bmm(A.view(Lnum, B * K, 128).transpose(1, 2), Q.view(Lnum, B * K, S * 128))
            dW = torch.cat([dWl.view(Lnum, 128, S, 128), dWe], dim=2)
        else:
            dW = dWe
        db = dbp.sum(dim=1)
        for la in range(Lnum):
            d = din0 if la == 0 else 128
            grads[id(m.filter[la].weight)] = dW[la, :, :, :d].reshape(128, -1)
            grads[id(m.filter[la].bias)] = db[la]
        # ---- spectral filter MLPs from dG [L, B K, S]
        if want_dg:
            _spectral_mlp_param_grads(m, grads, D, dG.view(Lnum, B * K, S))
        # ---- embedding rows
        if not m.general:
            if din0 in (16, 32, 64, 128):
                grads[id(m.embedding.weight)] = ops.embedding_grad(node_feat.contiguous(), dx0, din0, m.num_atom)
            else:
                onehot = torch.nn.functional.one_hot(node_feat.reshape(-1), m.num_atom).to(torch.float32)
                grads[id(m.embedding.weight)] = onehot.t() @ dx0[:, :N, :din0].reshape(-1, din0)
        out = [grads.get(id(p_)) if p_.requires_grad else None for p_ in m.parameters()]
        return (None, None, None, None, None, None) + tuple(out)


class _LanczosNetFunction(torch.autograd.Function):
    """forward: the fused HIP path.  backward: parameter gradients by autograd through
    `_torch_forward` (inputs L, D, V, mask, node ids are data: no gradient)."""

    @staticmethod
    def forward(ctx, module, node_feat, L, D, V, mask, *params):
        ctx.module = module
        ctx.save_for_backward(node_feat, L, D, V, mask)
        return module._hip_forward(node_feat, L, D, V, mask)

    @staticmethod
    def backward(ctx, grad_score):
        module = ctx.module
        node_feat, L, D, V, mask = ctx.saved_tensors
        params = [p for p in module.parameters()]
        with torch.enable_grad():
            score = module._torch_forward(node_feat, L, D, V, mask)
            need = [p for p in params if p.requires_grad]
            grads = torch.autograd.grad(score, need, grad_score.contiguous(), allow_unused=True)
        it = iter(grads)
        out = [next(it) if p.requires_grad else None for p in params]
        return (None, None, None, None, None, None) + tuple(out)


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


class AdaLanczosNet(_LanczosNetBase):
    """Drop-in for reference `model/ada_lanczos_net.py:12-368`: learned Gaussian-kernel Laplacian
    (:101-137) -> in-model Lanczos layer (:139-247) -> `Q MLP(T^k) Q^T` filters (:250-286) -> the
    same conv / readout.  `forward(node_feat, L, label=None, mask=None)`.

    HIP: Laplacian, Lanczos layer (reference exact incl. the quirks of SURVEY.md F6), T powers,
    filter symmetrisation and the fused conv kernel (dense-filter variant).  The 2000-4096-4096-
    4096-2000 filter MLPs (50 M parameters per layer, M = batch) are plain dense GEMMs and go to
    hipBLASLt through `torch.nn.functional.linear` — on the non-redundant 822 inputs / 1050 outputs
    that the symmetric, banded T^p and the symmetrised output leave (`_ada_filter_plan`).  Like the reference (F7) the re-orthogonalisation
    flag is effectively always on: `hasattr(config, 'use_reorthogonalization')` probes the TOP-LEVEL
    config (:35-38)."""
    filter_kind = 1
    _spectral_hidden = 4096
    # 'fp32_hip' (default since r04): the filter MLPs on the hand-written exact-fp32 Linear
    # lnz_f32_linear (csrc/f32_linear.hip: v_mfma_f32_16x16x4_f32, bias + ReLU fused, copies as
    # buffer_load ... lds, stream-K for the last Linear) — filters bit-identical to the library's,
    # the MLP chain as fast, no vendor GEMM in the step;  'fp32': the same GEMMs in
    # hipBLASLt (kept for A/B runs);  'f16x3' (opt-in): each operand split
    # into two fp16 pieces and hi w_hi + hi w_lo + lo w_hi accumulated in fp32 by the hand-written
    # lnz_f16x3_linear chain (csrc/f16x3_linear.hip; needs |activations| < 6.5e4; parity-tested at
    # the same 1e-5 bar);  'f16x3_lib': the r02 form of the same arithmetic — ONE library fp16 GEMM
    # of three times the depth per Linear, fed by lnz_split_f16x3 (kept for A/B runs)
    filter_gemm_mode = os.environ.get('LANCZOSNET_ADA_FILTER_GEMM', 'fp32_hip')
    # False: evaluate the filter MLPs on the full 2000 inputs / outputs (A/B runs and tests)
    fold_filter_mlp = True

    def _spectral_io(self):
        return self.num_eig_vec * self.num_eig_vec * self.num_scale_long

    def _override_dims(self):
        cfg = self.config
        self.use_reorthogonalization = cfg.model.use_reorthogonalization if hasattr(
            cfg, 'use_reorthogonalization') else True
        self.use_power_iteration_cap = cfg.model.use_power_iteration_cap if hasattr(
            cfg, 'use_power_iteration_cap') else True
        # (re-orthogonalisation off — reachable only through a TOP-LEVEL config attribute, F7 — runs
        # on the device-side restatement: the HIP Lanczos layer is built with it on)
        self.input_dim = self.num_atom  # model/ada_lanczos_net.py:40
        # The reference collects T^ii in ASCENDING ii whatever the order of the list
        # (model/ada_lanczos_net.py:262-270), and a repeated entry gives it fewer T blocks than its
        # first Linear has input columns (a shape error there).  Same here: the list is put in
        # ascending order once; a duplicate is refused.
        ld = [d for d in self.long_diffusion_dist]
        if len(set(ld)) != len(ld):
            raise ValueError('AdaLanczosNet: duplicate entries in long_diffusion_dist %r' % (ld,))
        if any(not isinstance(d, int) for d in ld):
            raise NotImplementedError("AdaLanczosNet: 'inf' diffusion distance is not built")
        self.long_diffusion_dist = sorted(ld)

    def forward(self, node_feat, L, label=None, mask=None):
        if mask is None:
            mask = torch.ones(node_feat.shape[:2], dtype=torch.uint8, device=L.device)
        dev = self._guard_forward(L, mask)
        t = self._to_module_device(dev, node_feat=node_feat, L=L, label=label, mask=mask)
        node_feat, L, label, mask = (t[k] for k in ('node_feat', 'L', 'label', 'mask'))
        B, N = node_feat.shape[0], node_feat.shape[1]
        # the start vector is drawn only when there is a Lanczos layer to run (:308-315)
        q1 = self._draw_q1(B, N, L.device) if self.num_scale_long > 0 else None
        drop = self.training and self.dropout > 0.0
        off = self._off_nominal(L.shape[1], drop)
        if off:
            # every configuration the reference class accepts runs: outside what the fused kernels
            # are built for, on the device-side restatement of the same operator sequence
            if off not in self.__dict__.setdefault('_warned_off_nominal', set()):
                self._warned_off_nominal.add(off)
                warnings.warn('lanczosnet_amd: AdaLanczosNet with %s is outside the HIP kernels (built '
                              'for re-orthogonalisation on, MLP filters over >= 1 long scale, hidden '
                              'width 64 / 128, N <= 32, no training dropout): using the device-side '
                              'torch restatement of model/ada_lanczos_net.py:289-368, which is slower'
                              % off)
            with torch.set_grad_enabled(self._needs_grad()):
                score = self._torch_forward_ada(node_feat, L, mask, q1, dropout=drop)
        elif self._needs_grad():
            # forward = HIP kernels; backward = HIP conv-stack backward + library GEMMs for the
            # filter MLPs + autograd through the fp64 Lanczos layer (_AdaLanczosNetFusedFunction)
            # where built, else autograd through the whole torch restatement
            fn = _AdaLanczosNetFusedFunction if self._fused_backward_supported() else \
                _AdaLanczosNetFunction
            score = fn.apply(self, node_feat, L, mask, q1, *[p for p in self.parameters()])
        else:
            score = self._hip_forward_ada(node_feat, L, mask, q1)
        if label is not None:
            return score, self.loss_func(score, label)
        return score

    def _off_nominal(self, N, drop):
        """'' when the HIP kernels serve this call, else the reasons they do not (one string)."""
        why = []
        if not self.use_reorthogonalization and self.num_scale_long > 0:
            why.append('use_reorthogonalization=False')
        if drop:
            why.append('dropout=%r in training' % self.dropout)
        if self.num_scale_long == 0:
            why.append('no long-diffusion scales')
        elif self.spectral_filter_kind != 'MLP':
            why.append('spectral_filter_kind=%r' % (self.spectral_filter_kind,))
        if not self._fused_supported():
            why.append('hidden_dim=%r' % (self.hidden_dim,))
        if N > 32:
            why.append('%d > 32 nodes' % N)
        return ', '.join(why)

    # set by lanczosnet_amd.train.GraphedTrainStep: a device buffer [B, N, 1] that the step object
    # refills from the CPU generator before every replay (nothing may touch the host inside a HIP
    # graph); None: draw here
    _static_q1 = None

    def _draw_q1(self, B, N, device):
        """The Lanczos start vector: same RNG consumption as the reference — CPU generator, shape
        (B, N, 1) (model/ada_lanczos_net.py:161)."""
        q = self._static_q1
        if q is not None and tuple(q.shape) == (B, N, 1) and q.device == device:
            return q
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            # a CPU draw + host-to-device copy inside a HIP-graph capture would bake ONE start
            # vector into every replay (or abort the capture): the step object must provide it
            raise RuntimeError(
                'AdaLanczosNet: forward under stream capture needs the static start-vector buffer '
                '[%d, %d, 1] on %s (lanczosnet_amd.train.GraphedTrainStep sets `_static_q1`); got %s'
                % (B, N, device, None if q is None else (tuple(q.shape), str(q.device))))
        return torch.randn(B, N, 1).to(device)

    def _fused_backward_supported(self):
        """The HIP conv-stack backward with dense filters is built for hidden width 128 on the
        strip kernels (K a multiple of 4) and the reference's 4-Linear filter MLPs."""
        return (self._fused_supported() and self.hidden_dim[0] == 128 and self.backward_impl == 'hip'
                and self.num_eig_vec <= 32 and self.num_eig_vec % 4 == 0 and self._tiles16_channels_ok() and
                all(len(seq) == 7 and all(isinstance(seq[i], nn.Linear) for i in (0, 2, 4, 6))
                    for seq in self.spectral_filter))

    def _ada_filter_plan(self, plan):
        """The filter MLPs (model/ada_lanczos_net.py:271-278) on the NON-REDUNDANT part of their
        input and output.  T is symmetric tridiagonal (:226-231), so T^p is symmetric and zero
        beyond its p-th diagonal: the first Linear only needs the columns of the entries (i <= j,
        j - i <= p) — the weight columns of (i, j) and (j, i) are added — and the symmetrised
        output 0.5 (DD + DD^T) is one row per (i <= j) of the last Linear with the two weight
        rows averaged.  2000 -> 822 inputs and 2000 -> 1050 outputs for K = 20, scales
        [5, 7, 10, 20, 30]: 17 % fewer flops in the dominant GEMM chain; results differ from the
        unfolded evaluation by fp32 rounding of the folded weights (and by the last-bit asymmetry
        of an fp32 T^p).  Returns None (plain evaluation) unless every filter is the reference's
        4-Linear Sequential."""
        if 'ada_filters' in plan and self.fold_filter_mlp and (
                plan['ada_filters'] is None or plan['ada_filters']['mode'] == self.filter_gemm_mode):
            return plan['ada_filters']
        if not self.fold_filter_mlp:
            return None
        K, S = self.num_eig_vec, self.num_scale_long
        ok = all(len(seq) == 7 and all(isinstance(seq[i], nn.Linear) for i in (0, 2, 4, 6)) and
                 seq[0].in_features == K * K * S and seq[6].out_features == K * K * S
                 for seq in self.spectral_filter)
        fp = None
        if ok:
            dev = self.spectral_filter[0][0].weight.device
            # the index sets depend on (K, scales) only: built once per device and kept on the module
            # (boolean-mask indexing is a host round trip — not allowed while a HIP graph of the
            # training step is being captured, and the plan is rebuilt inside that graph)
            st = getattr(self, '_ada_fold_idx', None)
            if st is None or st['dev'] != dev:
                iu, ju = torch.triu_indices(K, K, device=dev)
                P = iu.numel()
                a_cols, b_cols, offd = [], [], []
                for sc, dist in enumerate(self.long_diffusion_dist):
                    keep = (ju - iu) <= int(dist)
                    i, j = iu[keep], ju[keep]
                    a_cols.append(i * (K * S) + sc * K + j)   # T_s[i][j] in cat(T_list, dim=2).view(B, -1)
                    b_cols.append(j * (K * S) + sc * K + i)
                    offd.append(i != j)
                a_cols, b_cols, offd = torch.cat(a_cols), torch.cat(b_cols), torch.cat(offd)
                # output row (s, p) of the folded last Linear; DD.view(B, K, K, S): row (i, j, s)
                sidx = torch.arange(S, device=dev).view(S, 1)
                r_ij = ((iu * K + ju) * S).view(1, P) + sidx     # [S, P]
                r_ji = ((ju * K + iu) * S).view(1, P) + sidx
                pair = torch.zeros((K, K), dtype=torch.long, device=dev)
                pair[iu, ju] = torch.arange(P, device=dev)
                pair[ju, iu] = torch.arange(P, device=dev)
                out_idx = (sidx.view(S, 1, 1) * P + pair.view(1, K, K)).reshape(-1)   # (s, i, j) -> row
                st = self._ada_fold_idx = dict(dev=dev, a_cols=a_cols, b_cols=b_cols,
                                               offd=offd.to(torch.float32), r_ij=r_ij.reshape(-1),
                                               r_ji=r_ji.reshape(-1), out_idx=out_idx, P=int(P))
            a_cols, b_cols, offd, out_idx, P = st['a_cols'], st['b_cols'], st['offd'], st['out_idx'], st['P']
            r_ij, r_ji = st['r_ij'], st['r_ji']
            n_in = a_cols.numel()
            in_pad = (-n_in) % 32
            n_out = S * P
            out_pad = (-n_out) % 32
            W1, W4, b4 = [], [], []
            for seq in self.spectral_filter:
                w = seq[0].weight.detach().float()
                w1 = w[:, a_cols] + w[:, b_cols] * offd
                W1.append(torch.nn.functional.pad(w1, (0, in_pad)).contiguous())
                w = seq[6].weight.detach().float()
                w4 = 0.5 * (w[r_ij] + w[r_ji])
                W4.append(torch.nn.functional.pad(w4, (0, 0, 0, out_pad)).contiguous())
                bb = seq[6].bias.detach().float()
                b4.append(torch.nn.functional.pad(0.5 * (bb[r_ij] + bb[r_ji]),
                                                  (0, out_pad)).contiguous())
            fp = dict(in_idx=a_cols, in_pad=in_pad, out_idx=out_idx, W1=W1, W4=W4, b4=b4,
                      n_in=n_in, n_out=n_out, mode=self.filter_gemm_mode)
            if self.filter_gemm_mode == 'f16x3_lib':
                fp['W16'] = [[ops.split_weight_f16x3(W1[t]),
                              ops.split_weight_f16x3(seq[2].weight),
                              ops.split_weight_f16x3(seq[4].weight),
                              ops.split_weight_f16x3(W4[t])]
                             for t, seq in enumerate(self.spectral_filter)]
            elif self.filter_gemm_mode == 'f16x3':
                fp['Wp'] = [[ops.f16x3_pack_weight(W1[t]),
                             ops.f16x3_pack_weight(seq[2].weight),
                             ops.f16x3_pack_weight(seq[4].weight),
                             ops.f16x3_pack_weight(W4[t])]
                            for t, seq in enumerate(self.spectral_filter)]
            elif self.filter_gemm_mode not in ('fp32', 'fp32_hip'):
                raise ValueError("filter_gemm_mode must be 'fp32', 'fp32_hip', 'f16x3' or 'f16x3_lib'")
        plan['ada_filters'] = fp
        return fp

    @torch.no_grad()
    def _ada_dense_filters(self, plan, tcat, keep=None):
        """tcat [B, K*K*S] (the T powers, `cat(T_list, dim=2).view(B, -1)`) -> the symmetrised
        dense filters DDp [num_layer, B, S, K, K] of every conv layer (:271-278).  keep: a list
        that receives the hidden activations (h1, h2, h3) of every layer's MLP where the fp32 chain
        produces them (training: the backward then needs no second MLP forward)."""
        B = tcat.shape[0]
        K, S = self.num_eig_vec, self.num_scale_long
        DDp = torch.empty((self.num_layer, B, S, K, K), dtype=torch.float32, device=tcat.device)
        fp = self._ada_filter_plan(plan)
        if fp is None:
            for t, seq in enumerate(self.spectral_filter):
                ops.ada_symmetrize_filters(seq(tcat), K, S, out=DDp[t])  # hipBLASLt GEMMs
            return DDp
        lin = torch.nn.functional.linear
        x = tcat.index_select(1, fp['in_idx'])
        if fp['in_pad']:
            x = torch.nn.functional.pad(x, (0, fp['in_pad']))
        if fp['mode'] == 'f16x3':
            # hand-written chain: the input planes once, then per conv layer four launches whose
            # epilogues hand the next Linear its (hi, lo) operand; two activation buffers ping-pong
            xp = ops.f16x3_split(x)
            hid = self._spectral_hidden
            bufs = [torch.zeros((2, xp.shape[1], hid), dtype=torch.float16, device=x.device)
                    for _ in range(2)]
            o = torch.empty((B, fp['W4'][0].shape[0]), dtype=torch.float32, device=x.device)
            for t, seq in enumerate(self.spectral_filter):
                w = fp['Wp'][t]
                h = ops.f16x3_linear(xp, w[0], seq[0].bias, B, hid, out_planes=bufs[0])
                h = ops.f16x3_linear(h, w[1], seq[2].bias, B, hid, out_planes=bufs[1])
                h = ops.f16x3_linear(h, w[2], seq[4].bias, B, hid, out_planes=bufs[0])
                ops.f16x3_linear(h, w[3], fp['b4'][t], B, o.shape[1], relu=False, out_f32=o)
                torch.index_select(o, 1, fp['out_idx'], out=DDp[t].view(B, S * K * K))
            return DDp
        if fp['mode'] == 'f16x3_lib':
            inv = 1.0 / ops.F16X3_WEIGHT_SCALE   # the weights' power-of-two scale
            x3 = ops.split_f16x3(x)
            for t, seq in enumerate(self.spectral_filter):
                w = fp['W16'][t]
                h = torch.mm(x3, w[0].t(), out_dtype=torch.float32)
                for i, li in ((1, 0), (2, 2), (3, 4)):
                    h3 = ops.split_f16x3(h, bias=seq[li].bias, alpha=inv, relu=True)
                    h = torch.mm(h3, w[i].t(), out_dtype=torch.float32)
                o = torch.addcmul(fp['b4'][t], h, h.new_full((), inv))
                torch.index_select(o, 1, fp['out_idx'], out=DDp[t].view(B, S * K * K))
            return DDp
        hip = fp['mode'] == 'fp32_hip'   # hand-written exact-fp32 Linear, bias + ReLU in its epilogue
        for t, seq in enumerate(self.spectral_filter):
            if hip:
                h1 = ops.f32_linear(x, fp['W1'][t], seq[0].bias, relu=True)
                h2 = ops.f32_linear(h1, seq[2].weight, seq[2].bias, relu=True)
                h3 = ops.f32_linear(h2, seq[4].weight, seq[4].bias, relu=True)
                o = ops.f32_linear(h3, fp['W4'][t], fp['b4'][t])
            else:
                # bias + ReLU in the library GEMM's epilogue (hipBLASLt through
                # torch._addmm_activation: bit-identical to linear + relu_, one launch instead of
                # two — the elementwise pass over a [1024, 4096] block costs 9 % of its GEMM)
                h1 = _linear_relu(x, fp['W1'][t], seq[0].bias)
                h2 = _linear_relu(h1, seq[2].weight, seq[2].bias)
                h3 = _linear_relu(h2, seq[4].weight, seq[4].bias)
                o = lin(h3, fp['W4'][t], fp['b4'][t])
            torch.index_select(o, 1, fp['out_idx'], out=DDp[t].view(B, S * K * K))
            if keep is not None:
                keep.append((h1, h2, h3))
        return DDp

    @torch.no_grad()
    def _hip_forward_ada(self, node_feat, L, mask, q1):
        B, N = node_feat.shape[0], node_feat.shape[1]
        K, S = self.num_eig_vec, self.num_scale_long
        with torch.no_grad():
            plan = self._plan()
            Lf = L if L.dtype == torch.float32 else L.float()
            Le = ops.ada_graph_laplacian(node_feat, self.embedding.weight, Lf[:, :, :, 0])
            T, Q = ops.ada_lanczos_layer(Le, mask, q1, K)
            tcat = ops.ada_t_powers(T, self.long_diffusion_dist).view(B, -1)
            DDp = self._ada_dense_filters(plan, tcat)
            Lp = ops.pack_laplacian(Lf)
            return ops.lanczosnet_forward(plan, node_feat, Lp, Q, DDp, mask)

    def _torch_forward_ada(self, node_feat, L, mask, q1, dropout=False):
        """Differentiable torch restatement (device tensors, batched, no Python loops over the
        batch) of model/ada_lanczos_net.py:101-368 incl. the quirks of `_lanczos_layer` — used
        inside backward (forward values of the nominal configuration always come from the HIP
        kernels) and as the forward of the configurations `_off_nominal` names.  Three stages:
        `_torch_ada_spectrum` (learned Laplacian, Lanczos layer, T powers), `_torch_ada_filters`
        (the filter MLPs) and `_torch_ada_conv` (conv stack + readout)."""
        if self.num_scale_long == 0:   # no Lanczos layer, no filters (:308,324)
            return self._torch_ada_conv(self.embedding(node_feat), L, None, None, mask, dropout=dropout)
        state, tcat, Q = self._torch_ada_spectrum(node_feat, L, mask, q1)
        return self._torch_ada_conv(state, L, Q, self._torch_ada_filters(tcat), mask, dropout=dropout)

    def _torch_ada_spectrum(self, node_feat, L, mask, q1):
        """model/ada_lanczos_net.py:101-270 -> (embedded node state [B,N,D], cat of the T powers
        [B, K*K*S] float32, Lanczos basis Q [B,N,K] float32).  Three differentiable stages, all in
        fp64: `_torch_ada_laplacian`, `_torch_ada_lanczos`, `_torch_ada_powers`."""
        state, Le = self._torch_ada_laplacian(node_feat, L)
        T, Q = self._torch_ada_lanczos(Le, mask, q1)
        return state, self._torch_ada_powers(T), Q.float()

    def _torch_ada_laplacian(self, node_feat, L):
        """The learned Laplacian (model/ada_lanczos_net.py:101-137) -> (embedded node state
        [B,N,D] float32, Le [B,N,N] float64).
        The learned Laplacian and the Lanczos recurrence run in fp64, like the forward kernel
        (lnz_ada_lanczos_layer): an fp32 recurrence — and its backward — carries rounding noise
        of 1e-6 .. 1e-4 that depends on the summation order; fp64 gives the exact-arithmetic
        gradient, which is what the reference's own autograd approximates.  (B, N, K) are tiny."""
        B = node_feat.shape[0]
        dd = torch.float64
        state = self.embedding(node_feat)
        st = state.to(dd)
        adj = (L[:, :, :, 0] != 0).to(dd)
        diff = st.unsqueeze(1) - st.unsqueeze(2)                # [B, i, j, D] = x_j - x_i
        dist2 = (diff * diff).sum(dim=3)
        sigma2 = dist2.reshape(B, -1).mean(dim=1).view(B, 1, 1)
        A = torch.exp(-dist2 / sigma2) * adj
        row_sum = A.sum(dim=2, keepdim=True)
        Dg = 1.0 / (row_sum + (row_sum == 0).to(dd)).pow(0.5)
        return state, Dg * A * Dg.transpose(1, 2)

    def _torch_ada_lanczos(self, Le, mask, q1):
        """The Lanczos layer (model/ada_lanczos_net.py:139-247) on the fp64 Laplacian Le ->
        (T [B,K,K], Q [B,N,K]) in fp64, incl. the quirks of SURVEY.md F6."""
        eps = 1.1920928955078125e-07
        B, N = Le.shape[0], Le.shape[1]
        K = self.num_eig_vec
        dd = torch.float64
        m = (mask != 0).to(dd).unsqueeze(2)
        Tit = min(N, K)
        q = q1.to(dd) * m
        q = q / torch.norm(q, 2, dim=1, keepdim=True)
        Qs, alphas, betas, valids = [torch.zeros_like(q), q], [], [torch.zeros(B, 1, 1, dtype=dd, device=Le.device)], []
        # The reference's Gram-Schmidt (:177-189) subtracts the projections on q_1 .. q_{ii-1} ONE
        # AFTER THE OTHER from the running z, twice: z <- P_{ii-1} ... P_1 z with P_j = I - q_j q_j^T
        # / (q_j^T q_j + EPS).  The product M_ii = P_{ii-1} M_{ii-1} is carried along instead of
        # replaying 2 (ii-1) vector updates per step: the same map (and the same derivative), one
        # batched N x N product per step instead of ~2000 tiny launches per forward in fp64.
        eye = torch.eye(N, dtype=dd, device=Le.device).unsqueeze(0)
        M = None
        for ii in range(1, Tit + 1):
            z = torch.bmm(Le, Qs[ii])
            alpha = (Qs[ii] * z).sum(dim=1, keepdim=True)
            z = z - alpha * Qs[ii] - betas[ii - 1] * Qs[ii - 1]
            if ii > 1 and self.use_reorthogonalization:   # (:177)
                qp = Qs[ii - 1]
                Pj = eye - torch.bmm(qp, qp.transpose(1, 2)) / (
                    (qp * qp).sum(dim=1, keepdim=True) + eps)
                M = Pj if M is None else torch.bmm(Pj, M)
                z = torch.bmm(M, torch.bmm(M, z))
            beta = torch.norm(z, p=2, dim=1, keepdim=True)
            ok = (beta >= 1.0e-4).to(dd)
            valids.append(ok if ii == 1 else valids[-1] * ok)
            Qs.append((z * valids[-1]) / (beta + eps))
            alphas.append(alpha)
            betas.append(beta)
        alpha = torch.cat(alphas, dim=1).squeeze(2)
        beta = torch.cat(betas[1:-1], dim=1).squeeze(2) if Tit > 1 else alpha[:, :0]
        valid = torch.cat(valids, dim=1).squeeze(2)
        idx = torch.minimum(valid.sum(dim=1), m.squeeze(2).sum(dim=1)).long()
        valid = valid * (torch.arange(Tit, device=Le.device)[None, :] < idx[:, None]).to(dd)
        alpha = alpha * valid
        beta = beta * valid[:, :-1]
        T = torch.diag_embed(alpha) + torch.diag_embed(beta, offset=1) + torch.diag_embed(beta, offset=-1)
        Q = torch.cat(Qs[1:-1], dim=2) * valid.unsqueeze(1)
        Q = Q * (torch.arange(N, device=Le.device)[None, :] < idx[:, None]).to(dd).unsqueeze(2)
        if Tit < K:
            T = torch.nn.functional.pad(T, (0, K - Tit, 0, K - Tit))
            Q = torch.nn.functional.pad(Q, (0, K - Tit))
        return T, Q

    def _torch_ada_powers(self, T):
        """T powers (model/ada_lanczos_net.py:262-270) of the fp64 T -> cat(T^p, dim=2).view(B, -1)
        float32 (fp64 products like lnz_ada_t_powers)."""
        B = T.shape[0]
        T_list, TT = [], T
        for ii in range(1, self.max_long_diffusion_dist + 1):
            if ii in self.long_diffusion_dist:
                T_list.append(TT)
            TT = torch.bmm(TT, T)
        return torch.cat(T_list, dim=2).view(B, -1).float()

    def _torch_ada_filters(self, tcat):
        """model/ada_lanczos_net.py:271-278: the symmetrised dense filters [B, K, K, S] of every
        conv layer."""
        B, K, S = tcat.shape[0], self.num_eig_vec, self.num_scale_long
        if self.spectral_filter_kind != 'MLP':
            # :282-284: the T powers themselves, L_s = Q T^p Q^T (cat(T_list, dim=2) is [B, K, S K])
            DD = tcat.view(B, K, S, K).permute(0, 1, 3, 2)
            return [DD] * self.num_layer
        out = []
        for t in range(self.num_layer):
            DD = self.spectral_filter[t](tcat).view(B, K, K, S)
            out.append((DD + DD.transpose(1, 2)) * 0.5)
        return out

    def _torch_ada_conv(self, state, L, Q, DDs, mask, dropout=False):
        """model/ada_lanczos_net.py:289-368: conv stack on given filters + readout.  dropout=True:
        `F.dropout(state, p)` after every conv layer where the reference applies it (:347) — same
        call, same shape, same order."""
        B, N = state.shape[0], state.shape[1]
        S = self.num_scale_long
        Lc = L.float().permute(0, 3, 1, 2).contiguous()
        Qt = Q.transpose(1, 2) if S > 0 else None
        m = (mask != 0).float().unsqueeze(2)
        for t in range(self.num_layer):
            DD = DDs[t] if S > 0 else None
            W, bias = self._mix_weight(t), self.filter[t].bias
            d_in = state.shape[2]
            Wc = W.view(W.shape[0], -1, d_in)
            Z = torch.einsum('bnd,ocd->bcno', state, Wc).unbind(1)   # C x [B, N, dout] (see _torch_forward)
            out = bias.view(1, 1, -1).expand(B, N, -1)
            c = 0
            for p in self.short_diffusion_dist:
                z = Z[c]
                for _ in range(p):
                    z = torch.bmm(Lc[:, 0], z)
                out = out + z
                c += 1
            for s_ in range(S):
                out = out + torch.bmm(Q, torch.bmm(DD[:, :, :, s_], torch.bmm(Qt, Z[c])))
                c += 1
            for e in range(self.num_edgetype + 1):
                out = out + torch.bmm(Lc[:, e], Z[c])
                c += 1
            state = torch.relu(out)
            if dropout:
                state = torch.nn.functional.dropout(state, self.dropout, training=True)
        y = self.filter[-1](state) * self.att_func(state)
        return (y * m).sum(dim=1) / m.sum(dim=1)


class _AdaLanczosNetFusedFunction(torch.autograd.Function):
    """AdaLanczosNet training through the HIP kernels.

    forward: learned Laplacian, Lanczos layer and T powers by their fp64 training kernels
    (lnz_ada_graph_laplacian_f64, lnz_ada_lanczos_layer_f64, lnz_ada_t_powers_f64: each keeps the
    state its backward needs; the inference kernels of these stages work from the fp32 Laplacian like
    the reference's fp32 run, and a basis that differs by the Lanczos recurrence's amplification
    of that rounding — 2.5e-5 on the test batch — would put the same 1e-5 between the filter
    gradients and the reference's float64 ones); filter MLPs (hidden activations kept where the
    fp32 chain produces them) and the fused conv kernel storing every layer's activations run on
    its (T powers, Q).
    backward:
      * readout head, node-state gradients, conv weights / biases: `_fused_conv_backward` — the same
        launches as LanczosNet, the kernels running their dense-filter eigen-space variant;
      * filters and basis: with Yq = Q^T X_l, Cq = Q^T dY_l per layer,
          dDD_{l,s} = Cq (Yq W_{l,s}^T)^T,
          dQ += dY_l (sum_s DD_s Yq W_s^T)^T + X_l (sum_s DD_s Cq W_s)^T      (DD_s symmetric)
        as batched library GEMMs on [B, K, .] blocks;
      * filter MLPs (model/ada_lanczos_net.py:271-278): plain GEMMs on the stored activations (the
        reference's unfolded weights), symmetrisation 0.5 (DD + DD^T) transposed onto dDD;
      * T powers (lnz_ada_t_powers_f64_backward) -> dT; Lanczos layer (:139-247):
        lnz_ada_lanczos_layer_f64_backward, the reverse sweep of the recurrence as one launch
        (dT, dQ) -> dLe; learned Laplacian (lnz_ada_graph_laplacian_f64_backward) -> dX, added to
        the conv stack's dX_0; embedding rows by a one-hot GEMM."""

    @staticmethod
    def forward(ctx, module, node_feat, L, mask, q1, *params):
        m = module
        plan = m._plan()
        B, N = node_feat.shape[0], node_feat.shape[1]
        K = m.num_eig_vec
        Lf = L if L.dtype == torch.float32 else L.float()
        mask_u8 = mask.to(torch.uint8).contiguous()
        # learned Laplacian -> Lanczos layer -> T powers, all fp64 (csrc/ada_lanczos_grad.hip), each
        # keeping the state its backward kernel needs
        state = m.embedding(node_feat)
        Le, lap_saved = ops.ada_graph_laplacian_f64(state, Lf[:, :, :, 0])
        T64, Q64, lws = ops.ada_lanczos_layer_f64(Le, mask, q1, K)
        tcat3, pow_saved = ops.ada_t_powers_f64(T64, m.long_diffusion_dist)
        tcat, Q = tcat3.view(B, -1), Q64.float().contiguous()
        keep = []
        DDp = m._ada_dense_filters(plan, tcat, keep=keep)
        Lp = ops.pack_laplacian(Lf)
        tiles = ops.plan_tiles(mask_u8, allow_pairs=ops.pairing_supported(plan))
        act = torch.zeros((m.num_layer, B, 32, plan['dhid']), dtype=torch.float32, device=Q.device)
        # (one launch: extents, their exclusive prefix sums = the compact row numbering, the total)
        n_mol = ops.node_extents_block(mask_u8)
        # (as _LanczosNetFusedFunction: under HIP-graph capture nothing may touch the host, the
        # backward then sizes its message matrix by the padded row count)
        ctx.static_rows = (torch.cuda.is_current_stream_capturing()
                           or bool(getattr(module, 'train_static_rows', False)))
        rtot = ev = None
        if not ctx.static_rows:
            rtot = torch.empty((1,), dtype=torch.int64, pin_memory=True)
            rtot.copy_(n_mol[-1:], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        score = ops.lanczosnet_forward(plan, node_feat, Lp, Q, DDp, mask_u8, tiling=tiles,
                                       act_out=act)
        ctx.module, ctx.cap, ctx.rtot, ctx.rtot_ready = m, tiles[1], rtot, ev
        # the fp64 spectrum state rides with the saved tensors (version counters, saved-tensor hooks,
        # torch's own "backward a second time" error); only the distance tuple stays on ctx
        (lap_x, lap_sv), (pow_T, pow_P, pow_dist) = lap_saved, pow_saved
        ctx.n_keep, ctx.pow_dist = len(keep), pow_dist
        ctx.save_for_backward(node_feat, L, mask, q1, mask_u8, Lp, Q, DDp, act, tiles[0], n_mol, tcat,
                              lap_x, lap_sv, Le, lws, pow_T, pow_P,
                              *[h for hs in keep for h in hs])
        return score

    @staticmethod
    def backward(ctx, grad_score):
        m = ctx.module
        node_feat, L, mask, q1, mask_u8, Lp, Q, DDp, act, tile_buf, n_mol, tcat = ctx.saved_tensors[:12]
        lap_x, lap_sv, Le, lws, pow_T, pow_P = ctx.saved_tensors[12:18]
        hs = ctx.saved_tensors[18:]
        tiles = (tile_buf, ctx.cap)
        plan = m._plan_backward()
        B, N, K = Q.shape
        Lnum, dh = m.num_layer, plan['dhid']
        din0 = plan['din0_raw']
        S, n_short = m.num_scale_long, m.num_scale_short
        n_chan = n_short + S + m.num_edgetype + 1
        # LNZ_ADA_DEBUG=1: stage timestamps (events) and intermediate gradients for tools/experiments
        dbg = os.environ.get('LNZ_ADA_DEBUG') == '1'
        marks = []

        def mark(name):
            if dbg:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((name, e))
        mark('start')
        grads, dy, dx0, x0 = _fused_conv_backward(m, plan, grad_score, node_feat, Q, DDp, mask_u8, Lp,
                                                  act, tiles, n_mol, ctx.static_rows, ctx.rtot,
                                                  ctx.rtot_ready)
        mark('conv_stack')

        # ---- dense filters and Lanczos basis.  Layers of one input width go through the batched
        #      GEMMs TOGETHER (layers 1 .. L-1 share d = dh: 18 launches instead of 56)
        Qt = Q.transpose(1, 2)
        dDDp = torch.empty_like(DDp)
        dQ = torch.zeros_like(Q)

        def filters_basis(layers, X, dYl, d):
            # X [G,B,N,d], dYl [G,B,N,dh] for the G conv layers `layers`
            G = len(layers)
            Wl = torch.stack([m._mix_weight(la).detach().view(dh, n_chan, d)[:, n_short:n_short + S, :]
                              for la in layers])                                  # [G, o, s, i]
            DDk = torch.stack([DDp[la] for la in layers]).permute(0, 1, 3, 2, 4).reshape(G * B, K, S * K)
            Qg = Qt.unsqueeze(0).expand(G, B, K, N).reshape(G * B, K, N)
            Yq = torch.bmm(Qg, X.reshape(G * B, N, d))                            # [GB,K,d]
            Cq = torch.bmm(Qg, dYl.reshape(G * B, N, dh))                         # [GB,K,dh]
            Bq = torch.bmm(Yq.view(G, B * K, d), Wl.permute(0, 3, 2, 1).reshape(G, d, S * dh))
            CW = torch.bmm(Cq.view(G, B * K, dh), Wl.reshape(G, dh, S * d))
            # dDD[b,s,k,j] = sum_o Cq[b,k,o] Bq[b,j,s,o]
            Bs = Bq.view(G * B, K, S, dh).permute(0, 2, 1, 3).reshape(G * B, S * K, dh)   # rows (s, j)
            dd = torch.bmm(Cq, Bs.transpose(1, 2)).view(G, B, K, S, K).permute(0, 1, 3, 2, 4)
            for g, la in enumerate(layers):
                dDDp[la] = dd[g]
            A = torch.bmm(DDk, Bs)                                                # [GB,K,dh]
            E = torch.bmm(DDk, CW.view(G * B, K, S, d).permute(0, 2, 1, 3).reshape(G * B, S * K, d))
            t = torch.bmm(dYl.reshape(G * B, N, dh), A.transpose(1, 2)) + \
                torch.bmm(X.reshape(G * B, N, d), E.transpose(1, 2))
            return t.view(G, B, N, K).sum(dim=0)

        dQ += filters_basis([0], x0[:, :N, :din0].unsqueeze(0), dy[0][:, :N].unsqueeze(0), din0)
        if Lnum > 1:
            dQ += filters_basis(list(range(1, Lnum)), act[:Lnum - 1, :, :N], dy[1:, :, :N], dh)

        mark('filters_basis')
        # ---- filter MLPs: DD = 0.5 (raw + raw^T) with raw = MLP(tcat).view(B, K, K, S)
        draw = 0.5 * (dDDp + dDDp.transpose(3, 4))                             # [L,B,S,K,K]
        draw = draw.permute(0, 1, 3, 4, 2).reshape(Lnum, B, K * K * S)
        dtcat = torch.zeros_like(tcat)
        lin = torch.nn.functional.linear
        for t, seq in enumerate(m.spectral_filter):
            l1, l2, l3, l4 = seq[0], seq[2], seq[4], seq[6]
            if ctx.n_keep:
                h1, h2, h3 = hs[3 * t:3 * t + 3]
            else:   # (no stored activations: plain evaluation / split-precision forward chains)
                h1 = torch.relu_(lin(tcat, l1.weight.detach(), l1.bias.detach()))
                h2 = torch.relu_(lin(h1, l2.weight.detach(), l2.bias.detach()))
                h3 = torch.relu_(lin(h2, l3.weight.detach(), l3.bias.detach()))
            g = draw[t]
            for layer, h_in, h_prev in ((l4, h3, h3), (l3, h2, h2), (l2, h1, h1)):
                grads[id(layer.weight)] = g.t() @ h_in
                grads[id(layer.bias)] = g.sum(dim=0)
                g = (g @ layer.weight.detach()) * (h_prev > 0).to(g.dtype)
            grads[id(l1.weight)] = g.t() @ tcat
            grads[id(l1.bias)] = g.sum(dim=0)
            dtcat += g @ l1.weight.detach()

        mark('filter_mlps')
        if dbg:
            m._dbg = dict(dDDp=dDDp, dQ=dQ, dtcat=dtcat, dx0=dx0[:, :N, :din0].clone(), Q=Q, DDp=DDp,
                          tcat=tcat, act=act, dy=dy)
        # ---- T powers -> Lanczos layer (the reverse sweep of the recurrence) -> learned Laplacian:
        #      three fp64 launches; then the embedding rows (one-hot^T dX as a GEMM, like LanczosNet)
        lap_saved, pow_saved = (lap_x, lap_sv), (pow_T, pow_P, ctx.pow_dist)
        dT = ops.ada_t_powers_f64_backward(pow_saved, dtcat)
        dLe = ops.ada_lanczos_layer_f64_backward(Le, lws, dT, dQ.double())
        dstate = dx0[:, :N, :din0] + ops.ada_graph_laplacian_f64_backward(lap_saved, dLe).float()
        if din0 in (16, 32, 64, 128):
            grads[id(m.embedding.weight)] = ops.embedding_grad(node_feat.contiguous(), dstate.contiguous(), din0,
                                                               m.num_atom)
        else:
            onehot = torch.nn.functional.one_hot(node_feat.reshape(-1), m.num_atom).to(torch.float32)
            grads[id(m.embedding.weight)] = onehot.t() @ dstate.reshape(-1, din0)
        mark('spectrum')
        if dbg:
            m._dbg['marks'] = marks

        out = [grads.get(id(p_)) if p_.requires_grad else None for p_ in m.parameters()]
        return (None, None, None, None, None) + tuple(out)


class _AdaLanczosNetFunction(torch.autograd.Function):
    """forward: HIP kernels (+ hipBLASLt filter MLPs); backward: autograd through
    `_torch_forward_ada` with the SAME start vector q1."""

    @staticmethod
    def forward(ctx, module, node_feat, L, mask, q1, *params):
        ctx.module = module
        ctx.save_for_backward(node_feat, L, mask, q1)
        return module._hip_forward_ada(node_feat, L, mask, q1)

    @staticmethod
    def backward(ctx, grad_score):
        module = ctx.module
        node_feat, L, mask, q1 = ctx.saved_tensors
        params = [p for p in module.parameters()]
        with torch.enable_grad():
            score = module._torch_forward_ada(node_feat, L, mask, q1)
            need = [p for p in params if p.requires_grad]
            grads = torch.autograd.grad(score, need, grad_score.contiguous(), allow_unused=True)
        it = iter(grads)
        out = [next(it) if p.requires_grad else None for p in params]
        return (None, None, None, None, None) + tuple(out)
