"""`AdaLanczosNet`: the learned Laplacian, the in-model Lanczos layer and the dense `Q MLP(T^k) Q^T`
filters in front of the conv stack of the <= 32-node fused kernels, and its two autograd
Functions."""
import os
import warnings

import torch

from .. import ops
from ._common import (FUSED_MAX_NODES, FUSED_WIDTHS, STRIP_WIDTH, _linear_relu, embedding_grad,
                      is_reference_filter_mlp, masked_readout, param_grad_tuple, torch_param_grads)
from ._small import _fused_conv_backward
from .lanczos_net import _LanczosNetBase


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
        # (a differentiable L: the Functions below return no gradient for it, the restatement does)
        diff = self._differentiable_inputs(node_feat=node_feat, L=L)
        needs_grad = self._needs_grad(node_feat, L)
        if diff and not off:
            self._warn_differentiable_inputs(diff)
            self.last_route = 'ada_torch'
            score = self._torch_forward_ada(node_feat, L, mask, q1, dropout=drop)
        elif off:
            # every configuration the reference class accepts runs: outside what the fused kernels
            # are built for, on the device-side restatement of the same operator sequence
            if off not in self.__dict__.setdefault('_warned_off_nominal', set()):
                self._warned_off_nominal.add(off)
                warnings.warn('lanczosnet_amd: AdaLanczosNet with %s is outside the HIP kernels (built '
                              'for re-orthogonalisation on, MLP filters over >= 1 long scale, hidden '
                              'width %d / %d, N <= %d, no training dropout): using the device-side '
                              'torch restatement of model/ada_lanczos_net.py:289-368, which is slower'
                              % ((off,) + FUSED_WIDTHS + (FUSED_MAX_NODES,)))
            self.last_route = 'ada_torch'
            with torch.set_grad_enabled(needs_grad):
                score = self._torch_forward_ada(node_feat, L, mask, q1, dropout=drop)
        elif needs_grad:
            # forward = HIP kernels; backward = HIP conv-stack backward + library GEMMs for the
            # filter MLPs + autograd through the fp64 Lanczos layer (_AdaLanczosNetFusedFunction)
            # where built, else autograd through the whole torch restatement
            fn = _AdaLanczosNetFusedFunction if self._fused_backward_supported() else \
                _AdaLanczosNetFunction
            self.last_route = 'ada_train_hip' if fn is _AdaLanczosNetFusedFunction else 'ada_train_torch'
            score = fn.apply(self, node_feat, L, mask, q1, *[p for p in self.parameters()])
        else:
            self.last_route = 'ada_hip'
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
        if N > FUSED_MAX_NODES:
            why.append('%d > %d nodes' % (N, FUSED_MAX_NODES))
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
        return (self._fused_supported() and self.hidden_dim[0] == STRIP_WIDTH and self.backward_impl == 'hip'
                and self.num_eig_vec <= 32 and self.num_eig_vec % 4 == 0 and self._tiles16_channels_ok() and
                all(is_reference_filter_mlp(seq) for seq in self.spectral_filter))

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
        ok = all(is_reference_filter_mlp(seq) and
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
        return masked_readout(self, state, mask)


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
    @torch.autograd.function.once_differentiable
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
        grads[id(m.embedding.weight)] = embedding_grad(m, node_feat, dstate.contiguous(), N, din0)
        mark('spectrum')
        if dbg:
            m._dbg['marks'] = marks

        return param_grad_tuple(m, grads, 5)


class _AdaLanczosNetFunction(torch.autograd.Function):
    """forward: HIP kernels (+ hipBLASLt filter MLPs); backward: autograd through
    `_torch_forward_ada` with the SAME start vector q1."""

    @staticmethod
    def forward(ctx, module, node_feat, L, mask, q1, *params):
        ctx.module = module
        ctx.save_for_backward(node_feat, L, mask, q1)
        return module._hip_forward_ada(node_feat, L, mask, q1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_score):
        module = ctx.module
        node_feat, L, mask, q1 = ctx.saved_tensors
        with torch.enable_grad():
            score = module._torch_forward_ada(node_feat, L, mask, q1)
            grads = torch_param_grads(module, score, grad_score)
        return param_grad_tuple(module, grads, 5)
