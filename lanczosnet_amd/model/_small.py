"""Graphs of at most 32 nodes: the fused MFMA path (csrc/conv_forward.hip, csrc/conv_strip.hip).

`_SmallMixin` holds the envelope of these kernels, the packed-parameter plan, its transposed form
for the backward and the inference forward (pack + tile plan, spectral gains, fused network: three
launches).  Training: `_LanczosNetFusedFunction` (HIP backward, hidden width 128)
or `_LanczosNetFunction` (autograd through the module's torch restatement).
`_fused_conv_backward` is the part of the HIP backward that AdaLanczosNet shares."""
import os

import torch

from .. import ops
from ._common import (FUSED_WIDTHS, MAX_CHANNELS, MAX_INPUT_DIM, MAX_OUTPUT_DIM, MAX_SHORT_SCALES,
                      STRIP_MAX_LONG_SCALES, STRIP_WIDTH, _spectral_mlp_param_grads, _tn_split_k,
                      embedding_grad, head_parts, head_params, input_state, masked_readout,
                      param_grad_tuple, scatter_head_grads, spectral_mlp_operands, torch_param_grads)


class _SmallMixin:
    def _fused_supported(self):
        """True when the fused MFMA kernel is built for this architecture (uniform hidden width
        64 or 128, input width <= 128, head width <= 31)."""
        hid = set(self.hidden_dim[:self.num_layer])
        return (len(hid) == 1 and next(iter(hid)) in FUSED_WIDTHS and self.input_dim <= MAX_INPUT_DIM
                and self.output_dim <= MAX_OUTPUT_DIM)

    def _fused_channels_ok(self):
        """Scale and channel counts the fused forward kernels are built for (csrc/conv_forward.hip
        launch_conv, csrc/conv_strip.hip strip_forward_eligible): at most 8 short and 12 long
        diffusion scales, at most 32 message channels in all.  Beyond that the module takes the
        library path, like a width outside the kernels."""
        return self.num_scale_short <= MAX_SHORT_SCALES and self._tiles16_channels_ok()

    def _check_supported(self):
        if any(d == 'inf' for d in self.short_diffusion_dist + self.long_diffusion_dist):
            raise NotImplementedError("diffusion distance 'inf' is not built in the HIP path")
        if not self._fused_supported():
            raise NotImplementedError(
                'fused kernel is built for a uniform hidden width of %d or %d, input width <= %d, '
                'got hidden_dim=%r input_dim=%r' % (FUSED_WIDTHS + (MAX_INPUT_DIM, self.hidden_dim,
                                                                    self.input_dim)))

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
        # (input and head widths: `_check_supported` above)
        split_strips = (self.gemm_mode == 'f16x3' and dhid == STRIP_WIDTH and self.filter_kind == 0
                        and self._tiles16_channels_ok() and self.num_scale_short == 0)
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
        # (tests/forward_cases.narrow_plan rebuilds din0 / Wp / w_off / embedding / Wf of this dict for an unpadded
        # 32-column layer 0 of a width-128 model, to reach lanczosnet_forward_kernel<4,10,0,0,-1>: keep it in step)
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
        # the folded weights of the rare bond-type channels, packed once per weight set where the strip
        # forward may fold (csrc/conv_strip.hip: read through the weight ring instead of summed per wave)
        plan['Wf'] = None
        if ops.fold_weights_eligible(plan):
            plan['Wf'] = ops.pack_fold_weights(plan['Wp'], w_off, self.num_layer, din0p, dhid,
                                               self.num_scale_short, self.num_scale_long, plan['n_edge'])
        if self.gemm_mode == 'f16x3' and not split_strips:
            raise NotImplementedError(
                "gemm_mode='f16x3' runs inside the strip kernel: LanczosNet / LanczosNetGeneral with "
                "hidden width %d, input width <= %d, no short-diffusion scales, <= %d long scales, "
                "<= %d channels in all, output width <= %d"
                % (STRIP_WIDTH, MAX_INPUT_DIM, STRIP_MAX_LONG_SCALES, MAX_CHANNELS, MAX_OUTPUT_DIM))
        if self.gemm_mode not in ('fp32', 'bf16', 'f16x3'):
            raise ValueError("gemm_mode must be 'fp32', 'f16x3' (N <= 32) or 'bf16' (N > 32)")
        if self._has_mlp() and self.filter_kind == 0:
            plan['mlp_pack'] = ops.pack_spectral_mlp_layers(spectral_mlp_operands(self),
                                                            self.num_scale_long)
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

    def _tiles16_channels_ok(self):
        """Channel counts of the strip kernels (csrc/conv_strip.hip strip_forward_eligible), the
        only home of the training forward and the input-gradient pass: at most 12 long-diffusion
        channels, at most 32 channels in all."""
        n_long, n_short = len(self.long_diffusion_dist), len(self.short_diffusion_dist)
        return (n_long <= STRIP_MAX_LONG_SCALES
                and n_short + n_long + self.num_edgetype + 1 <= MAX_CHANNELS)

    def _fused_backward_supported(self):
        """The HIP backward (lnz_lanczosnet_input_grad / _messages) is built for the exact-fp32
        LanczosNet kernel with hidden width 128."""
        return (self.filter_kind == 0 and self.gemm_mode == 'fp32' and self._fused_supported()
                and self.hidden_dim[0] == STRIP_WIDTH and self.backward_impl == 'hip'
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
    Wo, bo, Wg, bg = head_parts(m)
    hip_head = (m.head_grad_impl == 'hip' and dh == STRIP_WIDTH and N <= 32 and
                Wo.shape[0] <= MAX_OUTPUT_DIM and mask_u8.shape[1] == N)
    hg = None
    with torch.enable_grad():
        if not hip_head:
            # (the stacked head from the live parameters: autograd reaches them)
            XL = act[Lnum - 1][:, :N].detach().requires_grad_(True)
            score = masked_readout(m, XL, mask_u8, stacked=head_params(m, live=True))
            hg = torch.autograd.grad(score, [XL, Wo, bo, Wg, bg], grad_score.contiguous())
    dy = torch.zeros((Lnum, B, 32, dh), dtype=torch.float32, device=dev)
    if hg is not None:
        for p_, g_ in zip((Wo, bo, Wg, bg), hg[1:]):
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
        dWh, dbh, db_last = ops.head_backward(act[Lnum - 1], mask_u8, grad_score, Wo.detach(), bo.detach(), N,
                                              dy[Lnum - 1], row_off=row_off, dY_compact=dyc[Lnum - 1],
                                              Wgate=Wg.detach(), bgate=bg.detach())
        scatter_head_grads(m, grads, dWh, dbh)
    ops.lanczosnet_input_grad(plan, Lp, V, G, mask_u8, act, dy, dx0, tiles, row_off=row_off,
                              dy_compact=dyc, dbias_part=dbp)

    # ---- X_0
    x0 = torch.zeros((B, 32, din0p), dtype=torch.float32, device=dev)
    x0[:, :N, :din0] = input_state(m, node_feat, detached=True)

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
    @torch.autograd.function.once_differentiable
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

        # ---- embedding rows
        if not m.general:
            grads[id(m.embedding.weight)] = embedding_grad(m, node_feat, dx0, N, din0)
        return param_grad_tuple(m, grads, 6)


class _LanczosNetFunction(torch.autograd.Function):
    """forward: the fused HIP path.  backward: parameter gradients by autograd through
    `_torch_forward` (inputs L, D, V, mask, node ids are data: no gradient)."""

    @staticmethod
    def forward(ctx, module, node_feat, L, D, V, mask, *params):
        ctx.module = module
        ctx.save_for_backward(node_feat, L, D, V, mask)
        return module._hip_forward(node_feat, L, D, V, mask)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_score):
        module = ctx.module
        node_feat, L, D, V, mask = ctx.saved_tensors
        with torch.enable_grad():
            score = module._torch_forward(node_feat, L, D, V, mask)
            grads = torch_param_grads(module, score, grad_score)
        return param_grad_tuple(module, grads, 6)
