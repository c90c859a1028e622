"""Graphs of 33 to 128 nodes: every layer, the head and the readout in ONE launch
(csrc/conv_mid.hip), and its opt-in HIP backward (`_MidGraphFusedFunction`, csrc/conv_mid_grad.hip;
DESIGN.md §4.9b)."""
import os

import torch

from .. import ops
from ._common import (FUSED_MAX_NODES, MAX_OUTPUT_DIM, MID_MAX_K, MID_MAX_NODES, MID_MAX_OPERATORS,
                      _spectral_mlp_param_grads, embedding_grad, input_state, masked_readout,
                      param_grad_tuple, scatter_head_grads)


class _MidMixin:
    # graphs of 33..128 nodes in training: 'hip' = the backward of the one-launch kernel
    # (_MidGraphFusedFunction, csrc/conv_mid_grad.hip), 'torch' (default) = autograd through
    # `_torch_forward`.  Opt-in until its step time is recorded
    mid_backward_impl = os.environ.get('LANCZOSNET_MID_BACKWARD', 'torch')
    mid_graph_kernel = os.environ.get('LANCZOSNET_MID_KERNEL', '1') != '0'

    def _mid_hip_supported(self, N, K, channels):
        """lnz_midgraph_forward: exact fp32, uniform hidden width 128, input width <= 128, no
        short-diffusion powers, K <= 32, <= 16 long scales, <= 2 operator channels, 32 < N <= 128."""
        return (self.mid_graph_kernel and FUSED_MAX_NODES < N <= MID_MAX_NODES and K <= MID_MAX_K
                and channels <= MID_MAX_OPERATORS and self.gemm_mode == 'fp32' and self.filter_kind == 0
                and self._strip_widths_ok() and self.num_scale_short == 0
                and self.num_scale_long <= self.gains_kernel_max_scales
                and self.output_dim <= MAX_OUTPUT_DIM and self._channel_order() is None)

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
            mid = cache['mid'] = dict(
                W=torch.cat(Ws).contiguous(), din0p=din0p,
                bias=torch.stack([self.filter[t].bias.detach().float() for t in range(self.num_layer)]).contiguous())
            mid['Whead'], mid['bhead'] = self._plan_head(cache)
        return cache

    @torch.no_grad()
    def _mid_graph_forward_hip(self, node_feat, L, D, V, mask):
        plan = self._plan_mid()
        mid = plan['mid']
        X0 = input_state(self, node_feat, width=mid['din0p'], as_float=True)
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
        X0 = input_state(m, node_feat, width=mid['din0p'], detached=True, as_float=True).contiguous()
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
    @torch.autograd.function.once_differentiable
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
        if m.head_grad_impl == 'hip':
            dWh, dbh = ops.midgraph_head_grad(Xwork, mask_u8, grad_score, mid['Whead'], mid['bhead'], dOut)
        else:
            with torch.enable_grad():
                XL = Xwork[-1][:, :N].detach().requires_grad_(True)
                Wh = mid['Whead'].detach().requires_grad_(True)
                bh = mid['bhead'].detach().requires_grad_(True)
                dXL, dWh, dbh = torch.autograd.grad(masked_readout(m, XL, mask_u8, stacked=(Wh, bh)),
                                                    [XL, Wh, bh], grad_score.contiguous())
            dOut[-1].zero_()
            dOut[-1][:, :N] = dXL * (XL > 0).float()
        scatter_head_grads(m, grads, dWh, dbh)
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
            grads[id(m.embedding.weight)] = embedding_grad(m, node_feat, dx0, N, din0)
        return param_grad_tuple(m, grads, 6)
