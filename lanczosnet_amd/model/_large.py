"""Graphs beyond the 32-node MFMA tile: the hand-written streaming kernels (csrc/conv_large.hip),
the node-space term on the nonzeros of L (csrc/conv_sparse.hip) with their channel-fold and
sparse-backoff state, and the library-GEMM restatement (hipBLASLt through torch) of everything the
kernels are not built for.  `_plan_large` is also the cache the 33..128-node plan lives in.
`_LargeSparseFusedFunction`: the opt-in HIP backward of the exact-fp32 sparse layers (csrc/conv_sparse_grad.hip)
on a `_SparseOperators` — R symmetric operators as sparse images serving C weight channels: an edge-list batch
(R = 1, C = 2), a typed one (R = C = 3 .. 8 distinct operator channels, one image each; §4.9d),
or a DENSE collated L beyond 128 nodes, which reaches the Function through `_dense_operators`: its image(s), and
the symmetry check that an edge list does not need (csrc/sparse_symmetry.hip; §4.9e).  The Function's forward
and the inference path run the same layer loop (`_sparse_conv_layers`)."""
import os
import warnings

import torch

from .. import ops
from ._common import (LARGE_MAX_K, LARGE_MAX_OPERATORS, MID_MAX_NODES, _spectral_mlp_param_grads, _tn_split_k,
                      embedding_grad, head_params, input_state, masked_readout, param_grad_tuple, scatter_head_grads,
                      spectral_mlp_operands)


class _LargeMixin:
    # graphs beyond 32 nodes, fp32-grade mode of the streamed kernels: 3 = three bf16 pieces per
    # operand (six products), 2 = two fp16 pieces (three products, 2/3 of the operand bytes)
    large_split_planes = int(os.environ.get('LANCZOSNET_LARGE_PLANES', '3'))
    # lnz_spectral_gains / lnz_pack_spectral_mlp_layers: csrc/gains_body.hpp SMAX
    gains_kernel_max_scales = 16
    # edge-list batches (an untyped SparseLaplacian) in training: 'hip' = the backward on the sparse image
    # (_LargeSparseFusedFunction, csrc/conv_sparse_grad.hip), 'torch' (default) = densify + autograd
    # through `_torch_forward`.  Opt-in: its step time is recorded, not yet a reason
    large_backward_impl = os.environ.get('LANCZOSNET_LARGE_BACKWARD', 'torch')
    # typed edge-list batches (a SparseLaplacian with `images`: two or more edge types) in training: 'hip' =
    # the same Function over the channels' images (R = channels), 'torch'
    # (default) = densify + autograd.  A switch of its own: each governs its own kind of batch
    large_typed_backward_impl = os.environ.get('LANCZOSNET_LARGE_BACKWARD_TYPED', 'torch')
    # DENSE collated batches (a float32 L [B,N,N,E+1] tensor: GraphData.collate_fn, collate_graph_adjacency)
    # beyond 128 nodes in training: 'hip' = the same backward on the sparse image(s) of the tensor, where the
    # operators are symmetric (lnz_large_sparse_image_symmetry), 'torch' (default) = autograd
    # through `_torch_forward`.  It governs dense tensors only; the two switches above govern theirs
    large_dense_backward_impl = os.environ.get('LANCZOSNET_LARGE_BACKWARD_DENSE', 'torch')

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
        state = input_state(self, node_feat)
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
        return masked_readout(self, state, mask)

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
                buf = ops.pack_spectral_mlp_layers(spectral_mlp_operands(self), self.num_scale_long)
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
                # several operator classes: their fp32 blocks stacked [R * 128, d32], NOT summed
                # (lnz_large_sparse_conv_channels_f32: one lnz_f32_linear per channel)
                Wn32s = torch.nn.functional.pad(Wn[:, :, :d_in].permute(1, 0, 2).reshape(len(reps) * dout, d_in),
                                                (0, d32 - d_in)).contiguous() if len(reps) > 1 else None
                layers.append(dict(Wb=Wb, Wt=Wt, bias=self.filter[t].bias.detach().float().contiguous(),
                                   din=d_in, Wn32=Wn32, Wn32s=Wn32s))
            cache['conv'][key] = layers
        return cache

    def _plan_head(self, cache):
        """The stacked head + gate rows `head_params` of the large-plan `cache` (built once per
        parameter signature; the 33..128-node plan and the readout kernel share them)."""
        if 'head' not in cache:
            cache['head'] = head_params(self)
        return cache['head']

    def _large_hip_supported(self, K, channels=1):
        """lnz_large_*: uniform hidden width 128, input width <= 128, no short-diffusion powers,
        K <= 64, <= 16 long scales, at most 8 operator channels (the pack kernel's channel map,
        csrc/conv_large.hip: `LargeChanMap`; more edge types take the library path like any other
        unsupported shape)."""
        return (self._strip_widths_ok() and self.num_scale_short == 0 and K <= LARGE_MAX_K
                and channels <= LARGE_MAX_OPERATORS
                and self.num_scale_long <= self.gains_kernel_max_scales)

    def _large_backward_supported(self, K, channels):
        """The HIP backward of the exact-fp32 sparse layers (lnz_large_grad_project / _spectral / _input):
        the envelope of `_large_hip_supported` in a split-precision mode (the node-space term exact
        fp32), the reference's channel order, diagonal gains; selected by `large_backward_impl ==
        'hip'` where `backward_impl` asks for HIP at all.  WHAT the batch is (one operator given as a
        clean sparse image) is `_route`'s `sparse_one_operator`."""
        return self.large_backward_impl == 'hip' and self._large_backward_envelope(K, channels)

    def _large_backward_envelope(self, K, channels):
        """What the HIP backwards on sparse images share, whichever switch selects them."""
        return (self.backward_impl == 'hip'
                and self._large_hip_supported(K, channels) and self.gemm_mode != 'bf16'
                and self.large_split_planes != 1 and self.large_sparse
                and self._channel_order() is None and self.filter_kind == 0)

    def _large_typed_backward_supported(self, K, channels):
        """The HIP backward over the R = 3 .. 8 operator channels of a typed batch (lnz_large_sparse_conv_split_f32,
        lnz_large_grad_input_channels): `_large_backward_envelope`, selected by `large_typed_backward_impl == 'hip'`.
        WHAT the batch is (clean images with their fp32 values) is `_route`'s `sparse_typed_operators`."""
        return (self.large_typed_backward_impl == 'hip' and 3 <= channels <= LARGE_MAX_OPERATORS
                and self._large_backward_envelope(K, channels))

    def _sparse_one_operator(self, L, drop, capturing):
        """`_route`'s `sparse_one_operator` for this call: L is an untyped SparseLaplacian (one edge
        type: two channels that are ONE operator) whose image carries its fp32 values and raised no
        flag.  The flag word is read here — the image was built at collate time, the wait is on
        finished work — and only where the answer can matter."""
        if not (isinstance(L, ops.SparseLaplacian) and L.images is None and L.channels == 2
                and L.image is not None and L.image.values is not None and L.N <= 65536):
            return False
        if drop or capturing or not self._needs_grad() or not self._large_backward_supported(0, L.channels):
            return False
        return int(L.image.flags.item()) == 0

    def _sparse_typed_operators(self, L, drop, capturing):
        """`_route`'s `sparse_typed_operators` for this call: L is a typed SparseLaplacian (two or more edge
        types: R = 3 .. 8 distinct operators) whose images carry their fp32 values and raised no flag.  The flag
        word is read last, and only where the answer can matter."""
        if not (isinstance(L, ops.SparseLaplacian) and L.images is not None
                and 3 <= L.channels <= LARGE_MAX_OPERATORS and L.images.values is not None and L.N <= 65536):
            return False
        if drop or capturing or not self._needs_grad() or not self._large_typed_backward_supported(0, L.channels):
            return False
        return int(L.images.flags.item()) == 0

    def _large_dense_backward_supported(self, K, channels):
        """The HIP backward for a dense collated L: `_large_backward_envelope`, selected by
        `large_dense_backward_impl == 'hip'`.  WHAT the tensor is (symmetric operators as clean sparse images) is
        `_route`'s `dense_one_operator` / `dense_channel_operators`."""
        return self.large_dense_backward_impl == 'hip' and self._large_backward_envelope(K, channels)

    def _dense_operators(self, L, K, drop, capturing):
        """`_route`'s `dense_one_operator` ('one') / `dense_channel_operators` ('each') for this call, or None.
        L is a dense float32 tensor on the device, beyond 128 nodes, whose operator channels are
          'one'   ONE operator class — every channel equals channel 0: the reference's single-edge-type collate or
                  a zero-stride expanded view — or
          'each'  3 .. 8 distinct channels under `large_sparse_channels == 'each'`,
        every operator SYMMETRIC (the backward forms L dP for L^T dP) and no image flag raised.  The image is the
        one riding on L where it carries values, else it is built here and left riding on L (the Function does
        not build it twice); the symmetry status and the flag word come back through pinned memory behind ONE
        event.  Asked only where the answer can matter (switch on, envelope met); the verdict stays on the image
        object, so a tensor that is reused asks once.  A refusal (channels differ under 'one', a row beyond
        row_cap, an asymmetric operator) warns once per module and pauses the question for `large_sparse_backoff`
        dense batches on this device, twice as many after every further refusal in a row."""
        if self.large_dense_backward_impl != 'hip' or drop or capturing or not self._needs_grad():
            return None
        if isinstance(L, ops.SparseLaplacian) or not isinstance(L, torch.Tensor):
            return None
        if L.dim() != 4 or L.dtype != torch.float32 or not L.is_cuda:
            return None
        N, Cn = L.shape[1], L.shape[3]
        if N <= MID_MAX_NODES or N > 65536 or Cn != self.num_edgetype + 1 \
                or not self._large_dense_backward_supported(K, Cn):
            return None
        if self.large_sparse_channels not in ('one', 'each'):
            raise ValueError("large_sparse_channels is 'one' or 'each', got %r" % (self.large_sparse_channels,))
        kind = 'each' if (self.large_sparse_channels == 'each' and 3 <= Cn <= LARGE_MAX_OPERATORS
                          and L.stride(3) != 0) else 'one'
        img = ops.attached_sparse_images(L) if kind == 'each' else ops.attached_sparse_image(L)
        if img is not None and img.values is None:
            img = None
        if img is not None and img.symmetric is not None:
            return kind if img.symmetric else None
        st = self.__dict__.setdefault('_large_dense_state', {}).setdefault(L.device.index, {})
        if self._paused(st):
            return None
        st['image_from'] = 'collate' if img is not None else 'module'
        if img is None and kind == 'each':
            img = ops.large_sparse_image_channels(L)
            ops.attach_sparse_images(L, img)
        elif img is None:
            img = ops.large_sparse_image(L, values=True)
            ops.attach_sparse_image(L, img)
        words = self._words_behind_event(st, img.flags, ops.large_sparse_image_symmetry(img))()
        flags, status = words[0], words[1:]
        st['last_flags'], st['last_status'] = flags, status
        img.symmetric = flags == 0 and not any(status)
        self._pause_after(st, refused=not img.symmetric)
        if img.symmetric:
            return kind
        if not getattr(self, '_warned_dense_refusal', False):
            self._warned_dense_refusal = True
            warnings.warn("lanczosnet_amd: large_dense_backward_impl = 'hip': %s; the dense batch trains through "
                          "the torch route, and the next %d dense batches on this device are not examined"
                          % (self._dense_refusal(L, img, flags, status), st['skip']), UserWarning)
        return None

    @staticmethod
    def _dense_refusal(L, img, flags, status):
        """The first offending graph and the reason, for the warning (once per module: it may look at L)."""
        B, cap = L.shape[0], img.cap
        if flags & 2:
            first = next((b for b in range(B) if int((L[b] != 0).sum(dim=1).max()) > cap), None)
            return 'graph %s has a row of more than row_cap = %d nonzeros' % (first, cap)
        if flags & 1:
            first = next((b for b in range(B) if not bool((L[b] == L[b][..., :1]).all())), None)
            return ("the operator channels of graph %s differ (large_sparse_channels = 'each' serves 3 .. %d "
                    "distinct channels)" % (first, LARGE_MAX_OPERATORS))
        w = next(i for i, x in enumerate(status) if x)
        why = ' and '.join(text for bit, text in ops.SYMMETRY_REASONS if status[w] & bit)
        return 'graph %d (operator channel %d) is not symmetric: %s' % (w % B, w // B, why)

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
        if not self.large_fold or Cn == 1 or Cn > LARGE_MAX_OPERATORS:
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
        compare = (self.large_fold and 1 < Cn <= LARGE_MAX_OPERATORS and not capturing
                   and Lf.stride(3) != 0)
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
    # A dense L with SEVERAL distinct operator channels (two or more edge types): 'one' claims one
    # operator class, finds the claim refuted (flag bit 0) and backs off to the streamed kernels;
    # 'each' (or LANCZOSNET_LARGE_SPARSE_CHANNELS=each) reads L once into one image per channel
    # (lnz_large_sparse_image_channels) and gathers over all of them (lnz_large_sparse_conv_channels).
    # A typed SparseLaplacian (collate_graph_edges with num_edge_type >= 2) carries those images and
    # takes that gather whatever this says.
    large_sparse_channels = os.environ.get('LANCZOSNET_LARGE_SPARSE_CHANNELS', 'one')

    def _densify(self, L, why):
        """A SparseLaplacian batch outside the sparse path: its dense L (`.to_dense()`, the tensor
        collate_graph_adjacency builds), announced once per module."""
        if not getattr(self, '_warned_densify', False):
            warnings.warn('lanczosnet_amd: %s: the SparseLaplacian batch is densified ([B,N,N,2] float32, '
                          '%.1f MB) and takes the dense route' % (why, L.B * L.N * L.N * 8 / 1e6), UserWarning)
            self._warned_densify = True
        return L.to_dense()

    large_head_kernel = os.environ.get('LANCZOSNET_LARGE_HEAD', '1') != '0'
    large_sparse_backoff = 32

    def _large_sparse_layers(self, node_feat, Lf, Vf, G, planes=1):
        """-> the last conv layer's state [B,N,128], or None when the batch has to take the
        streamed kernels (disabled, capturing, N beyond 16-bit columns, or a raised image flag).
        planes = 1: bf16 values x bf16 features (the streamed bf16 form's products); planes = 2, 3
        (the split-precision modes): the node-space term in EXACT fp32 — fp32 values x fp32
        features of lnz_f32_linear — and the lift from `planes` pieces as in the streamed form."""
        N, Cn = Lf.shape[1], Lf.shape[3]
        if not self.large_sparse or N > 65536 or torch.cuda.is_current_stream_capturing():
            return None
        st = self.__dict__.setdefault('_large_sparse_state', {}).setdefault(Lf.device.index, {})
        if self._paused(st):
            return None
        exact = planes != 1
        if self.large_sparse_channels not in ('one', 'each'):
            raise ValueError("large_sparse_channels is 'one' or 'each', got %r" % (self.large_sparse_channels,))
        if isinstance(Lf, ops.SparseLaplacian) and Lf.images is not None:
            img = Lf.images                       # a typed batch: one image per channel, from the edge lists
            st['image_from'] = 'edges'
        elif isinstance(Lf, ops.SparseLaplacian):
            img = Lf.image                        # built from the edge lists: no launch, no dense L
            st['image_from'] = 'edges'
        elif self.large_sparse_channels == 'each' and 1 < Cn <= LARGE_MAX_OPERATORS and Lf.stride(3) != 0:
            img = ops.large_sparse_image_channels(Lf)   # the images of several operators
            st['image_from'] = 'forward'
        else:
            img = ops.attached_sparse_image(Lf)   # left by the collate's Lanczos pass over this very tensor
            if img is not None and exact and img.values is None:
                img = None                        # (an image without the unrounded values)
            st['image_from'] = 'collate' if img is not None else 'forward'
            if img is None:
                img = ops.large_sparse_image(Lf, values=exact)
        read_flags = self._words_behind_event(st, img.flags)
        state = self._sparse_conv_layers(node_feat, img, Cn, Vf, G, planes)[1]
        flags = st['last_flags'] = read_flags()[0]   # the image launch: long finished
        # (a data set of dense graphs raises it every time: the pause doubles, up to 32 x)
        self._pause_after(st, refused=flags != 0)
        return None if flags else state

    def _sparse_conv_layers(self, node_feat, img, channels, Vf, G, planes, out=None):
        """The conv layers on the sparse image(s) `img` — a LargeSparseImage: ONE operator serving all `channels`
        weight channels, their blocks summed; a LargeSparseImages: one operator per channel — for the inference
        path and the training Function alike: the same launches on the same operands.  Layer t writes into
        out[t] of a caller's [num_layer,B,N,128] buffer, or the layers ping-pong between two buffers of their own.
        -> (the padded input state, the last layer's state [B,N,128], the work buffers)."""
        multi = isinstance(img, ops.LargeSparseImages)
        exact = planes != 1
        Vb = ops.large_pack_vectors(Vf, planes)
        classes = tuple(range(channels)) if multi else (0,) * channels
        plan = self._plan_large(planes, classes)
        # (lnz_f32_linear's K: the exact form takes the input columns padded to a multiple of 32)
        state = X0 = input_state(self, node_feat, width=(self.input_dim + 31) // 32 * 32 if exact else None,
                                 as_float=True).contiguous()
        bufs = [None, None]
        work = ops.large_sparse_work_buffers(img.B, img.N, Vf.device, R=img.R if multi else None, planes=planes)
        weight = 'Wb' if not exact else 'Wn32s' if multi else 'Wn32'
        for t, lay in enumerate(plan['conv'][(planes, classes)]):
            state = ops.large_sparse_conv_layer(state, lay['din'], img, Vb, Vf, lay[weight], lay['Wt'],
                                                G[t] if G is not None else None, lay['bias'], work,
                                                planes, relu=True, out=bufs[t & 1] if out is None else out[t])
            bufs[t & 1] = state
        return X0, state, work

    # -- the pause after a refused image, and the words that decide it (`_large_sparse_state`, `_large_dense_state`) --
    @staticmethod
    def _paused(st):
        """True while the pause after a refusal lasts: one call fewer to go."""
        if st.get('skip', 0) > 0:
            st['skip'] -= 1
            return True
        return False

    def _pause_after(self, st, refused):
        """A refusal pauses the question for `large_sparse_backoff` calls on this device, twice as many after every
        further refusal in a row (up to 32 x); an accepted image ends the row."""
        st['streak'] = min(st.get('streak', 0) + 1, 6) if refused else 0
        if refused:
            st['skip'] = self.large_sparse_backoff << (st['streak'] - 1)

    @staticmethod
    def _words_behind_event(st, *words):
        """Start the copy of the device int32 `words` into the state's pinned buffer behind an event -> read(),
        which waits for that event alone (not for launches issued since) and returns the words as one list."""
        n = sum(w.numel() for w in words)
        host = st.get('host')
        if host is None or host.numel() != n:
            host = st['host'] = torch.zeros((n,), dtype=torch.int32).pin_memory()
        at = 0
        for w in words:
            host[at:at + w.numel()].copy_(w.reshape(-1), non_blocking=True)
            at += w.numel()
        ev = torch.cuda.Event()
        ev.record()

        def read():
            ev.synchronize()
            return host.tolist()
        return read

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
        cache = self._plan_large()
        G = None
        if S > 0:
            G = ops.spectral_gains(D, self.long_diffusion_dist, self.num_layer, cache['mlp_pack'])
        state = self._large_sparse_layers(node_feat, Lf, Vf, G, planes)
        if state is None and isinstance(Lf, ops.SparseLaplacian):
            # (a raised image flag, a pause after one, or the sparse layers switched off)
            Lf = self._densify(Lf, 'the sparse conv layers do not serve this batch')
        for attempt in range(2 if state is None else 0):
            Lb, Vb, classes, verify = self._large_pack(Lf, Vf, planes)
            plan = self._plan_large(planes, classes)
            work = ops.large_work_buffers(Lb)
            state = input_state(self, node_feat, as_float=True).contiguous()
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
            return ops.large_head(state, mask, *self._plan_head(cache))
        return masked_readout(self, state, mask)


class _SparseOperators:
    """What `_LargeSparseFusedFunction` reads of a batch: R symmetric operators as sparse images with their fp32
    values, serving `channels` weight channels — R = 1 (`img` a LargeSparseImage: every channel is that operator)
    or R = channels (`img` a LargeSparseImages: one operator per channel).
      an untyped SparseLaplacian           R = 1, channels = 2
      a typed one                          R = channels = 3 .. 8
      a dense L, `_dense_operators` 'one'  R = 1: the image riding on the tensor
      ... 'each' (`each=True`)             R = channels: the images riding on it
    n_nodes is the edge lists'; None for a dense L: the mask need not be a prefix, and rows outside it get an
    exactly zero gradient from the masked readout (from then on they receive gradient only through L and V, as
    autograd computes it)."""
    __slots__ = ('B', 'N', 'channels', 'R', 'img', 'n_nodes')

    def __init__(self, L, each=False):
        self.B, self.N, self.channels = L.shape[0], L.shape[1], L.shape[3]
        if isinstance(L, ops.SparseLaplacian):
            self.img, self.n_nodes = (L.image if L.images is None else L.images), L.n_nodes
        else:
            self.img, self.n_nodes = (ops.attached_sparse_images(L) if each else ops.attached_sparse_image(L)), None
        assert self.img is not None and self.img.values is not None
        self.R = self.channels if isinstance(self.img, ops.LargeSparseImages) else 1


class _LargeSparseFusedFunction(torch.autograd.Function):
    """Training a batch of graphs beyond the dense kernels' sizes whose operators are symmetric and given as
    sparse images (`_SparseOperators`: an edge-list batch, a typed one, or a dense collated L with its image(s))
    through the HIP kernels, with no dense L (DESIGN.md §4.9c - e).

    forward: spectral gains + `_sparse_conv_layers` — the launches of the inference route, so the score is that
    route's bit for bit — each layer into its own slice of ONE [num_layer, B, N, 128] buffer, then the readout.
    backward, last layer first: lnz_large_grad_project (dP, db, A = V^T dP); dZ_c = L_c dP = L_c^T dP into the
    forward's feature buffer — R = 1: the forward's gather on dP onto zeros, R > 1:
    lnz_large_sparse_conv_split_f32, R results from one source —; lnz_large_grad_spectral (dG, Q, dY; Y = V^T X
    recomputed by one library GEMM); library GEMMs for dWn_c = dZ_c^T X (R = 1: the one block serves every
    channel) and dW_s = A^T Q_s; dX = sum_c dZ_c Wn_c + V dY by lnz_large_grad_input (R = 1: Wn the channels'
    blocks summed) or lnz_large_grad_input_channels; the head by autograd on the stored last state;
    lnz_spectral_mlp_grad; lnz_embedding_grad.  Inputs L, D, V, mask, node features are data: no gradient."""

    @staticmethod
    def forward(ctx, module, node_feat, L, D, V, mask, *params):
        m, op = module, L
        S = m.num_scale_long
        Vf = V.float().contiguous()
        cache = m._plan_large()
        G = None
        if S > 0:
            G = ops.spectral_gains(D, m.long_diffusion_dist, m.num_layer, cache['mlp_pack'])
        Xs = torch.empty((m.num_layer, op.B, op.N, 128), dtype=torch.float32, device=V.device)
        X0, state, work = m._sparse_conv_layers(node_feat, op.img, op.channels, Vf, G, m.large_split_planes, out=Xs)
        mask_u8 = mask.to(torch.uint8).contiguous()
        if m.large_head_kernel and m.output_dim <= 16:
            score = ops.large_head(state, mask_u8, *m._plan_head(cache))
        else:
            score = masked_readout(m, state, mask)
        # (the [R, B, N, 128] feature buffer of the forward is the backward's dZ: no allocation of its own)
        ctx.module, ctx.op, ctx.has_gains, ctx.dZ = m, op, G is not None, work[0].view(op.R, op.B, op.N, 128)
        ctx.save_for_backward(node_feat, X0, D, Vf, mask_u8, op.n_nodes, Xs, *([G] if G is not None else []))
        return score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_score):
        m, op = ctx.module, ctx.op
        node_feat, X0, D, V, mask_u8, n_nodes, Xs = ctx.saved_tensors[:7]
        G = ctx.saved_tensors[7] if ctx.has_gains else None
        Lnum, B, N, _ = Xs.shape
        K, S, C, R = V.shape[2], m.num_scale_long, op.channels, op.R
        # (the buffer goes with this backward, not with the graph, which a caller's `loss` keeps alive into the
        # next step; a second backward over a retained graph takes a buffer of its own)
        dZ, ctx.dZ = ctx.dZ, None
        if dZ is None:
            dZ = torch.empty((R, B, N, 128), dtype=torch.float32, device=Xs.device)
        grads = {}
        # ---- head (model/lanczos_net.py:185-194): autograd on the stored last state
        Whead, bhead = m._plan_head(m._plan_large())
        with torch.enable_grad():
            XL = Xs[-1].detach().requires_grad_(True)
            Wh = Whead.detach().requires_grad_(True)
            bh = bhead.detach().requires_grad_(True)
            dXL, dWh, dbh = torch.autograd.grad(masked_readout(m, XL, mask_u8, stacked=(Wh, bh)),
                                                [XL, Wh, bh], grad_score.contiguous())
        scatter_head_grads(m, grads, dWh, dbh)
        g = dXL.contiguous()            # dX' of the layer at hand; lnz_large_grad_project masks it in place
        Vt = V.transpose(1, 2)
        dGs = []
        for t in range(Lnum - 1, -1, -1):
            X = X0 if t == 0 else Xs[t - 1]
            d = m.input_dim if t == 0 else 128
            W = m.filter[t].weight.detach().float().contiguous()      # [128, (S + C) d]
            A, dbg = ops.large_grad_project(g, Xs[t], V, n_nodes)     # g is dP from here on
            if R == 1:
                dZ.zero_()
                with torch.cuda.device(dZ.device):
                    ops._abi().large_sparse_conv_f32(op.img.entries, op.img.values, op.img.counts, op.img.cap, g,
                                                     B, N, 0, dZ[0])
            else:
                ops.large_sparse_conv_split(op.img, g, out=dZ)        # dZ[c] = L_c dP
            Xr = X.view(B * N, X.shape[2])
            # (R = 1: the C channels are ONE operator, its block is every channel's)
            blocks = [_tn_split_k(dZ[c].view(B * N, 128), Xr)[:, :d] for c in range(R)] * (C // R)
            dY = None
            if S > 0:
                Y = torch.bmm(Vt, X)                                  # V^T X  [B, K, ldx]
                dG, Q, dY = ops.large_grad_spectral(A, Y, G[t], W, d, want_dgains=m._has_mlp())
                dWl = A.view(B * K, 128).t() @ Q.view(B * K, S * d)
                blocks = list(dWl.view(128, S, d).unbind(1)) + blocks
                if dG is not None:
                    dGs.append(dG)
            grads[id(m.filter[t].weight)] = torch.stack(blocks, dim=1).reshape(128, -1)
            grads[id(m.filter[t].bias)] = dbg.sum(dim=0)
            if t > 0 or not m.general:
                Wv = W.view(128, S + C, d)
                if R == 1:
                    Wn = Wv[:, S]
                    for c in range(1, C):
                        Wn = Wn + Wv[:, S + c]
                    Wn = torch.nn.functional.pad(Wn, (0, 128 - d)).contiguous()
                    ops.large_grad_input(dZ[0], Wn, V if S > 0 else None, dY, d, out=g)
                else:
                    Wn = torch.nn.functional.pad(Wv[:, S:].permute(1, 0, 2), (0, 128 - d)).contiguous()
                    ops.large_grad_input_channels(dZ, Wn, V if S > 0 else None, dY, d, out=g)
        # ---- spectral filter MLPs from dG [L, B K, S]
        if dGs:
            _spectral_mlp_param_grads(m, grads, D, torch.stack(dGs[::-1]).view(Lnum, B * K, S))
        # ---- embedding rows
        if not m.general:
            grads[id(m.embedding.weight)] = embedding_grad(m, node_feat, g, N, m.input_dim)
        return param_grad_tuple(m, grads, 6)


