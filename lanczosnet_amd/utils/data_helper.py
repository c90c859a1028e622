"""Device-side counterparts of reference `utils/data_helper.py` for dense padded batches.

  check_dist                      utils/data_helper.py:9-14   (host logic, same behaviour)
  get_laplacian_l4_batched        :92-116,155-156  -> HIP `lnz_laplacian_l4`
  get_graph_laplacian_eigs_batched :169-258 (use_eigen_decomp=True, is_sym=True branch) +
                                  the pad/cut of dataset/qm8.py:264-291 -> HIP `lnz_lanczos_ritz`;
                                  the use_eigen_decomp=False branch (:205-208) -> `lnz_lanczos_ritz_kstep`;
                                  method='full': the full decomposition at any N -> `lnz_sym_eigh_topk`
"""


def check_dist(dist):
    for dd in dist:
        if not isinstance(dd, int) and dd != 'inf':
            raise ValueError("Non-supported value of diffusion distance")
    return dist


def get_laplacian_l4_batched(adjs, n_nodes):
    """adjs [B,N,N,E] cuda float, n_nodes [B] -> L [B,N,N,E+1] (channel 0 = simple graph)."""
    from .. import ops
    return ops.laplacian_l4(adjs, n_nodes)


def get_graph_laplacian_eigs_batched(L_simple, n_nodes, k, use_eigen_decomp=None, method='auto',
                                     lanczos_steps=None):
    """L_simple [B,N,N] (e.g. `L[..., 0]`), n_nodes [B] -> (D [B,k], V [B,N,k]) ordered by
    descending |eigenvalue| like `np.argsort(-|eigs|, kind='mergesort')` (:218-223).

    use_eigen_decomp (the reference's switch, :173,199-208):
      True   the pairs of the FULL decomposition (`np.linalg.eigh`, :201) — full-length Lanczos +
             tridiagonal eigensolver, `lnz_lanczos_ritz`, graphs of up to 192 nodes; larger ones go
             to the vendor eigensolver on the device (`torch.linalg.eigh`, fp64) with a UserWarning
             (the reference itself calls this branch "computationally heavy for large size adj");
      False  the k-dimensional Krylov method (`eigsh(L, k, which='LM')`, :208) — the k-step
             Lanczos of `lnz_lanczos_ritz_kstep` (N <= 2048, k <= 64) or `lnz_lanczos_ritz_kstep_wide`
             (N <= 16384, k <= 256), ragged batches;
      None   (default) True up to 192 nodes, False beyond, with a UserWarning naming the branch.
    method: 'auto' (the routing above) or 'full': the full decomposition at every N <= 2048 on the
      hand-written eigensolver (`lnz_sym_eigh_topk`), no warning; not with use_eigen_decomp=False.
    lanczos_steps: the dimension M >= k of the Krylov space of the k-step branch (ARPACK's `ncv`);
      None = k, the recurrence of exactly k steps.  Only the k-step branch has it: a ValueError with
      use_eigen_decomp=True or method='full'; the default routing ignores it up to 192 nodes."""
    from .. import ops
    if lanczos_steps is not None:
        lanczos_steps = int(lanczos_steps)
        if lanczos_steps < k:
            raise ValueError("get_graph_laplacian_eigs_batched: lanczos_steps=%d < k=%d: the Krylov space "
                             "holds at least the k pairs kept" % (lanczos_steps, k))
        if method == 'full' or use_eigen_decomp:
            raise ValueError("get_graph_laplacian_eigs_batched: lanczos_steps belongs to the k-step branch "
                             "(use_eigen_decomp=False), not to a full decomposition")
    if method not in ('auto', 'full'):
        raise ValueError("get_graph_laplacian_eigs_batched: method is 'auto' or 'full', got %r" % (method,))
    if method == 'full':
        if use_eigen_decomp is not None and not use_eigen_decomp:
            raise ValueError("get_graph_laplacian_eigs_batched: method='full' is the full decomposition; "
                             "use_eigen_decomp=False asks for the k-step Krylov branch")
        return ops.sym_eigh_topk(L_simple, n_nodes, k)
    N = L_simple.shape[1]
    if use_eigen_decomp is None:
        return ops.lanczos_ritz(L_simple, n_nodes, k, lanczos_steps=lanczos_steps)
    if use_eigen_decomp:
        if N > ops.RITZ_FULL_MAX_N:
            return _full_decomposition_library(L_simple, n_nodes, k)
        return ops.lanczos_ritz(L_simple, n_nodes, k)
    return ops.lanczos_ritz_kstep(L_simple, n_nodes, k if lanczos_steps is None else lanczos_steps, k)


def _full_decomposition_library(L_simple, n_nodes, k):
    """use_eigen_decomp=True beyond the hand-written kernels' 192 nodes: the reference's branch has no
    size limit (`np.linalg.eigh`, :199-201).  Served — with a UserWarning, like every path outside
    the kernels — by the vendor's symmetric eigensolver on the device (`torch.linalg.eigh`, fp64):
    per graph the n_b x n_b block (the reference decomposes the unpadded matrix), |eigenvalue| order
    with the reference's stable tie rule, the kernels' sign convention (largest-magnitude component
    positive), zero padding to [B,k] / [B,N,k] (dataset/graph_data.py:262-287).  Graphs of one size
    share a batched call."""
    import warnings

    import torch
    from .. import ops
    ops._need_cuda(L_simple, n_nodes)
    warnings.warn('get_graph_laplacian_eigs_batched(use_eigen_decomp=True) beyond %d nodes: the full '
                  'decomposition runs on the vendor eigensolver (torch.linalg.eigh, fp64), not on a hand-written '
                  'kernel; use_eigen_decomp=False is the k-step branch (lnz_lanczos_ritz_kstep)'
                  % ops.RITZ_FULL_MAX_N, UserWarning, stacklevel=3)
    B, N = L_simple.shape[0], L_simple.shape[1]
    sizes = [N] * B if n_nodes is None else [int(x) for x in n_nodes.cpu().tolist()]
    D = torch.zeros((B, k), dtype=torch.float32, device=L_simple.device)
    V = torch.zeros((B, N, k), dtype=torch.float32, device=L_simple.device)
    for n in sorted(set(sizes)):
        if n <= 0:
            continue
        idx = torch.tensor([b for b, s in enumerate(sizes) if s == n], device=L_simple.device)
        A = L_simple.index_select(0, idx)[:, :n, :n].to(torch.float64)
        w, U = torch.linalg.eigh(A)                                   # ascending
        # stable sort by descending |w| (np.argsort(-|w|, kind='mergesort'), :218-220)
        order = torch.sort(-w.abs(), dim=1, stable=True).indices
        kk = min(k, n)
        order = order[:, :kk]
        wk = torch.gather(w, 1, order)
        Uk = torch.gather(U, 2, order.unsqueeze(1).expand(-1, n, -1))
        big = Uk.abs().argmax(dim=1, keepdim=True)                    # first of the largest magnitudes
        sg = torch.sign(torch.gather(Uk, 1, big))
        sg = torch.where(sg == 0, torch.ones_like(sg), sg)
        Uk = Uk * sg
        D[idx, :kk] = wk.to(torch.float32)
        Vn = torch.zeros((idx.numel(), N, k), dtype=torch.float32, device=L_simple.device)
        Vn[:, :n, :kk] = Uk.to(torch.float32)
        V[idx] = Vn
    return D, V
