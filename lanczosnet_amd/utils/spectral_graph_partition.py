"""The partition Laplacians of GPNN (reference `utils/spectral_graph_partition.py:35-50`), batched, on the
tensors' own device.

`get_L_cluster_cut(L_simple, node_label)` is the reference function for a whole padded batch: strip the
diagonal of the simple graph's Laplacian, binarise what is left, split the edges by whether their two ends
carry the same label, and take the L4 Laplacian `D^-1/2 (I + A) D^-1/2` of each part.  The padded rows behave
as the reference's do on the padded matrix: an isolated node's L4 row is 1 on the diagonal.

`spectral_clustering` (`eigsh` + a seeded `KMeans`, :10-32) is NOT ported: the labels are the caller's.
"""
import torch

__all__ = ['get_L_cluster_cut']


def _l4(adj):
    """D^-1/2 (I + A) D^-1/2 of adj [B, N, N] (float64): every row sum is >= 1, nothing to guard."""
    A = adj + torch.eye(adj.shape[1], dtype=adj.dtype, device=adj.device)
    r = A.sum(dim=2).pow(-0.5)
    return r.unsqueeze(2) * A * r.unsqueeze(1)


def get_L_cluster_cut(L_simple, node_label):
    """L_simple [B, N, N] (any float dtype; only its off-diagonal `!= 0` pattern is read, it is not written),
    node_label [B, N] integer -> (L_cluster, L_cut) [B, N, N] float32, computed in float64 and rounded once."""
    if L_simple.dim() != 3 or L_simple.shape[1] != L_simple.shape[2] or tuple(node_label.shape) != tuple(L_simple.shape[:2]):
        raise ValueError('get_L_cluster_cut: L_simple [B, N, N] and node_label [B, N] expected, got %s and %s'
                         % (tuple(L_simple.shape), tuple(node_label.shape)))
    N = L_simple.shape[1]
    off = ~torch.eye(N, dtype=torch.bool, device=L_simple.device)
    adj = ((L_simple != 0) & off).to(torch.float64)
    same = (node_label.unsqueeze(2) == node_label.unsqueeze(1)).to(torch.float64)
    adj_cluster = adj * same
    adj_cut = adj - adj_cluster
    return _l4(adj_cluster).float(), _l4(adj_cut).float()
