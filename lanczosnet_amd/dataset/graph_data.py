"""Dataset surface of the reference's synthetic-graph experiment (`dataset/graph_data.py:11-293`,
`config/graph_lanczos_net.yaml`, pickles written by `dataset/get_graph_data.py:51-92`).

Graphs of 20..100 nodes with float node embeddings `X [n, node_emb_dim]`, ONE edge type and a
graph-level label `Y [1, graph_emb_dim]`; the model is `LanczosNetGeneral`.  The two entry points of
`dataset/qm8.py`, and one more for large graphs:

* `collate_graph_preprocessed(items, num_eigs)` — items are the reference's per-graph pickle dicts
  (node_feat, L_multi, L_simple_4, D_simple, V_simple, label); the host-side padding of the
  reference's default branch (`dataset/graph_data.py:222-291`);
* `collate_graph_adjacency(items, num_eigs, device)` — items carry only the RAW graph (`adjs [n,n,E]`,
  `node_feat [n,D]`, `label [1,P]`); the Laplacians (`lnz_laplacian_l4`, replacing
  get_graph_data.py:61-72) and the Ritz pairs (`lnz_lanczos_ritz`, workgroup-per-graph kernel for
  N > 32, replacing utils/data_helper.py:197-223 and the pad / cut of graph_data.py:262-287) are
  computed ON THE DEVICE.  Batches padded beyond 192 nodes (BASELINE config 5: 2048) get the
  pairs of the K-step recurrence instead (`lnz_lanczos_ritz_kstep`: the reference's
  use_eigen_decomp=False branch, utils/data_helper.py:205-208; announced by a UserWarning).

* `collate_graph_edges(items, num_eigs, device)` — the same batch from EDGE LISTS (`edges [m,2]`): no
  array of N x N elements on the host or the device, `L` an `ops.SparseLaplacian` (large graphs of one
  edge type, 192 < N <= 16384; csrc/edge_image.hip).

`GraphData(config, split)` is the class the runner instantiates with
`eval(config.dataset.loader_name)(config, split=...)` (runner/graph_runner.py:38-40).

Returned keys (reference dict): node_feat [B,N,D] float32, node_mask [B,N] uint8, label [B,P] float32,
L [B,N,N,E+1] float32, D [B,K], V [B,N,K].
"""
import numpy as np
import torch


def _pad_common(items):
    sizes = [int(np.asarray(it['node_feat']).shape[0]) for it in items]
    B, N = len(items), max(sizes)
    dim = int(np.asarray(items[0]['node_feat']).shape[1])
    node_feat = np.zeros((B, N, dim), dtype=np.float32)
    mask = np.zeros((B, N), dtype=np.uint8)
    for b, (it, n) in enumerate(zip(items, sizes)):
        node_feat[b, :n] = np.asarray(it['node_feat'])   # float64 pickles -> .float() (:68-75)
        mask[b, :n] = 1
    label = np.concatenate([np.asarray(it['label'], dtype=np.float64).reshape(1, -1)
                            for it in items], axis=0).astype(np.float32)
    return sizes, B, N, node_feat, mask, label


def collate_graph_preprocessed(items, num_eigs, simple_key='L_simple_4', negate_simple=False):
    """Host-side restatement of the reference's default branch (dataset/graph_data.py:222-291)."""
    sizes, B, N, node_feat, mask, label = _pad_common(items)
    E = np.asarray(items[0]['L_multi']).shape[2]
    L = np.zeros((B, N, N, E + 1), dtype=np.float32)
    for b, (it, n) in enumerate(zip(items, sizes)):
        ls = np.asarray(it[simple_key])
        L[b, :n, :n, 0] = -ls if negate_simple else ls
        L[b, :n, :n, 1:] = it['L_multi']
    out = dict(node_feat=torch.from_numpy(node_feat), node_mask=torch.from_numpy(mask),
               label=torch.from_numpy(label), L=torch.from_numpy(L))
    if num_eigs:
        D = np.zeros((B, num_eigs), dtype=np.float32)
        V = np.zeros((B, N, num_eigs), dtype=np.float32)
        for b, (it, n) in enumerate(zip(items, sizes)):
            d, v = np.asarray(it['D_simple']), np.asarray(it['V_simple'])
            kk = min(num_eigs, d.shape[0])
            D[b, :kk] = d[:kk]
            V[b, :n, :kk] = v[:, :kk]
        out['D'], out['V'] = torch.from_numpy(D), torch.from_numpy(V)
    return out


def collate_graph_adjacency(items, num_eigs, device='cuda', model_name='LanczosNetGeneral',
                            eigs_method='auto', lanczos_steps=None):
    """Raw graphs in, device-resident batch out (Laplacians and Ritz pairs by the HIP kernels).
    model_name picks the simple-graph channel like the reference's collate (graph_data.py:247-260):
    L4 by default, the asymmetric diffusion map L7 for DCNN, MINUS the symmetric one (L6, alpha =
    0.5) for ChebyNet — the bond-type channels are L4 in every branch (get_graph_data.py:61-72).
    eigs_method: 'auto', or 'full' for the pairs of the full decomposition at every size
    (ops.sym_eigh_topk, the offline `eigh` of get_graph_data.py:63-68); no sparse image is then
    left on L (the large-graph forward builds its own).
    lanczos_steps: M >= num_eigs steps of the K-step recurrence for graphs beyond 192 nodes (None =
    num_eigs); beyond 2048 nodes or 64 steps the pairs come from the wide K-step entry, which
    leaves no sparse image on L either."""
    from .. import ops
    if eigs_method not in ('auto', 'full'):
        raise ValueError("collate_graph_adjacency: eigs_method is 'auto' or 'full', got %r" % (eigs_method,))
    sizes, B, N, node_feat, mask, label = _pad_common(items)
    E = np.asarray(items[0]['adjs']).shape[2]
    adjs = np.zeros((B, N, N, E), dtype=np.float32)
    for b, (it, n) in enumerate(zip(items, sizes)):
        adjs[b, :n, :n, :] = it['adjs']
    dev = torch.device(device)
    n_nodes = torch.tensor(sizes, dtype=torch.int32, device=dev)
    adjs_d = torch.from_numpy(adjs).to(dev)
    L = ops.laplacian_l4(adjs_d, n_nodes)
    out = dict(node_feat=torch.from_numpy(node_feat).to(dev),
               node_mask=torch.from_numpy(mask).to(dev), label=torch.from_numpy(label).to(dev),
               n_nodes=n_nodes)
    if num_eigs:
        # (the Ritz pairs are those of the L4 simple graph in every branch, graph_data.py:262-287)
        # (beyond 192 nodes the same pass over L also leaves the conv's sparse image riding on it)
        out['D'], out['V'] = ops.lanczos_ritz_collated(L, n_nodes, num_eigs, method=eigs_method,
                                                       lanczos_steps=lanczos_steps)
    if model_name == 'DCNN':
        L[:, :, :, 0] = ops.laplacian(adjs_d, n_nodes, 'L7')[:, :, :, 0]
    elif model_name == 'ChebyNet':
        L[:, :, :, 0] = -ops.laplacian(adjs_d, n_nodes, 'L6')[:, :, :, 0]
    out['L'] = L
    return out


def collate_graph_edges(items, num_eigs, device='cuda', lanczos_steps=None, num_edge_type=1):
    """Raw graphs as EDGE LISTS in, device-resident batch out with no array of N x N elements on the
    host or the device: items carry `edges [m,2]` (integer local node ids, each undirected edge once,
    either endpoint order; unweighted simple graphs, ONE edge type — the reference's graph
    configuration), `node_feat [n,D]`, `label [1,P]`.  Returns the keys of collate_graph_adjacency;
    `L` is an `ops.SparseLaplacian` (the model's forward takes it; `.to_dense()` is the [B,N,N,2]
    tensor), D / V the Ritz pairs of the K-step recurrence on its image (ops.lanczos_ritz_edges,
    replacing utils/data_helper.py:92-116,155-156,205-223 and dataset/get_graph_data.py:61-72).
    Batches padded to N <= 192 nodes are outside the K-step territory: they are densified and the
    result is collate_graph_adjacency's for the same graphs.  ValueError for a malformed argument
    (here) or a graph that is not a simple graph (found on the device).
    num_edge_type = E >= 2 (at most 7): every item also carries `edge_type [m]`, integers in [0, E), one
    type per edge (a node pair carries at most one edge; pairs with two bond types stay with
    collate_graph_adjacency).  `L` then has E + 1 channels (channel 0 the simple graph, channel 1 + e
    edge type e alone, dataset/get_graph_data.py:60-72) and carries one sparse image per channel; D / V
    are channel 0's.  num_edge_type = 1: an `edge_type` key, if present, must be all zeros."""
    num_edge_type = int(num_edge_type)
    if not 1 <= num_edge_type <= 7:
        raise ValueError('collate_graph_edges: num_edge_type=%d: 1 .. 7 edge types are served' % num_edge_type)
    if not isinstance(items, (list, tuple)) or len(items) == 0:
        raise ValueError('collate_graph_edges: a non-empty list of items expected')
    num_eigs = int(num_eigs or 0)
    if num_eigs < 0:
        raise ValueError('collate_graph_edges: num_eigs=%d' % num_eigs)
    if lanczos_steps is not None and int(lanczos_steps) < num_eigs:
        raise ValueError('collate_graph_edges: lanczos_steps=%d < num_eigs=%d' % (lanczos_steps, num_eigs))
    lists, types = [], []
    for b, it in enumerate(items):
        for key in ('edges', 'node_feat', 'label'):
            if key not in it:
                raise ValueError('collate_graph_edges: item %d has no %r' % (b, key))
        e = np.asarray(it['edges'])
        if e.size == 0:
            e = np.zeros((0, 2), dtype=np.int32)
        if e.ndim != 2 or e.shape[1] != 2:
            raise ValueError('collate_graph_edges: item %d: edges of shape %s, [m, 2] expected' % (b, e.shape))
        if not np.issubdtype(e.dtype, np.integer):
            raise ValueError('collate_graph_edges: item %d: edges of dtype %s, integer node ids expected'
                             % (b, e.dtype))
        if np.asarray(it['node_feat']).ndim != 2:
            raise ValueError('collate_graph_edges: item %d: node_feat [n, D] expected' % b)
        if e.size and (e.min() < -2**31 or e.max() >= 2**31):
            raise ValueError('collate_graph_edges: item %d: node ids beyond int32' % b)
        lists.append(e.astype(np.int32))
        if num_edge_type > 1 or 'edge_type' in it:
            if 'edge_type' not in it:
                raise ValueError('collate_graph_edges: item %d has no %r (num_edge_type=%d)'
                                 % (b, 'edge_type', num_edge_type))
            ty = np.asarray(it['edge_type'])
            if ty.size == 0:
                ty = np.zeros((0,), dtype=np.int32)
            if ty.ndim != 1 or ty.shape[0] != lists[-1].shape[0]:
                raise ValueError('collate_graph_edges: item %d: edge_type of shape %s, [%d] expected'
                                 % (b, ty.shape, lists[-1].shape[0]))
            if not np.issubdtype(ty.dtype, np.integer):
                raise ValueError('collate_graph_edges: item %d: edge_type of dtype %s, integers expected'
                                 % (b, ty.dtype))
            if ty.size and (ty.min() < 0 or ty.max() >= num_edge_type):
                raise ValueError('collate_graph_edges: item %d: an edge type outside [0, %d)' % (b, num_edge_type))
            types.append(ty.astype(np.int32))
    from .. import ops
    sizes, B, N, node_feat, mask, label = _pad_common(items)
    if N > ops.KSTEP_WIDE_MAX_N:
        raise ValueError('collate_graph_edges: %d nodes: graphs of up to %d nodes are served'
                         % (N, ops.KSTEP_WIDE_MAX_N))
    if N <= ops.RITZ_FULL_MAX_N:
        dense = []
        for it, e, n in zip(items, lists, sizes):
            if e.size and (e.min() < 0 or e.max() >= n or (e[:, 0] == e[:, 1]).any()):
                raise ValueError('collate_graph_edges: an endpoint outside the graph or a self loop')
            a = np.zeros((n, n, num_edge_type), dtype=np.float32)
            ty = types[len(dense)] if num_edge_type > 1 else 0
            a[e[:, 0], e[:, 1], ty] = 1.0
            a[e[:, 1], e[:, 0], ty] = 1.0
            dense.append(dict(adjs=a, node_feat=it['node_feat'], label=it['label']))
        return collate_graph_adjacency(dense, num_eigs, device=device, lanczos_steps=lanczos_steps)
    dev = torch.device(device)
    edge_off = np.zeros((B + 1,), dtype=np.int64)
    np.cumsum([e.shape[0] for e in lists], out=edge_off[1:])
    edges = torch.from_numpy(np.concatenate(lists, axis=0)).to(dev)
    edge_off = torch.from_numpy(edge_off).to(dev)
    n_nodes = torch.tensor(sizes, dtype=torch.int32, device=dev)
    out = dict(node_feat=torch.from_numpy(node_feat).to(dev), node_mask=torch.from_numpy(mask).to(dev),
               label=torch.from_numpy(label).to(dev), n_nodes=n_nodes)
    typed = {}
    if num_edge_type > 1:
        typed = dict(edge_type=torch.from_numpy(np.concatenate(types, axis=0)).to(dev), num_edge_type=num_edge_type)
    if num_eigs:
        out['D'], out['V'], out['L'] = ops.lanczos_ritz_edges(edges, edge_off, n_nodes, N, num_eigs,
                                                              lanczos_steps=lanczos_steps, **typed)
    else:
        out['L'] = ops.sparse_laplacian_from_edges(edges, edge_off, n_nodes, N, **typed)
    return out


class GraphData(object):
    """Drop-in for reference `dataset/graph_data.py:11-293`: globs `synthetic_{split}_*.p` under
    `config.dataset.data_path`, one pickle per graph, `collate_fn` pads a list of them to the batch
    maximum.  The file lists are SORTED (the reference keeps `glob.glob`'s directory order,
    :28-33).  Branches built: the default one (LanczosNetGeneral, GCN, ... with `L_simple_4`),
    DCNN (`L_simple_7`) and ChebyNet (`-L_simple_6`), :247-260; GPNN / GraphSAGE / GAT build
    partition, neighbour-sampling and attention-bias tensors for models outside this path."""

    def __init__(self, config, split='train'):
        import glob
        import os
        assert split in ('train', 'dev', 'test'), 'no such split'
        self.split, self.config = split, config
        self.seed = config.seed
        self.data_path = config.dataset.data_path
        self.num_edgetype = config.dataset.num_edge_type
        self.model_name = config.model.name
        self.use_eigs = hasattr(config.model, 'num_eig_vec')
        self.num_eigs = config.model.num_eig_vec if self.use_eigs else 0
        self.files = sorted(glob.glob(os.path.join(self.data_path, 'synthetic_%s_*.p' % split)))

    def __len__(self):
        return len(self.files)

    def __getitem__(self, index):
        import pickle
        with open(self.files[index], 'rb') as f:
            return pickle.load(f)

    def collate_fn(self, batch):
        assert isinstance(batch, list)
        if self.model_name in ('GPNN', 'GraphSAGE', 'GAT'):
            raise NotImplementedError('GraphData mirrors the default collate branch '
                                      '(LanczosNetGeneral, GCN, DCNN, ChebyNet); got %s'
                                      % self.model_name)
        key = {'DCNN': 'L_simple_7', 'ChebyNet': 'L_simple_6'}.get(self.model_name, 'L_simple_4')
        return collate_graph_preprocessed(batch, self.num_eigs if self.use_eigs else 0,
                                          simple_key=key,
                                          negate_simple=self.model_name == 'ChebyNet')
