"""Generates tests/golden/gpnn.npz by IMPORTING the reference (run in the build container, on the CPU): the
reference GPNN (model/gpnn.py) on the cases of tests/gpnn_mirror.py — (a) the shape of config/qm8_gpnn.yaml
(D 128, 7 channels, 10 outer steps, counts (1, 1), 'avg') and (b) the same with 'sum', 3 steps and counts
(2, 0) on the collate_batch fixture with the node labels of the reference's own spectral_clustering (run,
as dataset/qm8.py:126-130 runs it, on the padded simple-graph Laplacian with num_partition = 3), (c) B 3, N 5,
C 2, D 32, 2 steps, (d) B 2, N 32, C 7, D 128, 4 steps with mask=None and (e) update_func 'RNN', D 32, 2
steps on batches drawn by gpnn_mirror.draw_inputs (seeds 91 .. 93) — with the weights of
gpnn_mirror.draw_params (seeds 61 .. 65).  L_cluster / L_cut of every case come from the reference's
get_L_cluster_cut and must equal gpnn_mirror.partition_laplacians' to the bit (asserted here).  That function
uses `np.float`, which numpy 2 removed: the alias is supplied in this process, the reference is not patched.
The reference overwrites its L argument (model/gpnn.py:158), so every call gets a clone; the mask goes in as
.bool().  Per case: the scores of the float32 module and of its `.double()` copy, their distance e_ref =
max|s32 - s64| / max|s64|, the float32 training loss, the parameter names and shapes and per-parameter
gradient sums and abs-sums.  Beside them: the collate fixture's node labels, and for the partition helper the
labels and the reference's L_cluster / L_cut of case (c)'s batch.  No weights are stored.
    python tests/golden/make_golden_gpnn.py"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
from tests.golden.make_golden import import_reference  # noqa: E402
import gpnn_mirror as M  # noqa: E402


def main():
  if not hasattr(np, 'float'):
    np.float = float   # utils/spectral_graph_partition.py:43, in this process only
  ref_model, _, _ = import_reference()
  import utils.spectral_graph_partition as ref_part
  torch.set_num_threads(4)
  out = {}

  c = np.load(os.path.join(HERE, 'collate_batch.npz'))
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    labels = np.stack([ref_part.spectral_clustering(c['L'][b, :, :, 0].astype(np.float64), M.NUM_PARTITION)
                       for b in range(c['L'].shape[0])]).astype(np.int64)
  out['collate_node_label'] = labels.astype(np.int8)

  for name in sorted(M.CASES):
    cfg, batch, use_mask = M.case_inputs(name, collate_labels=labels)
    pairs = [ref_part.get_L_cluster_cut(batch['L'][b, :, :, 0].astype(np.float64), batch['node_label'][b])
             for b in range(batch['L'].shape[0])]
    Lcl = torch.from_numpy(np.stack([p[0] for p in pairs])).float()
    Lct = torch.from_numpy(np.stack([p[1] for p in pairs])).float()
    assert np.array_equal(Lcl.numpy(), batch['L_cluster']) and np.array_equal(Lct.numpy(), batch['L_cut'])
    if name == 'c':
      out['part_node_label'] = batch['node_label'].astype(np.int8)
      out['part_L_cluster'] = np.stack([p[0] for p in pairs])
      out['part_L_cut'] = np.stack([p[1] for p in pairs])
    net = ref_model.GPNN(cfg)
    P = M.draw_params([(k, p.shape) for k, p in net.named_parameters()], M.PARAM_SEED[name])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    nf, L = torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L'])
    mask = torch.from_numpy(batch['node_mask']).bool() if use_mask else None
    label = torch.from_numpy(batch['label'])
    net.eval()
    with torch.no_grad():
      s32 = net(nf, L.clone(), Lcl, Lct, mask=mask).numpy()
    net.train()
    score, loss = net(nf, L.clone(), Lcl, Lct, label=label, mask=mask)
    loss.backward()
    named = list(net.named_parameters())
    # (b): num_prop_cut = 0 leaves nothing without a gradient — the partition cell serves the cluster steps
    assert all(p.grad is not None for _, p in named)
    gsum = np.array([float(p.grad.double().sum()) for _, p in named])
    gabs = np.array([float(p.grad.double().abs().sum()) for _, p in named])
    net.zero_grad()
    net = net.double().eval()
    with torch.no_grad():
      s64 = net(nf, L.clone().double(), Lcl.double(), Lct.double(), mask=mask).numpy()
    assert np.array_equal(L.numpy(), batch['L'])
    assert np.array_equal(Lcl.numpy(), batch['L_cluster']) and np.array_equal(Lct.numpy(), batch['L_cut'])
    e_ref = float(np.abs(s32.astype(np.float64) - s64).max() / np.abs(s64).max())
    out[name + '_score32'] = s32
    out[name + '_score64'] = s64
    out[name + '_e_ref'] = e_ref
    out[name + '_loss'] = float(loss.detach())
    out[name + '_names'] = np.array([k for k, _ in named])
    out[name + '_shapes'] = np.array(['x'.join(str(d) for d in p.shape) for _, p in named])
    out[name + '_gsum'] = gsum
    out[name + '_gabs'] = gabs
    print('case %s: e_ref %.2e, loss %.6f, %d parameters' % (name, e_ref, out[name + '_loss'], len(named)))
  np.savez_compressed(os.path.join(HERE, 'gpnn.npz'), **out)
  print('gpnn.npz', os.path.getsize(os.path.join(HERE, 'gpnn.npz')), 'B')


if __name__ == '__main__':
  main()
