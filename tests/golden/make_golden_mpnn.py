"""Generates tests/golden/mpnn.npz by IMPORTING the reference (run in the build container): the
reference MPNN (model/mpnn.py, model/set2set.py) on the cases of tests/mpnn_mirror.py — (a) the shape of
config/qm8_mpnn.yaml (D 128, 7 channels, 7 steps, msg_func MLP, 'avg', 10 Set2Vec steps) and (b) the same
with 'sum' and 3 steps on the collate_batch fixture, (c) B 3, N 5, C 2, D 32, 2 steps, 3 Set2Vec steps,
(d) B 2, N 32, C 7, D 128 with mask=None, (e) msg_func 'embedding', D 32 and (f) B 1, 'avg' on batches
drawn by mpnn_mirror.draw_inputs (seeds 71 .. 74) — with the weights of mpnn_mirror.draw_params (seeds
61 .. 66).  The reference overwrites its L argument (model/mpnn.py:125), so every call gets a clone; the
mask goes in as .bool().  Set2Vec allocates its zeros in the default dtype, so the float64 copy runs
under torch.set_default_dtype(torch.float64).  Per case: the scores of the float32 module and of its
`.double()` copy, their distance e_ref = max|s32 - s64| / max|s64|, the float32 training loss, the
parameter names and shapes and per-parameter gradient sums and abs-sums.  No weights are stored.
    python tests/golden/make_golden_mpnn.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
from tests.golden.make_golden import import_reference  # noqa: E402
import mpnn_mirror as G  # noqa: E402


def main():
  ref_model, _, _ = import_reference()
  torch.set_num_threads(4)
  out = {}
  for name in sorted(G.CASES):
    cfg, batch, use_mask = G.case_inputs(name)
    net = ref_model.MPNN(cfg)
    P = G.draw_params([(k, p.shape) for k, p in net.named_parameters()], G.PARAM_SEED[name])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    nf, L = torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L'])
    mask = torch.from_numpy(batch['node_mask']).bool() if use_mask else None
    label = torch.from_numpy(batch['label'])
    net.eval()
    with torch.no_grad():
      s32 = net(nf, L.clone(), mask=mask).numpy()
    net.train()
    score, loss = net(nf, L.clone(), label=label, mask=mask)
    loss.backward()
    named = list(net.named_parameters())
    assert all(p.grad is not None for _, p in named)
    gsum = np.array([float(p.grad.double().sum()) for _, p in named])
    gabs = np.array([float(p.grad.double().abs().sum()) for _, p in named])
    net.zero_grad()
    net = net.double().eval()
    torch.set_default_dtype(torch.float64)
    try:
      with torch.no_grad():
        s64 = net(nf, L.clone().double(), mask=mask).numpy()
    finally:
      torch.set_default_dtype(torch.float32)
    assert s64.dtype == np.float64
    assert np.array_equal(L.numpy(), batch['L'])
    e_ref = float(np.abs(s32.astype(np.float64) - s64).max() / np.abs(s64).max())
    out[name + '_score32'] = s32
    out[name + '_score64'] = s64
    out[name + '_e_ref'] = e_ref
    out[name + '_loss'] = float(loss.detach())
    out[name + '_names'] = np.array([k for k, _ in named])
    out[name + '_shapes'] = np.array(['x'.join(str(d) for d in p.shape) for _, p in named])
    out[name + '_gsum'] = gsum
    out[name + '_gabs'] = gabs
    print('case %s: e_ref %.2e, loss %.6f, %d parameters' % (name, e_ref, float(loss.detach()), len(named)))
  np.savez_compressed(os.path.join(HERE, 'mpnn.npz'), **out)
  print('mpnn.npz', os.path.getsize(os.path.join(HERE, 'mpnn.npz')), 'B')


if __name__ == '__main__':
  main()
