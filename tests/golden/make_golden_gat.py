"""Generates tests/golden/gat.npz by IMPORTING the reference (run in the build container): the
reference GAT (model/gat.py) on the cases of tests/gat_mirror.py — (a) the shape of
config/qm8_gat.yaml (7 layers, 8 heads of width 16, 7 channels) and (b) the same with 3 layers on the
collate_batch fixture, (c) B 3, N 5, C 2, H 2, 2 layers and (d) B 2, N 32, C 7, H 8, 3 layers on
batches drawn by gat_mirror.draw_inputs (seeds 71 and 72) — with the weights of
gat_mirror.draw_params (seeds 41 .. 44).  Per case: the scores of the float32 module and of its
`.double()` copy, their distance e_ref = max|s32 - s64| / max|s64|, the float32 training loss, the
parameter names and per-parameter gradient sums with a flag where `.grad is None` (the bias_*
parameters that the reference's aliased list never reads).  No weights are stored.
    python tests/golden/make_golden_gat.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
from tests.golden.make_golden import import_reference  # noqa: E402
import gat_mirror as G  # noqa: E402


def main():
  ref_model, _, _ = import_reference()
  torch.set_num_threads(4)
  out = {}
  for name in sorted(G.CASES):
    cfg, batch = G.case_inputs(name)
    net = ref_model.GAT(cfg)
    P = G.draw_params([(k, p.shape) for k, p in net.named_parameters()], G.PARAM_SEED[name])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    nf, L = torch.from_numpy(batch['node_feat']), torch.from_numpy(batch['L'])
    mask, label = torch.from_numpy(batch['node_mask']).bool(), torch.from_numpy(batch['label'])
    net.eval()
    with torch.no_grad():
      s32 = net(nf, L, mask=mask).numpy()
    net.train()
    score, loss = net(nf, L, label=label, mask=mask)
    loss.backward()
    named = list(net.named_parameters())
    none = np.array([p.grad is None for _, p in named])
    gsum = np.array([0.0 if p.grad is None else float(p.grad.double().sum()) for _, p in named])
    gabs = np.array([0.0 if p.grad is None else float(p.grad.double().abs().sum()) for _, p in named])
    net.zero_grad()
    net = net.double().eval()
    with torch.no_grad():
      s64 = net(nf, L.double(), mask=mask).numpy()
    e_ref = float(np.abs(s32.astype(np.float64) - s64).max() / np.abs(s64).max())
    out[name + '_score32'] = s32
    out[name + '_score64'] = s64
    out[name + '_e_ref'] = e_ref
    out[name + '_loss'] = float(loss.detach())
    out[name + '_names'] = np.array([k for k, _ in named])
    out[name + '_shapes'] = np.array(['x'.join(str(d) for d in p.shape) for _, p in named])
    out[name + '_gsum'] = gsum
    out[name + '_gabs'] = gabs
    out[name + '_grad_none'] = none
    print('case %s: e_ref %.2e, loss %.6f, %d parameters, %d without a gradient'
          % (name, e_ref, float(loss), len(named), int(none.sum())))
  np.savez_compressed(os.path.join(HERE, 'gat.npz'), **out)
  print('gat.npz', os.path.getsize(os.path.join(HERE, 'gat.npz')), 'B')


if __name__ == '__main__':
  main()
