#!/usr/bin/env python
"""GPU: the bits of the baseline kernels that share csrc/ggnn_tile.hpp, as one line per case: the op, the case and
the SHA-256 of every output's bytes.  For a change that must not move a bit (a refactor of the shared tile):
run it on a build of the commit before and on a build of the commit after, on the same machine and ROCm, and
compare the two listings line for line.  A listing on its own proves nothing, and none is kept as a fixture:
digests belong to a compiler version.

The inputs are the GPU tests' own draws and case lists (tests/ on sys.path): ggnn_forward over
test_gpu_ggnn.KERNEL_CASES at both tile heights, ggnn_forward_states over the first three shapes of
test_gpu_ggnn_train's trajectory test, gpnn_forward over test_gpu_gpnn.KERNEL_CASES, mpnn_forward over
test_gpu_mpnn.KERNEL_CASES at both heights, ggnn_backward_step / mpnn_backward_step over their STEP_CASES from
the tests' dS_T (every step's dS and row-space buffers), ggnn_readout_backward over READOUT_CASES.

    python tools/baseline_bits.py > bits.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import mpnn_grad_mirror as MGM  # noqa: E402
import test_gpu_ggnn as TG  # noqa: E402
import test_gpu_ggnn_train as TGT  # noqa: E402
import test_gpu_gpnn as TP  # noqa: E402
import test_gpu_mpnn as TM  # noqa: E402
from lanczosnet_amd import ops  # noqa: E402


def sha(x):
  return hashlib.sha256(x.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def line(op, case, *outputs):
  print(op, ' '.join(str(c) for c in case), *[sha(x) for x in outputs], flush=True)


def device_l(L, lkind):
  """L on the device the way the tests hand it over: plain, one channel expanded, or a slice of a wider tensor"""
  return TP._case_graphs(lkind, L, L[..., 0], L[..., 0])[1][0]


def backward_steps(op, case, S, dST, Ld, W, steps, avg, forward_states, pack, make_buffers, step):
  """the trajectory, then the step kernel for t = steps-1 .. 0: every step's dS and buffers"""
  B, N, D = S.shape
  Wd = [w.cuda() for w in W]
  states = forward_states(S.cuda(), Ld, Wd, steps, avg)
  tr, bufs = pack(Wd[0], Wd[2], Wd[4], Wd[6]), make_buffers(B, N, Ld.shape[3], D, 'cuda')
  dS, spare = dST.cuda(), torch.zeros(B, N, D, device='cuda')
  for t in range(steps - 1, -1, -1):
    spare, _ = step(states[t], dS, Ld, *Wd[:8], transposes=tr, avg=avg, dS=spare, buffers=bufs)
    dS, spare = spare, dS
    line(op, case + ('t', t), dS, *bufs)


def main():
  for case in TG.KERNEL_CASES:
    N, C, D, B, num_prop, agg, mkind, pad, lkind = case
    S, L, W = TG._operands(3000 + N + 7 * C + D, B, N, C, D)
    mask = TG._mask(mkind, B, N, 17 + N)
    for rows in (32, 64):
      score, state, _ = TG._run(S, L, W, mask, num_prop, agg, Ld=device_l(L, lkind), pad=pad, tile_rows=rows)
      line('ggnn_forward', case + (rows,), score, state)
  for case in TGT.test_forward_states_has_the_bits_of_the_forward_and_leaves_the_trajectory.pytestmark[0].args[1][:3]:
    N, C, D, B, steps, tile = case
    S, L, W = TGT.GM.draw_operands(97 + N, B, N, C, D)
    score, states = ops.ggnn_forward_states(S.cuda(), L.cuda(), TGT._mask('ragged', B, N, 6).cuda(),
                                            *[w.cuda() for w in W], steps, avg=True, tile_rows=tile)
    line('ggnn_forward_states', case, score, states)
  for case in TP.KERNEL_CASES:
    N, C, D, B, num_prop, ncl, nct, agg, mkind, pad, lkind = case
    S, L, Lcl, Lct, W = TP._operands(TP._case_seed(N, C, D), B, N, C, D)
    _, graphs = TP._case_graphs(lkind, L, Lcl, Lct)
    score, state, _ = TP._run(S, L, Lcl, Lct, W, TP._mask(mkind, B, N, 17 + N), (num_prop, ncl, nct), agg,
                              graphs=graphs, pad=pad)
    line('gpnn_forward', case, score, state)
  for case in TM.KERNEL_CASES:
    N, C, D, B, num_prop, agg, pad, lkind = case
    S, L, W = TM._operands(4000 + N + 7 * C + D, B, N, C, D)
    for rows in (32, 64):
      line('mpnn_forward', case + (rows,), TM._run(S, device_l(L, lkind), W, num_prop, agg, pad=pad, tile_rows=rows)[0])
  for case in TGT.STEP_CASES:
    N, C, D, B, steps, agg, pad, lkind = case
    S, L, W, dST = TGT.step_case_inputs(N, C, D, B, lkind)
    backward_steps('ggnn_backward_step', case, S, dST, device_l(L, lkind), W, steps, agg == 'avg',
                   lambda s, l, w, n, a: ops.ggnn_forward_states(s, l, None, *w, n, avg=a)[1],
                   ops.ggnn_pack_transposes, ops.ggnn_step_buffers, ops.ggnn_backward_step)
  for case in MGM.STEP_CASES:
    N, C, D, B, steps, agg, pad, lkind = case
    S, L, W, dST = MGM.step_case_inputs(N, C, D, B, steps, agg, lkind)
    backward_steps('mpnn_backward_step', case, S, dST, device_l(L, lkind), W, steps, agg == 'avg',
                   lambda s, l, w, n, a: ops.mpnn_forward_states(s, l, *w, n, avg=a),
                   ops.mpnn_pack_transposes, ops.mpnn_step_buffers, ops.mpnn_backward_step)
  for case in TGT.READOUT_CASES:
    N, D, P, mkind, B, pad = case
    S, _, W = TGT.GM.draw_operands(5000 + N + D + P, B, N, 1, D, P=P)
    mask = TGT._mask(mkind, B, N, 23 + N)
    dscore = torch.randn(B, P, generator=torch.Generator().manual_seed(14))
    line('ggnn_readout_backward', case, *ops.ggnn_readout_backward(
        TGT._padded(S, pad)[0], None if mask is None else mask.cuda(), *[w.cuda() for w in W[8:]], dscore.cuda()))


if __name__ == '__main__':
  main()
