"""lnz_head_backward and lnz_node_extents (csrc/head_grad.hip) at their seams, against float64 autograd through the
reference's read-out (model/lanczos_net.py:185-194) on operands drawn on the host (tests/train_kernel_cases.py:
HEAD_CASES; the CPU side of it: tests/test_train_kernel_cases_cpu.py).

Cases (B, N, P, n_wg, gate form): P = 16 takes head_backward_kernel<17, true>, 15 / 17 / 31 / 1 / 2 the <32, false>
form; n_wg = 1 (one workgroup walks every molecule, so the prefetch chain runs), n_wg > B (clamped), B no
multiple of n_wg.  Every case runs in BOTH gate forms — the stacked head (Wgate=None) and the module's own call with
the gate row on its own (model/_small.py) — which must give the same bits.  Masks: a masked node 0, an interior
hole, an EMPTY mask, a molecule whose only real node is the last one (extent N, count 1).  The state is post-ReLU
with exact zeros, and every row outside the mask (holes, rows N .. 31) holds finite non-zero values; one case has
gate pre-activations of +-100.

Bar (the scheme of test_gpu_gat_train.py): truth = float64; e32 = the error of the same autograd in CPU float32 in
units of max|truth| of that tensor, the LARGEST of eight evaluations (as given, and seven with molecules and nodes
consistently permuted); the kernel has to be within max(k e32, 4 * 2^-23) of max|truth|, k = 4.  Measured with the
reference alone (tools/train_kernel_reference_spread.py): worst / best of the eight evaluations is at most 3.27
(B7_N31_P15, dW) over these cases — under 4, so k stays 4 —, e32 between 5.7e-8 (B = N = P = 1) and 1.2e-6 (dY of
the +-100 case); dW 1.7e-7 .. 4.0e-7.  Where the truth is identically zero (rows outside the mask, rows N .. 31,
the empty-mask molecule) the kernel's dY has to be exactly 0.

The empty mask: torch autograd gives 0 / 0 for that molecule's score; the kernel contributes nothing for it (its dz
are exact zeros) — pinned here: its dY is 0, every result is finite, and the parameter gradients are the truth of
the batch WITHOUT it (which is what train_kernel_cases.head_eval computes)."""
import functools

import pytest
import torch

import train_kernel_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SPARE = 40        # rows of the compact buffer behind the last molecule (>= 32: a whole tile of slack)
GAP = 3           # unused rows between two molecules of the compact buffer


def _same_bits(a, b):
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _device_operands(B, N, P, g100):
  o = C.head_operands(B, N, P, g100)
  d = {k: o[k].to(DEV) for k in ('X', 'gs', 'W', 'b')}
  d['mask'] = o['mask'].to(torch.uint8).to(DEV)
  ext = (o['mask'].long() * torch.arange(1, N + 1)).amax(dim=1)
  d['extent'] = ext
  d['row_off'] = torch.cumsum(ext + GAP, 0) - ext - GAP + 1      # gaps of GAP rows, one unused row in front
  return d


def _run(d, P, n_wg, gate, compact=True):
  from lanczosnet_amd import ops
  B = d['X'].shape[0]
  N = d['mask'].shape[1]
  dY = torch.full((B, 32, 128), float('nan'), device=DEV)
  dYc = off = None
  if compact:
    R = int(d['row_off'][-1] + d['extent'][-1])
    dYc = torch.full((R + SPARE, 128), float('nan'), device=DEV)
    off = d['row_off'].to(DEV)
  if gate == 'stacked':
    res = ops.head_backward(d['X'], d['mask'], d['gs'], d['W'], d['b'], N, dY, row_off=off, dY_compact=dYc,
                            n_wg=n_wg)
  else:
    res = ops.head_backward(d['X'], d['mask'], d['gs'], d['W'][:P].contiguous(), d['b'][:P].contiguous(), N, dY,
                            row_off=off, dY_compact=dYc, n_wg=n_wg,
                            Wgate=d['W'][P:].contiguous(), bgate=d['b'][P:].contiguous())
  return (dY,) + tuple(res), dYc


@pytest.mark.parametrize('case', C.HEAD_CASES, ids=[C.head_id(c) for c in C.HEAD_CASES])
def test_head_backward_at_its_seams(case):
  B, N, P, n_wg, gate = case
  g100 = case[:4] == C.HEAD_GATE100
  d = _device_operands(B, N, P, g100)
  truth, e32, _ = C.head_reference(B, N, P, g100)
  got, dYc = _run(d, P, n_wg, gate)
  other, dYc2 = _run(d, P, n_wg, 'split' if gate == 'stacked' else 'stacked')
  again, _ = _run(d, P, n_wg, gate)
  for name, a, b_, c in zip(C.HEAD_NAMES, got, other, again):
    assert _same_bits(a, b_), 'the two gate forms differ in ' + name
    assert _same_bits(a, c), 'two identical calls differ in ' + name
  assert _same_bits(dYc, dYc2)
  dY = got[0].cpu()
  mask = d['mask'].cpu().bool()
  for name, g in zip(C.HEAD_NAMES, got):
    g = g.double().cpu()
    assert torch.isfinite(g).all(), name
    g = g[:, :N] if name == 'dY' else g
    t = truth[name]
    assert tuple(g.shape) == tuple(t.shape), name
    scale = float(t.abs().max())
    err = float((g - t).abs().max()) / scale
    bar = C.bar(e32[name], C.K_HEAD)
    print('head_backward %s %s: %.2e of max|truth|, float32 autograd (worst of 8) %.2e, bar %.2e'
          % (C.head_id(case), name, err, e32[name], bar))
    assert err <= bar, (name, err, bar)
  # exactly zero where the truth is: rows outside the mask (the empty-mask molecule among them), rows N .. 31
  assert (dY[:, :N][~mask] == 0).all() and (dY[:, N:] == 0).all()
  # the compact copy, every molecule: its extent rows bit for bit (hole rows included), nothing else written
  dYc = dYc.cpu()
  written = torch.zeros(dYc.shape[0], dtype=torch.bool)
  for b in range(B):
    lo, e = int(d['row_off'][b]), int(d['extent'][b])
    assert _same_bits(dYc[lo:lo + e], dY[b, :e]), b
    written[lo:lo + e] = True
  assert int(written.sum()) == int(d['extent'].sum())
  assert torch.isnan(dYc[~written]).all(), 'rows outside every molecule\'s [row_off, row_off + extent) were written'
  # dY is computed per molecule: the same bits whatever the number of workgroups
  for other_wg in (1, 3, 256):
    if other_wg != n_wg:
      alt, _ = _run(d, P, other_wg, gate, compact=False)
      assert _same_bits(alt[0], got[0]), other_wg


def test_head_backward_refusals():
  from lanczosnet_amd import ops

  def call(B=2, N=5, P=3, n_wg=2, compact=False, off=False):
    X = torch.ones((B, 32, 128), device=DEV)
    mask = torch.ones((B, N), dtype=torch.uint8, device=DEV)
    W, b = torch.ones((P + 1, 128), device=DEV), torch.ones((P + 1,), device=DEV)
    dY = torch.zeros((B, 32, 128), device=DEV)
    return ops.head_backward(X, mask, torch.ones((B, P), device=DEV), W, b, N, dY, n_wg=n_wg,
                             dY_compact=torch.zeros((B * N + 32, 128), device=DEV) if compact else None,
                             row_off=N * torch.arange(B, dtype=torch.int64, device=DEV) if off else None)

  call()
  call(compact=True, off=True)
  for kw in (dict(P=32), dict(N=33)):
    with pytest.raises(ops.NotSupported):
      call(**kw)
  for kw in (dict(n_wg=0), dict(n_wg=4097), dict(compact=True)):
    with pytest.raises(ops.LnzError) as e:
      call(**kw)
    assert not isinstance(e.value, ops.NotSupported), kw


@pytest.mark.parametrize('N', [1, 32])
@pytest.mark.parametrize('B', [1, 1023, 1024, 1025, 2049])
def test_node_extents_at_the_chunk_boundaries(B, N):
  """The 1024-molecule chunk loop's carry at its boundaries; all-zero masks at the first and the last position
  of a chunk; integer equality with the cumulative-sum restatement, the total included."""
  from lanczosnet_amd import ops
  g = torch.Generator().manual_seed(B + N)
  mask = (torch.rand((B, N), generator=g) < 0.6).to(torch.uint8)
  for b in (0, 1023, 1024, 2047, 2048, B - 1):
    if 0 <= b < B and B > 1:
      mask[b] = 0
  if B > 2:
    mask[1, N - 1] = 1          # extent N
  want = (mask.long() * torch.arange(1, N + 1)).amax(dim=1)
  ext, off, tot = ops.node_extents(mask.to(DEV))
  assert ext.dtype == off.dtype == tot.dtype == torch.int64
  assert torch.equal(ext.cpu(), want)
  assert torch.equal(off.cpu(), torch.cumsum(want, 0) - want)
  assert int(tot) == int(want.sum())
  if B == 1:
    assert int(tot) == int(want[0]) and int(off[0]) == 0
