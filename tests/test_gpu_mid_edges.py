"""The four launches for graphs of 33..128 nodes (csrc/conv_mid.hip: lnz_midgraph_forward;
csrc/conv_mid_grad.hip: lnz_midgraph_head_grad, lnz_midgraph_input_grad, lnz_midgraph_project;
DESIGN.md §4.9b) through the raw ops, one case per kernel seam, against the float64 restatement of
tests/mid_mirror.py — never through the module, `lanczos_ritz` or `spectral_gains`: V, G and the
weights are data to these kernels and are drawn seeded (`_case`).

What is compared.  Forward: every layer's state rows and the score, per graph.  Every backward
launch on THE INPUTS IT WAS GIVEN — the GPU forward's exchange buffer and the GPU dOut, moved to the
host and promoted to float64: dOut of the last layer and the head's per-graph partials; dOut of every
other layer and dX0; A, Q, M, dG and db.  The stored-state sign pattern is then an input of the
comparison, not something fp32 and float64 can disagree on (the caveat above the case list of
test_gpu_mid_train.py does not arise).  Bar: `rel_err_rows` of conftest.py — per graph, the maximum
error over the maximum of the float64 value — below the project's fp32 bar 1e-5, per
layer.  Exactly zero: state rows [N, NR); dOut, dX0 and M rows at or beyond a graph's n; dOut of the
last layer where the mask is 0.  dG has no slots >= K (its shape).  `folded` exactly.

CONDITIONING.  The bar is met only where fp32 itself meets it.  Every case was run on the CPU with
the mirror in fp32 against the mirror in float64, same functions, same inputs (`_mirror_chain`
through `_deviations`; tests/test_mid_mirror_cpu.py repeats it and holds every case four times inside
the bar: a kernel with another summation order draws another sample of the same rounding).  The
figures are in the CONDITIONING comment below the case list."""
import functools

import numpy as np
import pytest
import torch

import mid_mirror
from conftest import rel_err_rows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-5
OUTPUTS = ('state', 'score', 'dOut_last', 'dWhead', 'dbhead', 'dOut', 'dX0', 'A', 'Q', 'M', 'dG', 'db')

# name: ns (the graphs' node counts), N, K, S, C, din0, layers, dout and
#   second: channel 1 of L (C = 2) — 'equal' | 'unequal' | 'mixed' (unequal in every other graph) | 'nonsym'
#   lform:  how L lies in memory — 'plain' | 'expand' (one channel, channel stride 0) | 'chmajor'
#           ([B,C,N,N] permuted to [B,N,N,C]) | 'wide' (every other channel of a [B,N,N,2C] tensor)
#   mask:   'prefix' | 'holes' (rows among the first n masked out)
# The seam each case sits on is named with the code that has it.
_D = dict(K=20, S=3, C=2, din0=16, layers=3, dout=2, second='mixed', lform='plain', mask='prefix')
CASES = {
    # every 16-row wave seam of the full tile (`wave < R`, `t < R`, `row < N` with R = 8), graphs of
    # n < K among them (dead eigen slots), folded and unfolded graphs in one batch, 14 graphs = two
    # groups of 8 with `b >= b1` blocks
    'N=128, n on every wave seam': dict(_D, ns=[1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 96, 97, 127, 128], N=128),
    # R = 3 with one live row in the last tile; the reference's eight long scales (one per wave)
    'N=33': dict(_D, ns=[33, 20, 33, 7, 32], N=33, S=8, second='equal'),
    # the reference's own shape: N = 100 (R = 7, four live rows in the last tile), K = 20, S = 8, equal channels
    'N=100': dict(_D, ns=[100, 57, 99, 81], N=100, S=8, second='equal'),
    # N = 127: R = 8 with one dead row; C = 1 (the <1> instantiations); S = 1; din0 = 48 (nk = 3, d4 = 12)
    'N=127, C=1, S=1, din0=48': dict(_D, ns=[127, 126, 112, 5], N=127, K=32, S=1, C=1, din0=48),
    # R = 1 and R = 2: the launchers accept N <= 32 (`N > 0`)
    'N=16 (R=1)': dict(_D, ns=[16, 1, 9], N=16, K=16, S=2, second='unequal', layers=2),
    'N=17 (R=2), S=7': dict(_D, ns=[17, 16, 5, 2], N=17, K=17, S=7, C=1, din0=32),
    # K: one slot; exactly the first slot tile; one slot in the second; both tiles full
    'K=1': dict(_D, ns=[40, 33, 3], N=40, K=1, S=2, second='equal'),
    'K=16, S=8': dict(_D, ns=[48, 10, 16, 17], N=48, K=16, S=8),
    # S = 9: wave 0 takes scales 0 and 8 (the second fetch at s >= 8)
    'K=17, S=9': dict(_D, ns=[48, 10, 16, 17, 18], N=48, K=17, S=9),
    # S = 16: every wave two scales, gs full (tid < S * 32 = 512)
    'K=32, S=16': dict(_D, ns=[64, 31, 32, 33, 5], N=64, K=32, S=16, second='unequal'),
    # S = 0: no gains, no A / Q / dG, the project kernel's early return; din0 = 112 (nk = 7: wave 7 idle in phase 1)
    'S=0, din0=112': dict(_D, ns=[50, 34, 12], N=50, K=12, S=0, second='unequal', din0=112),
    'din0=128, C=1, two layers': dict(_D, ns=[36, 35, 20], N=36, S=3, C=1, din0=128, layers=2),
    # a non-symmetric operator channel: the input gradient reads L transposed
    'non-symmetric channel': dict(_D, ns=[72, 40, 60], N=72, S=2, second='nonsym'),
    # element strides of L
    'L expanded (channel stride 0)': dict(_D, ns=[40, 37, 12], N=40, K=12, S=2, second='equal', lform='expand'),
    'L channel-major, permuted': dict(_D, ns=[40, 37, 12], N=40, K=12, S=2, second='unequal', lform='chmajor'),
    'L every other channel of a wider tensor': dict(_D, ns=[40, 37, 12], N=40, K=12, S=2, second='unequal', lform='wide'),
    # depth 1 (the forward's first layer is its last; the input gradient returns before any exchange),
    # one output, one graph
    'one layer, dout=1, B=1': dict(_D, ns=[77], N=80, layers=1, dout=1, second='unequal'),
    # dout = 31 at N = 128: yh fills 4096 of the 4224 floats of Ys, Wh all 32 rows; B = 7
    'dout=31, N=128, B=7': dict(_D, ns=[128, 100, 128, 64, 33, 90, 127], N=128, S=2, dout=31),
    # B = 9: a second group of 32 blocks with one graph, through the exchange of all three layers
    'B=9': dict(_D, ns=[40, 39, 38, 37, 36, 35, 34, 33, 20], N=40, S=2),
    # the kernels read the mask per row
    'mask with holes': dict(_D, ns=[60, 45, 33, 10], N=60, S=2, mask='holes'),
    # one graph and a one-row head through the exchange of all three layers (31 of 32 blocks return early)
    'B=1, dout=1, three layers': dict(_D, ns=[70], N=70, S=2, dout=1, second='unequal'),
}
IDS = list(CASES)
MIXED = 'N=128, n on every wave seam'
SEEDS = {}   # name: seed, where the default (1000 + the case's position) had to be changed (CONDITIONING)

# CONDITIONING (module docstring), on the CPU: the mirror in fp32 against the mirror in float64 on the
# inputs each stage was given — worst per-graph deviation over the layers, in units of 1e-7, of
#                                          state score dOut_last dWhead dbhead dOut dX0  A    Q    M    dG   db
#   N=128, n on every wave seam              2.8  5.3  1.7  2.8  1.2  2.5  3.6  5.2  4.4  2.6  6.3  1.2
#   N=33                                     3.1  0.8  1.4  1.4  0.5  3.0  3.2  2.5  2.8  1.8  3.6  2.1
#   N=100                                    2.7  0.8  2.0  2.9  1.2  2.9  3.9  3.6  3.8  2.6  4.6  1.4
#   N=127, C=1, S=1, din0=48                 3.6  2.6  1.8  3.0  0.4  2.6  2.2  3.2  3.9  2.6  3.8  0.9
#   N=16 (R=1)                               2.7  1.8  1.4  1.7  0.7  2.4  2.3  0.9  2.0  0.4  2.5  0.8
#   N=17 (R=2), S=7                          3.0  2.1  1.5  1.4  1.1  3.6  5.0  1.1  1.6  1.2  4.2  0.9
#   K=1                                      3.1  0.6  1.9  1.9  0.9  1.6  3.5  1.4  1.2  1.8  7.2  1.0
#   K=16, S=8                                3.2  1.7  1.7  1.2  0.7  4.0  4.3  2.5  2.1  1.0  4.0  1.2
#   K=17, S=9                                3.4  1.7  1.8  1.3  1.0  3.5  5.6  2.0  2.6  1.0  4.3  1.1
#   K=32, S=16                               3.9  1.1  1.8  2.3  0.7  3.8  4.1  2.0  2.4  0.8  4.2  1.3
#   S=0, din0=112                            3.9  1.6  1.7  1.1  0.5  2.2  2.6    -    -  0.9    -  1.2
#   din0=128, C=1, two layers                4.0  1.7  1.5  1.9  0.5  3.0  3.1  2.7  2.6  1.1  2.5  1.0
#   non-symmetric channel                    3.3  3.0  2.0  1.7  1.3  3.0  3.8  3.9  2.7  4.0  5.1  0.8
#   L expanded (channel stride 0)            2.4  1.0  1.6  1.2  0.6  2.6  2.5  2.3  2.2  1.5  5.7  1.0
#   L channel-major, permuted                3.9  1.0  1.3  1.2  1.0  2.1  2.7  1.5  2.4  1.3  2.9  1.0
#   L every other channel of a wider tensor  3.7  0.7  1.3  1.5  0.6  2.7  2.8  2.7  2.3  0.9  5.0  1.2
#   one layer, dout=1, B=1                   1.6  1.0  1.4  2.6  0.6    -  1.7  1.5  1.7  0.5  1.5  0.6
#   dout=31, N=128, B=7                      2.3  1.1  4.5  3.3  1.0  3.1  2.2  3.7  4.6  2.6  4.6  1.1
#   B=9                                      2.4  1.0  1.7  1.4  1.4  2.5  2.9  2.3  2.9  1.6  8.4  1.6
#   mask with holes                          2.1  1.2  1.7  1.4  0.9  3.0  2.9  2.4  3.4  1.2  3.2  1.7
#   B=1, dout=1, three layers                2.2  0.2  1.5  2.1  0.6  1.9  2.1  2.4  3.3  0.9  7.5  1.0
# (- = the case has no such output.)  The worst is 8.4e-7 (dG at B = 9): fp32 alone stays eleven times
# inside the bar on every case, and no seed had to be changed.  On an MI355X the kernels' worst over all
# cases and outputs was 1.0e-6 (dG, the wave-seam case), the next 8.4e-7 (dG at K = 1).


def _sym_norm(rs, n, p):
  """D^-1/2 (A + I) D^-1/2 of a random graph on n nodes (float64)."""
  up = np.triu(rs.rand(n, n) < p, 1).astype(np.float64)
  A = up + up.T + np.eye(n)
  d = 1.0 / np.sqrt(A.sum(axis=1))
  return A * d[:, None] * d[None, :]


@functools.lru_cache(maxsize=None)
def _case(name):
  """Host operands of a case (fp32 torch tensors; W a list of [128, S + C, din_l]), drawn from its seed."""
  c = CASES[name]
  ns, N, K, S, C, din0, nl, dout = (c[k] for k in ('ns', 'N', 'K', 'S', 'C', 'din0', 'layers', 'dout'))
  rs = np.random.RandomState(SEEDS.get(name, 1000 + IDS.index(name)))
  B = len(ns)
  L = np.zeros((B, N, N, C))
  V = np.zeros((B, N, K))
  mask = np.zeros((B, N), np.uint8)
  for b, n in enumerate(ns):
    L[b, :n, :n, 0] = _sym_norm(rs, n, 0.3)
    if C == 2:
      kind = c['second'] if c['second'] != 'mixed' else ('unequal' if b % 2 == 0 else 'equal')
      L[b, :n, :n, 1] = {'equal': lambda: L[b, :n, :n, 0], 'unequal': lambda: _sym_norm(rs, n, 0.05),
                         'nonsym': lambda: rs.randn(n, n) * 0.1}[kind]()
    k = min(n, K)
    V[b, :n, :k] = np.linalg.qr(rs.randn(n, k))[0]   # rows >= n and columns >= n stay zero
    mask[b, :n] = 1
    if c['mask'] == 'holes' and n > 1:
      mask[b, rs.choice(n, size=max(1, n // 4), replace=False)] = 0
  f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
  W = [f(rs.randn(128, S + C, d) / np.sqrt((S + C) * d)) for d in [din0] + [128] * (nl - 1)]
  return dict(c, name=name, B=B, L=f(L), V=f(V), mask=torch.from_numpy(mask),
              G=f(rs.uniform(-1, 1, size=(nl, B, S, K))) if S else None,
              X0=f(rs.randn(B, N, din0)),   # all N rows: nothing may leak from rows >= n through L or V
              W=W, bias=f(rs.randn(nl, 128) * 0.1), Whead=f(rs.randn(dout + 1, 128) / np.sqrt(128)),
              bhead=f(rs.randn(dout + 1) * 0.1), gscore=f(rs.randn(B, dout)))


def _pad_rows(t, NR, dim):
  pad = [0, 0] * (t.dim() - 1 - dim) + [0, NR - t.shape[dim]]
  return torch.nn.functional.pad(t, pad)


def _mirror_chain(c, dtype):
  """The four launches by tests/mid_mirror.py in `dtype` on the host, each stage on the previous
  stage's output, in the layout of `_gpu_chain` (node rows padded to NR with zeros)."""
  m, NR = mid_mirror, (c['N'] + 15) // 16 * 16
  states, score = m.forward(c['X0'].to(dtype), c['L'], c['V'], c['G'], c['mask'], c['W'], c['bias'],
                            c['Whead'], c['bhead'])
  d_last, dWh, dbh = m.head_grad(states[-1], c['mask'], c['gscore'], c['Whead'], c['bhead'])
  dOut, dX0 = m.input_grad(d_last, states, c['L'], c['V'], c['G'], c['W'], c['din0'])
  A, Q, M, dG, db = m.project(dOut, states, c['X0'], c['L'], c['V'], c['G'], c['W'])
  return dict(states=_pad_rows(states, NR, 2), score=score, dOut=_pad_rows(dOut, NR, 2), dWhead=dWh, dbhead=dbh,
              dX0=_pad_rows(dX0, NR, 1), A=A, Q=Q, M=_pad_rows(M, NR, 2), dG=dG, db=db, folded=None)


def _device_L(L, lform):
  """The values of L [B,N,N,C] on the device in the case's memory layout."""
  L = L.to(DEV)
  if lform == 'expand':
    assert torch.equal(L[..., 0], L[..., 1])
    out = L[..., :1].contiguous().expand(-1, -1, -1, 2)
    assert out.stride(3) == 0
  elif lform == 'chmajor':
    out = L.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert out.stride(3) == L.shape[1] * L.shape[2]
  elif lform == 'wide':
    wide = torch.full(L.shape[:3] + (2 * L.shape[3],), 7.0, device=DEV)   # the channels between are junk
    wide[..., ::2] = L
    out = wide[..., ::2]
    assert out.stride(3) == 2
  else:
    out = L.contiguous()
  assert torch.equal(out, L)
  return out


def _gpu_chain(c, V=None):
  """The four launches through the raw ops; every output on the host.  dOut and the head's workspace,
  the buffers allocated here, start as NaN: an element no launch writes shows.  (The wrappers allocate
  the others; `_deviations` wants every element of every output finite.)"""
  from lanczosnet_amd import ops
  t = lambda x: None if x is None else x.to(DEV).contiguous()
  B, N, P = c['B'], c['N'], c['dout']
  X0, G, mask, bias, Wh, bh, gscore = (t(c[k]) for k in ('X0', 'G', 'mask', 'bias', 'Whead', 'bhead', 'gscore'))
  V = t(c['V'] if V is None else V)
  L = _device_L(c['L'], c['lform'])
  W, Wt = (t(w) for w in mid_mirror.pack_weights(c['W']))
  score, Xw = ops.midgraph_forward(X0, L, V, G, mask, W, bias, Wh, bh, c['layers'], return_work=True)
  assert tuple(Xw.shape) == (c['layers'], B, (N + 15) // 16 * 16, 128) and tuple(score.shape) == (B, P)
  dOut = torch.full_like(Xw, float('nan'))
  dWh, dbh = ops.midgraph_head_grad(Xw, mask, gscore, Wh, bh, dOut)
  # the per-graph partials: the same launch on a workspace of our own (ops.midgraph_head_grad adds them up)
  ws = torch.full((int(ops._abi().midgraph_head_grad_workspace_floats(B, P)),), float('nan'), device=DEV)
  d2 = torch.full_like(Xw[-1], float('nan'))
  ops._abi().midgraph_head_grad(Xw[-1], mask, gscore, Wh, bh, B, N, P, d2, ws)
  nw = B * (P + 1) * 128
  dWpart, dbpart = ws[:nw].view(B, P + 1, 128), ws[nw:].view(B, P + 1)
  assert torch.equal(d2, dOut[-1]) and torch.equal(dWpart.sum(dim=0), dWh) and torch.equal(dbpart.sum(dim=0), dbh)
  dX0, folded = ops.midgraph_input_grad(dOut, Xw, L, V, G, Wt, N, c['din0'], want_dx0=True)
  A, Q, M, dG, db = ops.midgraph_project(dOut, Xw, X0, L, V, G, W)
  torch.cuda.synchronize()
  h = lambda x: None if x is None else x.cpu()
  return dict(states=h(Xw), score=h(score), dOut=h(dOut), dWhead=h(dWpart), dbhead=h(dbpart), dX0=h(dX0),
              A=h(A), Q=h(Q), M=h(M), dG=h(dG), db=h(db), folded=h(folded))


@functools.lru_cache(maxsize=None)
def _forward64(name):
  """The float64 forward of a case, computed once and never written to."""
  c = _case(name)
  return mid_mirror.forward(c['X0'].double(), c['L'], c['V'], c['G'], c['mask'], c['W'], c['bias'],
                            c['Whead'], c['bhead'])


def _worst(got, ref):
  """max over the leading (layer) dimension of rel_err_rows over the graphs; nan if any of them is
  (np.max propagates it, Python's max() does not)."""
  return float(np.max([rel_err_rows(g.numpy(), r.numpy()) for g, r in zip(got, ref)]))


def _deviations(c, out, V=None):
  """Worst per-graph deviation of every output of a chain (`_gpu_chain` or `_mirror_chain` in fp32)
  from the float64 mirror ON THE INPUTS EACH LAUNCH WAS GIVEN, and the exact zeros."""
  m = mid_mirror
  N, ns, nl, K, S = c['N'], c['ns'], c['layers'], c['K'], c['S']
  V = c['V'] if V is None else V
  states, dOut = out['states'][:, :, :N], out['dOut'][:, :, :N]
  for k, v in out.items():   # every element of every output, padding included
    assert v is None or not v.is_floating_point() or torch.isfinite(v).all(), k
  dev = {}
  # ---- forward: all of it is one launch
  s64, score64 = _forward64(c['name']) if V is c['V'] else m.forward(
      c['X0'].double(), c['L'], V, c['G'], c['mask'], c['W'], c['bias'], c['Whead'], c['bhead'])
  dev['state'] = _worst(states, s64)
  dev['score'] = _worst([out['score']], [score64])
  assert not out['states'][:, :, N:].any()
  # ---- head, on the stored last state
  d64, dWh64, dbh64 = m.head_grad(states[-1].double(), c['mask'], c['gscore'], c['Whead'], c['bhead'])
  dev['dOut_last'] = _worst([dOut[-1]], [d64])
  dev['dWhead'] = _worst([out['dWhead']], [dWh64])
  dev['dbhead'] = _worst([out['dbhead']], [dbh64])
  assert tuple(out['dWhead'].shape) == (c['B'], c['dout'] + 1, 128)
  assert not out['dOut'][-1][_pad_rows(c['mask'], out['dOut'].shape[2], 1) == 0].any()
  # ---- dOut of the other layers and dX0, on the stored states and the head's dOut
  dO64, dX64 = m.input_grad(dOut[-1].double(), states.double(), c['L'], V, c['G'], c['W'], c['din0'])
  dev['dOut'] = _worst(dOut[:-1], dO64[:-1]) if nl > 1 else None
  dev['dX0'] = _worst([out['dX0'][:, :N]], [dX64])
  assert tuple(out['dX0'].shape) == (c['B'], out['dOut'].shape[2], c['din0'])
  # ---- the projections, on the stored states and the launches' dOut
  A64, Q64, M64, dG64, db64 = m.project(dOut.double(), states, c['X0'], c['L'], V, c['G'], c['W'])
  dev['M'] = _worst(out['M'][:, :, :N], M64)
  dev['db'] = _worst(out['db'], db64)
  for k, ref in (('A', A64), ('Q', Q64), ('dG', dG64)):
    assert (out[k] is None) == (S == 0), k
    dev[k] = _worst(out[k], ref) if S else None
  if S:
    assert tuple(out['dG'].shape) == (nl, c['B'], K, S) and tuple(out['A'].shape) == (nl, c['B'], K, 128)
    assert tuple(out['Q'].shape) == (nl, c['B'], K, S, 128)
  for b, n in enumerate(ns):   # rows at or beyond a graph's node count, rows [N, NR) among them
    assert not out['dOut'][:, b, n:].any(), ('dOut', b)
    assert not out['dX0'][b, n:].any(), ('dX0', b)
    assert not out['M'][:, b, n:].any(), ('M', b)
  if out['folded'] is not None:
    want = [int(c['C'] == 2 and torch.equal(c['L'][b, ..., 0], c['L'][b, ..., 1])) for b in range(c['B'])]
    assert out['folded'].tolist() == want, (out['folded'].tolist(), want)
  return dev


def _line(dev):
  return '  '.join('%s %s' % (k, '-' if dev[k] is None else '%.1e' % dev[k]) for k in OUTPUTS)


def _worst_of(dev):
  """(deviation, output) of the worst output; a nan deviation is the worst there is."""
  vals = [(float('inf') if np.isnan(v) else v, k) for k, v in dev.items() if v is not None]
  return max(vals)


def _inside(dev, bar):
  """Every output's deviation is a number below `bar` (`v < bar` is False for nan)."""
  return all(v < bar for v in dev.values() if v is not None)


# ---- 1. every launch against float64, one case per seam
@pytest.mark.parametrize('name', IDS, ids=IDS)
def test_every_launch_matches_float64_on_its_own_inputs(name):
  c = _case(name)
  with torch.no_grad():
    dev = _deviations(c, _gpu_chain(c))
    cond = _deviations(c, _mirror_chain(c, torch.float32))
  print('%s\n  kernels     %s\n  fp32 mirror %s' % (name, _line(dev), _line(cond)))
  assert _inside(dev, BAR), _worst_of(dev)


# ---- 2. non-finite Ritz entries stay with their graph
def test_a_nan_and_an_inf_in_v_are_read_as_zero_and_stay_with_their_graph():
  """finite_or_zero on both stagings of V (Vt and the vf fragments) in the forward and the input
  gradient, and on Vt in the projections: every output of every launch is finite (`_deviations`), graph
  1 equals the mirror with zeros there, every other graph has the bits of the same batch without them."""
  c = _case('K=16, S=8')
  bad = 1
  V = c['V'].clone()
  assert c['ns'][bad] == 10 and c['V'][bad, 3, 2] != 0 and c['V'][bad, 7, 9] != 0   # live rows, live slots
  V[bad, 3, 2], V[bad, 7, 9] = float('nan'), float('inf')
  with torch.no_grad():
    clean, out = _gpu_chain(c), _gpu_chain(c, V=V)
    dev = _deviations(c, out, V=V)
  print('NaN and inf in V of graph %d\n  kernels     %s' % (bad, _line(dev)))
  assert _inside(dev, BAR), _worst_of(dev)
  others = [b for b in range(c['B']) if b != bad]
  for k, bdim in (('states', 1), ('score', 0), ('dOut', 1), ('dWhead', 0), ('dbhead', 0), ('dX0', 0), ('A', 1),
                  ('Q', 1), ('M', 1), ('dG', 1), ('db', 1)):
    a, b = (x[k].index_select(bdim, torch.tensor(others)) for x in (clean, out))
    assert torch.equal(a, b), k
    assert not torch.equal(clean[k].select(bdim, bad), out[k].select(bdim, bad)), k   # (the entries mattered)


# ---- 3. repeatability
def test_a_second_run_of_all_four_launches_gives_the_same_bits():
  c = _case(MIXED)
  with torch.no_grad():
    one, two = _gpu_chain(c), _gpu_chain(c)
  for k in one:
    assert torch.equal(one[k], two[k]), k


# ---- 4. the envelope checks of the four raw ops: nothing is launched
def _shapes(N=40, K=20, S=2, C=2, din0=16, dout=2, B=2, nl=2):
  z = lambda *s: torch.zeros(s, device=DEV)
  NR, nch = (N + 15) // 16 * 16, S + C
  return dict(X0=z(B, N, din0), L=z(B, N, N, C), V=z(B, N, K), G=z(nl, B, S, K) if S else None,
              mask=torch.ones((B, N), dtype=torch.uint8, device=DEV), W=z(128 * nch * (din0 + 128 * (nl - 1))),
              Wt=z(nl * 128 * nch * 128), bias=z(nl, 128), Wh=z(dout + 1, 128), bh=z(dout + 1), gscore=z(B, dout),
              Xw=z(nl, B, NR, 128), dOut=z(nl, B, NR, 128), N=N, din0=din0, nl=nl)


def _forward(s):
  from lanczosnet_amd import ops
  ops.midgraph_forward(s['X0'], s['L'], s['V'], s['G'], s['mask'], s['W'], s['bias'], s['Wh'], s['bh'], s['nl'])


def _head_grad(s):
  from lanczosnet_amd import ops
  ops.midgraph_head_grad(s['Xw'], s['mask'], s['gscore'], s['Wh'], s['bh'], s['dOut'])


def _input_grad(s):
  from lanczosnet_amd import ops
  ops.midgraph_input_grad(s['dOut'], s['Xw'], s['L'], s['V'], s['G'], s['Wt'], s['N'], s['din0'], want_dx0=True)


def _project(s):
  from lanczosnet_amd import ops
  ops.midgraph_project(s['dOut'], s['Xw'], s['X0'], s['L'], s['V'], s['G'], s['W'])


CONV_OPS = (_forward, _input_grad, _project)
ENVELOPE = {   # what is outside: (the shapes, every raw op that takes that argument)
    'N=129': (dict(N=129), CONV_OPS + (_head_grad,)),
    'K=33': (dict(K=33), CONV_OPS),
    'S=17': (dict(S=17), CONV_OPS),
    'C=3': (dict(C=3), CONV_OPS),
    'din0=24': (dict(din0=24), CONV_OPS),
    'din0=144': (dict(din0=144), CONV_OPS),
    'dout=32': (dict(dout=32), (_forward, _head_grad)),
}


@pytest.mark.parametrize('what', list(ENVELOPE))
def test_outside_the_envelope_every_raw_op_refuses(what):
  from lanczosnet_amd import ops
  kw, fns = ENVELOPE[what]
  s = _shapes(**kw)
  for fn in fns:
    with pytest.raises(ops.NotSupported):
      fn(s)


def test_the_same_calls_inside_the_envelope_go_through():
  """(so that each refusal above is the one argument's doing)"""
  for fn in (_forward, _head_grad, _input_grad, _project):
    fn(_shapes())
  torch.cuda.synchronize()


def test_long_scales_without_gains_are_refused():
  """S > 0 with G = None.  The wrappers of ops.py read S from G; the entry points take both."""
  from lanczosnet_amd import ops
  s, S = _shapes(S=0), 2
  B, N, din0, nl = 2, s['N'], s['din0'], s['nl']
  K, C, NR = s['V'].shape[2], s['L'].shape[3], s['Xw'].shape[2]
  st = s['L'].stride()
  W = torch.zeros(128 * (S + C) * (din0 + 128 * (nl - 1)), device=DEV)
  Wt = torch.zeros(nl * 128 * (S + C) * 128, device=DEV)
  sync = torch.zeros(B * (nl + 1) + 16, dtype=torch.int32, device=DEV)
  ws = torch.zeros(int(ops._abi().midgraph_project_workspace_floats(B, N, K, C, S, nl)), device=DEV)
  with pytest.raises(ops.NotSupported):
    ops._abi().midgraph_forward(s['X0'], s['L'], *st, s['V'], None, s['mask'], W, s['bias'], s['Wh'], s['bh'], B, N,
                                K, C, S, nl, din0, 2, s['Xw'].view(-1), sync, torch.zeros(B, 2, device=DEV))
  with pytest.raises(ops.NotSupported):
    ops._abi().midgraph_input_grad(s['dOut'], s['Xw'], s['L'], *st, s['V'], None, Wt, B, N, K, C, S, nl, din0, sync,
                                   torch.zeros(B, NR, din0, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV))
  with pytest.raises(ops.NotSupported):
    ops._abi().midgraph_project(s['dOut'], s['Xw'], s['X0'], s['L'], *st, s['V'], None, W, B, N, K, C, S, nl, din0,
                                1, ws)
