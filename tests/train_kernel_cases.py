"""Cases, host-drawn operands and float64 / float32 references of the three hand-written kernels in the
backward of the <= 32-node training step, shared by tests/test_train_kernel_cases_cpu.py (no GPU), the
GPU files test_gpu_head_grad_edges.py, test_gpu_mlp_grad_edges.py, test_gpu_gain_grad_edges.py and
tools/train_kernel_reference_spread.py:

  lnz_head_backward        (csrc/head_grad.hip)            HEAD_CASES
  lnz_spectral_mlp_grad    (csrc/spectral_gains_grad.hip)  MLP_CASES
  lnz_lanczosnet_gain_grad (csrc/conv_strip.hip strip_gain_grad<1..6>, csrc/conv_forward.hip
                            lanczosnet_gain_grad_kernel<4,1> / <4,0>)   GAIN_CASES

Every reference is written from the reference model's formulas (model/lanczos_net.py:95-123, 146-149,
157-194), never from a kernel: `*_eval(operands, dtype, draw)` evaluates one of them in `dtype` on the CPU,
draw 0 on the operands as given, draws 1..7 with the molecules and the rows (nodes / live eigen rows)
consistently permuted and the results un-permuted.  `reference(fn)` gives

  truth   the float64 evaluation (draw 0),
  e32     per output tensor, the LARGEST error of the eight float32 evaluations in units of max|truth|,
  spread  per output tensor, worst / best of the eight, each error first raised to one ulp (2^-23) of the
          scale: below that the bar's floor of 4 ulp decides whatever k is.

The kernel has to be within bar(e32, k) = max(k e32, 4 * 2^-23) of max|truth|; k is the project's 4 unless
the measured spread of a case is larger (K_HEAD, K_GAIN, K_MLP and K_MLP_CASE below, re-measured by
tools/train_kernel_reference_spread.py).  No kernel output enters a bar."""
import functools

import numpy as np
import torch

ULP = 2.0 ** -23
DRAWS = 8

# k of the bar: the project's 4, and for a case whose eight float32 evaluations differ by more than that, the
# case's own worst / best.  Measured on the CPU with the references alone
# (tools/train_kernel_reference_spread.py), largest worst / best over a kernel's cases and tensors:
#   head 3.27 (B7_N31_P15, dW), gain gradient 2.08 (sub5_B5_L1, dG/0): k = 4;
#   filter MLP: 8.14 at S = 1 (db6/1; the one feature is D^30, ~0 on most rows, and the gradients nearly
#   cancel: e32 7.3e-6) and 4.88 at S = 4 (db6/0), at most 2.84 in every other case.
K_HEAD = 4.0
K_GAIN = 4.0
K_MLP = 4.0
K_MLP_CASE = {(65, 2, 2, 1, 'asc'): 8.14, (65, 2, 2, 4, 'asc'): 4.88}


def mlp_k(case):
  return K_MLP_CASE.get(tuple(case), K_MLP)


def bar(e32, k):
  return max(k * e32, 4.0 * ULP)


def _perm(draw, n, salt):
  if draw == 0:
    return torch.arange(n)
  g = torch.Generator().manual_seed(7919 * draw + 31 * n + salt)
  return torch.randperm(n, generator=g)


def reference(fn):
  """fn(dtype, draw) -> {name: tensor}.  -> (truth, e32, spread), see the module docstring."""
  truth = fn(torch.float64, 0)
  errs = {k: [] for k in truth}
  for draw in range(DRAWS):
    got = fn(torch.float32, draw)
    for k, t in truth.items():
      s = float(t.abs().max())
      errs[k].append(float((got[k].double() - t).abs().max()) / s if s > 0 else 0.0)
  e32 = {k: max(v) for k, v in errs.items()}
  spread = {k: max(max(v), ULP) / max(min(v), ULP) for k, v in errs.items()}
  return truth, e32, spread


# ------------------------------------------------------------------------------------------- head
# (B, N, P, n_wg, gate form)
HEAD_CASES = [
    (1, 1, 1, 1, 'stacked'),
    (5, 32, 16, 1, 'split'),       # <17, true>; one workgroup walks all molecules: the prefetch chain runs
    (5, 32, 16, 256, 'split'),     # n_wg > B, clamped
    (7, 31, 15, 3, 'stacked'),     # <32, false>; B no multiple of n_wg
    (7, 17, 17, 3, 'split'),       # the first P past the exact instantiation
    (9, 32, 31, 4, 'split'),       # P at PMAX
    (6, 5, 2, 6, 'stacked'),
]
HEAD_GATE100 = (5, 32, 16, 1)     # this (B, N, P, n_wg): gate pre-activations scaled to +-100
HEAD_NAMES = ('dY', 'dW', 'db', 'dbl')


def head_id(c):
  return 'B%d_N%d_P%d_wg%d_%s' % c


@functools.lru_cache(maxsize=None)
def head_operands(B, N, P, gate100=False):
  """X [B,32,128] post-ReLU with exact zeros on the real rows and finite non-zero values on every row
  outside the mask (holes, the rows from the node count to 31: the forward leaves bias-driven values in a
  molecule's 4-row padding); mask [B,N] bool; gs [B,P]; W [P+1,128], b [P+1] (output rows, then the gate)."""
  g = torch.Generator().manual_seed(1000 * B + 37 * N + P + (500 if gate100 else 0))
  mask = torch.zeros((B, N), dtype=torch.bool)
  if B < 3:
    mask[:] = True
  else:
    assert N >= 5
    n0 = int(torch.randint(3, N + 1, (1,), generator=g))
    mask[0, 1:n0] = True                                  # a masked node 0
    n1 = int(torch.randint(4, N + 1, (1,), generator=g))
    mask[1, :n1] = True
    mask[1, n1 // 2] = False                              # an interior hole
    #    [2]: an empty mask
    if B > 3:
      mask[3, N - 1] = True                               # the only real node is the last: extent N, count 1
    for b in range(4, B):
      mask[b, :int(torch.randint(1, N + 1, (1,), generator=g))] = True
    if B > 4:
      mask[B - 1, :] = True
  X = torch.relu(torch.randn((B, 32, 128), generator=g))
  junk = 0.25 + torch.randn((B, 32, 128), generator=g).abs()
  real = torch.zeros((B, 32), dtype=torch.bool)
  real[:, :N] = mask
  X = torch.where(real[:, :, None], X, junk)
  W = 0.1 * torch.randn((P + 1, 128), generator=g)
  b = 0.1 * torch.randn((P + 1,), generator=g)
  gs = torch.randn((B, P), generator=g)
  if gate100:
    a = (X.double() @ W[P].double())[real]
    W[P] = (W[P].double() * (100.0 / float(a.abs().max()))).float()
    b[P] = 0.0
  return dict(X=X, mask=mask, gs=gs, W=W, b=b)


def head_gate_preactivations(o):
  """float64 gate pre-activations of the real rows"""
  P = o['gs'].shape[1]
  N = o['mask'].shape[1]
  return (o['X'][:, :N].double() @ o['W'][P].double() + o['b'][P].double())[o['mask']]


def head_eval(o, dtype, draw):
  """Autograd through the reference's read-out (model/lanczos_net.py:185-194): y = (W_o x + b_o) *
  sigmoid(w_g x + b_g), score_b = mean of y over the masked nodes, cotangent gs; dY = dL/dx through the
  ReLU that made x, dbl its column sums.  A molecule with an empty mask is left out (its score is 0 / 0 in
  the reference): its dY is zero, the parameter gradients are those of the batch without it."""
  mask, P = o['mask'], o['gs'].shape[1]
  B, N = mask.shape
  pb, pn = _perm(draw, B, 1), _perm(draw, N, 2)
  X = o['X'][:, :N].to(dtype)[pb][:, pn]
  mp, gp = mask[pb][:, pn], o['gs'].to(dtype)[pb]
  live = mp.any(dim=1)
  Xl = X[live].clone().requires_grad_(True)
  W = o['W'].to(dtype).clone().requires_grad_(True)
  b = o['b'].to(dtype).clone().requires_grad_(True)
  Z = Xl @ W.t() + b
  y = Z[..., :P] * torch.sigmoid(Z[..., P:])
  mk = mp[live].to(dtype).unsqueeze(2)
  score = (y * mk).sum(dim=1) / mk.sum(dim=1)
  gX, gW, gb = torch.autograd.grad(score, [Xl, W, b], gp[live])
  dYp = torch.zeros((B, N, 128), dtype=dtype)
  dYp[live] = gX * (Xl.detach() > 0)
  tmp = torch.empty_like(dYp)
  tmp[:, pn] = dYp
  dY = torch.empty_like(dYp)
  dY[pb] = tmp
  return dict(dY=dY, dW=gW, db=gb, dbl=dYp.sum(dim=(0, 1)))


@functools.lru_cache(maxsize=None)
def head_reference(B, N, P, gate100=False):
  o = head_operands(B, N, P, gate100)
  return reference(lambda dtype, draw: head_eval(o, dtype, draw))


# ------------------------------------------------------------------------------------- filter MLP
DIST8 = [1, 2, 3, 5, 7, 10, 20, 30]
KINK_MARGIN = 1e-5
KINK_CAP = 0.05
MLP_NAMES = ('dW0', 'db0', 'dW2', 'db2', 'dW4', 'db4', 'dW6', 'db6')


def mlp_dist(S):
  """S powers, the power 30 among them (odd and even ones from S = 2)"""
  return DIST8[:S - 1] + [30]


# (live rows R, parts, conv layers L, S, live-row list: None | 'asc' | 'shuffled')
_MLP_MAIN = [(1, 1, 1), (63, 1, 2), (64, 1, 16), (65, 1, 2), (129, 1, 2), (129, 3, 1), (65, 5, 2)]
MLP_CASES = []
for _R, _parts, _L in _MLP_MAIN:
  MLP_CASES.append((_R, _parts, _L, 8, None))
  MLP_CASES.append((_R, _parts, _L, 8, 'shuffled' if (_R, _parts) == (129, 1) else 'asc'))
MLP_CASES += [(65, 2, 2, _S, 'asc') for _S in range(1, 8)]    # every S (8: above)


def mlp_id(c):
  return 'R%d_p%d_L%d_S%d_%s' % (c[0], c[1], c[2], c[3], 'all' if c[4] is None else 'list' if c[4] == 'asc' else c[4])


@functools.lru_cache(maxsize=None)
def mlp_operands(R, parts, L, S, live):
  """D [B,K], dist, layers (per conv layer the four (weight, bias) pairs of its S-128-128-128-S filter MLP),
  dG [L, B K, S], rows = None or (list [B K] int32, count) — a strict subset of the rows, ascending or
  shuffled, its unused tail pointing at a row whose D and dG are NaN —, idx = the live rows in list order,
  kink = the share of (layer, row) pairs whose incoming gradient was zeroed (see mlp_off_the_kink)."""
  seed = 100000 + 1000 * R + 100 * parts + 10 * L + S + (5000 if live else 0)
  rs = np.random.RandomState(seed)
  dist = mlp_dist(S)
  if live is None:
    B, K = R, 1
    idx = np.arange(R)
    poison = None
  else:
    K = 4
    B = (R + 11) // 4 + 1
    pick = rs.permutation(B * K)
    idx, poison = pick[:R], int(pick[R])
    if live == 'asc':
      idx = np.sort(idx)
    else:
      assert R > 2 and not (np.diff(idx) > 0).all()
  D = (rs.rand(B * K) * 1.9 - 0.95).astype(np.float32)           # |lambda(L4)| <= 1
  special = np.array([0.0, 1.0, -1.0, 1e-3, -1e-3, 0.05, -0.05], np.float32)   # (1e-3, 0.05: ^30 underflows)
  if R >= len(special):
    D[idx[:len(special)]] = special
  layers = [[(torch.from_numpy((rs.randn(o, i) / np.sqrt(i)).astype(np.float32)),
              torch.from_numpy((0.1 * rs.randn(o)).astype(np.float32)))
             for (o, i) in ((128, S), (128, 128), (128, 128), (S, 128))] for _ in range(L)]
  dG = rs.randn(L, B * K, S).astype(np.float32)
  rows = None
  if live is not None:
    buf = np.full(B * K, poison, np.int32)
    buf[:R] = idx
    rows = (torch.from_numpy(buf), R)
    D[poison] = np.nan
    dG[:, poison] = np.nan
  o = dict(D=torch.from_numpy(D).view(B, K), dist=dist, layers=layers, dG=torch.from_numpy(dG), rows=rows,
           idx=torch.from_numpy(idx.astype(np.int64)))
  o['kink'] = mlp_off_the_kink(o)
  return o


def mlp_off_the_kink(o, margin=KINK_MARGIN):
  """Zero the incoming gradient of every (layer, live row) in which some hidden unit's float64
  pre-activation lies within `margin` of the ReLU kink: such a unit may take either side in float32, in
  the kernel and in the float32 reference alike, and float64 is an oracle only off the kink
  (tests/test_gpu_mlp_grad.py).  The row still runs through the kernel.  -> the share of pairs zeroed."""
  x = o['D'].reshape(-1)[o['idx']].double()
  feats = torch.stack([torch.pow(x, p) for p in o['dist']], dim=1)
  zeroed = 0
  for l, lins in enumerate(o['layers']):
    h = feats
    near = torch.zeros(h.shape[0], dtype=torch.bool)
    for (w, b) in lins[:3]:
      z = h @ w.double().t() + b.double()
      near |= (z.abs() < margin).any(dim=1)
      h = torch.relu(z)
    o['dG'][l, o['idx'][near]] = 0.0
    zeroed += int(near.sum())
  return zeroed / float(len(o['layers']) * o['idx'].numel())


def mlp_eval(o, dtype, draw):
  """Autograd through the reference's nn.Sequential (model/lanczos_net.py:95-123, 146-149) on the live rows,
  cotangent dG: {'<tensor>/<layer>': gradient}."""
  idx = o['idx'][_perm(draw, o['idx'].numel(), 3)]
  x = o['D'].reshape(-1)[idx].to(dtype)
  feats = torch.stack([torch.pow(x, p) for p in o['dist']], dim=1)
  out = {}
  for l, lins in enumerate(o['layers']):
    ps = [t.to(dtype).clone().requires_grad_(True) for wb in lins for t in wb]
    h = feats
    for i in range(4):
      h = h @ ps[2 * i].t() + ps[2 * i + 1]
      if i < 3:
        h = torch.relu(h)
    g = torch.autograd.grad(h, ps, o['dG'][l][idx].to(dtype))
    for name, t in zip(MLP_NAMES, g):
      out['%s/%d' % (name, l)] = t
  return out


@functools.lru_cache(maxsize=None)
def mlp_reference(R, parts, L, S, live):
  o = mlp_operands(R, parts, L, S, live)
  return reference(lambda dtype, draw: mlp_eval(o, dtype, draw))


# ---------------------------------------------------------------------------------- gain gradient
# name: molecules (node counts, batch order), K, long scales S, conv layers, input width, and the ONE strip
# the batch must make on a one-unit plan: subtiles, whether a molecule straddles two of them.
# form: what lnz_lanczosnet_gain_grad must take on that plan ('strip', or 'tile': more than 12 long scales).
GAIN_CASES = {
    'one_node_B1':     dict(mols=[1], K=20, S=8, layers=2, din=64, sub=1, straddle=False, form='strip'),
    'sub1_K7':         dict(mols=[8, 4, 3], K=7, S=8, layers=2, din=64, sub=1, straddle=False, form='strip'),
    'sub2_straddle_S1': dict(mols=[12, 9, 5], K=20, S=1, layers=2, din=64, sub=2, straddle=True, form='strip'),
    'sub3_din48':      dict(mols=[20, 14, 10], K=20, S=8, layers=2, din=48, sub=3, straddle=True, form='strip'),
    'sub4_din128':     dict(mols=[32, 17, 11], K=20, S=8, layers=2, din=128, sub=4, straddle=True, form='strip'),
    'sub5_B5_L1':      dict(mols=[32, 30, 5, 3, 2], K=20, S=8, layers=1, din=64, sub=5, straddle=True, form='strip'),
    'sub6_S12':        dict(mols=[32, 32, 29], K=20, S=12, layers=2, din=64, sub=6, straddle=True, form='strip'),
    'mol24_K1':        dict(mols=[1 + (i % 4) for i in range(24)], K=1, S=8, layers=2, din=64, sub=6,
                            straddle=False, form='strip'),
    'n32_K32':         dict(mols=[32], K=32, S=8, layers=2, din=64, sub=2, straddle=True, form='strip'),
    'S13_tile':        dict(mols=[12, 9, 5], K=20, S=13, layers=2, din=64, sub=2, straddle=True, form='tile'),
    'S16_tile_L1':     dict(mols=[20, 14, 10], K=20, S=16, layers=1, din=128, sub=3, straddle=True, form='tile'),
}


def gain_cfg(name):
  """the module configuration of a case (the QM8 one with the case's sizes)"""
  import oracle
  c = GAIN_CASES[name]
  return dict(oracle.DEFAULT_QM8_CFG, num_layer=c['layers'], hidden_dim=[128] * c['layers'],
              long_diffusion_dist=list(range(1, c['S'] + 1)), num_eig_vec=c['K'], input_dim=c['din'])


def gain_padded_width(din):
  """LanczosNet._plan's rule for hidden width 128: the input width in 64-column groups"""
  return (din + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def gain_operands(name):
  """mask [B,N] uint8 (N = the largest molecule), V [B,N,K] with orthonormal columns on a molecule's own
  rows and slots (zero at rows >= n and slots >= n), act / dy [L,B,32,128], x0 [B,32,padded width] — all
  zero at rows >= n and x0 in the padding columns —, params: oracle.make_lanczosnet_params of gain_cfg."""
  import oracle
  c = GAIN_CASES[name]
  mols, K, Lnum = c['mols'], c['K'], c['layers']
  B, N = len(mols), max(mols)
  g = torch.Generator().manual_seed(sum(ord(ch) for ch in name))
  n = torch.tensor(mols)
  mask = (torch.arange(N)[None, :] < n[:, None]).to(torch.uint8)
  V = torch.zeros((B, N, K))
  for b, nb in enumerate(mols):
    q, _ = torch.linalg.qr(torch.randn((nb, nb), generator=g, dtype=torch.float64))
    V[b, :nb, :min(nb, K)] = q[:, :min(nb, K)].float()
  rows = (torch.arange(32)[None, :] < n[:, None]).float()
  dinp = gain_padded_width(c['din'])
  act = torch.rand((Lnum, B, 32, 128), generator=g) * rows[None, :, :, None]
  dy = torch.randn((Lnum, B, 32, 128), generator=g) * rows[None, :, :, None]
  x0 = torch.randn((B, 32, dinp), generator=g) * rows[:, :, None]
  x0[:, :, c['din']:] = 0.0
  params = oracle.make_lanczosnet_params(gain_cfg(name), 3)
  return dict(mask=mask, n=n, V=V, act=act, dy=dy, x0=x0, params=params)


def gain_eval(o, name, dtype, draw):
  """dG[l][b][k][s] = sum_o (V^T dY_l)[k][o] ((V^T X_l) W_{l,s}^T)[k][o], W_{l,s} the column block of the
  raw `filter.l.weight` of long channel s in the reference's channel order [short | long | edge types]
  (model/lanczos_net.py:157-181; no short scales here, so block s): {'dG/<layer>': [B,K,S]}."""
  c = GAIN_CASES[name]
  S, din = c['S'], c['din']
  B, N, K = o['V'].shape
  pb, pn = _perm(draw, B, 4), _perm(draw, N, 5)
  V = o['V'].to(dtype)[pb][:, pn]
  Vt = V.transpose(1, 2)
  out = {}
  for la in range(c['layers']):
    X = (o['x0'][:, :N, :din] if la == 0 else o['act'][la - 1][:, :N]).to(dtype)[pb][:, pn]
    dY = o['dy'][la][:, :N].to(dtype)[pb][:, pn]
    d = X.shape[2]
    W = torch.from_numpy(o['params']['filter.%d.weight' % la]).to(dtype).view(128, -1, d)[:, :S, :]
    Q = torch.einsum('bki,osi->bkso', torch.bmm(Vt, X), W)
    dG = (Q * torch.bmm(Vt, dY).unsqueeze(2)).sum(dim=3)
    un = torch.empty_like(dG)
    un[pb] = dG
    out['dG/%d' % la] = un
  return out


@functools.lru_cache(maxsize=None)
def gain_reference(name):
  o = gain_operands(name)
  return reference(lambda dtype, draw: gain_eval(o, name, dtype, draw))


def strip_shape(plan):
  """(strips, subtiles of the first, molecules of the first, a molecule straddles two subtiles) of a strip
  plan in strip_mirror's form [(molecules [(b, first row, extent)], subtiles)]"""
  mols, sub = plan[0]
  straddle = any(st // 16 != (st + (4 if n <= 4 else (n + 3) // 4 * 4) - 1) // 16 for _, st, n in mols)
  return len(plan), int(sub), len(mols), straddle
