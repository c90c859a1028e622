"""Cases, host-drawn operands and float64 / float32 references of the fused inference forward for graphs of
at most 32 nodes, shared by tests/test_forward_cases_cpu.py (no GPU), tests/test_gpu_strip_forward_edges.py,
tests/test_gpu_tile_forward_edges.py and tools/forward_reference_spread.py:

  lanczosnet_strip_kernel    (csrc/conv_strip.hip)    STRIP_CASES  (geometry at the QM8 shape, model envelope)
  lanczosnet_forward_kernel  (csrc/conv_forward.hip)  TILE_CASES

Everything a case feeds the kernel is drawn on the host (forward_operands): connected graphs, L from
oracle.laplacian_multi_l4 in float64 rounded once, V from oracle.graph_laplacian_eigs + collate_eigs rounded
once, the gains G (or the dense symmetric filters DD) drawn normal — not an MLP output —, the parameters of
oracle.make_lanczosnet_params.  forward_eval is written from the reference's formulas
(model/lanczos_net.py:143-197: messages [short | long | edge types], X' = relu(cat(M_c X) W^T + b), the gated
head, the mean over the nodes the mask keeps) and takes G / DD as an operand.  Draw 0 evaluates the operands as
given, draws 1..7 permute the molecules and every molecule's nodes consistently and un-permute the results;
train_kernel_cases.reference gives the truth (float64), e32 (the worst of the eight float32 evaluations in units
of max|truth|) and the spread.  The kernel must be within bar(e32, k) of max|truth| per tensor; k is the
project's 4 unless a case is listed in K_FORWARD_CASE.  For gemm_mode 'f16x3' the yardstick is e_split: the same
eight evaluations with every operand of a conv-layer product rounded to fp16 hi + lo pieces first.  No kernel
output enters a bar."""
import functools

import numpy as np
import torch

from train_kernel_cases import ULP, bar, _perm, reference  # noqa: F401

K_FORWARD = 4.0
# cases whose eight float32 evaluations differ by more than 4 (tools/forward_reference_spread.py): name -> k
K_FORWARD_CASE = {}
BAR_CAP = 5e-6            # every bar of this file is at most half the 1e-5 the forward kernels are held to elsewhere
SPLIT_HEADER_BAR = 1e-5   # include/lanczosnet_hip.h: the parity bar of gemm_mode 1

RARE = 'lanczosnet_strip_kernel<0,0,1,false,false>'
PLAIN = 'lanczosnet_strip_kernel<0,0,false,false>'
SHORT = 'lanczosnet_strip_kernel<0,0,true,false>'
DENSE = 'lanczosnet_strip_kernel<0,2,false,false>'
DENSE_SHORT = 'lanczosnet_strip_kernel<0,2,true,false>'
SPLIT = 'lanczosnet_strip_kernel<0,0,false,true>'
TILE = 'lanczosnet_forward_kernel<%d,10,%d,0,%d>'

QM8 = dict(layers=7, K=20, S=8, n_edge=7, din=64, dhid=128, dout=16)
ENV = dict(layers=2, K=20, S=3, n_edge=4, din=64, dhid=128, dout=5)
ENV_MOLS = [12, 9, 5, 8, 3, 14]


def forward_k(name):
  return K_FORWARD_CASE.get(name, K_FORWARD)


def _case(base, mols, kernel, **over):
  c = dict(base, mols=list(mols), kernel=kernel, short=[], general=False, dense=False, gemm='fp32', n_cu=1,
           seams=(), special=None, act=False, plain=(), seed=0)
  c.update(over)
  # strips of the default launch that take the folded form of the rare bond-type channels (decided per strip
  # on the device; flop_model.strip_takes_rare on the host-drawn L must give the same: expected_rare_strips)
  c.setdefault('rare_strips', 1 if kernel == RARE and not c['act'] else 0)
  return c


# ------------------------------------------------------------------------------------------ strips
# Geometry (the QM8 shape, one-unit plan unless n_cu says otherwise): `seams` is what the strip plan of the
# case's extents must contain (strip_seams below), asserted on the CPU through strip_mirror and on the GPU from
# the plan the device made.  Each case runs in the default form and through the channel loop (fold=False).
# (S = 8 long scales, bench.py's QM8 configuration, where the issue's text says three: the timed shape.)
# Every strip of at most five subtiles must take the folded form in the default launch (rare_strips).
STRIP_GEOMETRY = {
    'h1_pad5':       _case(QM8, [5, 3], RARE, seams=('h1', 'pad5', 'tail_dead', 'mols_in_subtile_2')),
    'h2_B1_n32':     _case(QM8, [32], RARE, seams=('h2', 'B1', 'two_full_subtiles')),
    'h2_two_across': _case(QM8, [12, 6], RARE, seams=('h2', 'start12', 'two_rows_across', 'straddle')),
    'h3_row4':       _case(QM8, [20, 12, 8], RARE, seams=('h3', 'start4', 'straddle')),
    'h3_row12':      _case(QM8, [28, 20], RARE, seams=('h3', 'start12', 'rows12_31', 'straddle')),
    'h4_row8':       _case(QM8, [20, 12, 24, 8], RARE, seams=('h4', 'start8', 'start12', 'straddle')),
    'h5_skip':       _case(QM8, [28, 24, 12, 3], RARE, seams=('h5', 'skip_dead', 'tail_dead', 'straddle')),
    'h6_plain':      _case(QM8, [32, 32, 29], RARE, seams=('h6', 'straddle'), rare_strips=0),
    'h6_mol24':      _case(QM8, [1 + (i % 4) for i in range(24)], RARE,
                           seams=('h6', 'mol24', 'n1', 'n2', 'n3', 'n4', 'mols_in_subtile_3'), rare_strips=0),
    'h2_three':      _case(QM8, [4, 4, 7, 4, 3], RARE, seams=('h2', 'mols_in_subtile_3', 'tail_dead')),
    'two_heights':   _case(QM8, [32, 32, 32, 30, 6], RARE, n_cu=2, seams=('two_heights', 'h4', 'h5'),
                           rare_strips=2),
}

# Model envelope (two layers unless the case says otherwise), one strip each.
STRIP_ENVELOPE = {
    'K1':        _case(ENV, ENV_MOLS, RARE, K=1),
    'K3':        _case(ENV, ENV_MOLS, RARE, K=3),
    'K20':       _case(ENV, ENV_MOLS, RARE),
    'K32':       _case(ENV, ENV_MOLS + [32], RARE, K=32, rare_strips=0),       # six subtiles: the channel loop
    'K4_dense':  _case(ENV, ENV_MOLS, DENSE, K=4, dense=True),
    'K20_dense': _case(ENV, ENV_MOLS, DENSE, dense=True),
    'K32_dense': _case(ENV, ENV_MOLS + [32], DENSE, K=32, dense=True),
    'dense_short': _case(ENV, ENV_MOLS, DENSE_SHORT, dense=True, short=[2]),
    'long0':     _case(ENV, ENV_MOLS, RARE, S=0),
    'long1':     _case(ENV, ENV_MOLS, RARE, S=1),
    'long12':    _case(ENV, ENV_MOLS, RARE, S=12),
    'short1':    _case(ENV, ENV_MOLS, SHORT, short=[3]),
    'short8':    _case(ENV, ENV_MOLS, SHORT, short=[1, 2, 3, 4, 5, 6, 7, 8]),
    'edge1':     _case(ENV, ENV_MOLS, PLAIN, n_edge=1),
    'edge2':     _case(ENV, ENV_MOLS, PLAIN, n_edge=2),
    # one folded channel folds only when it touches no row at all (no bond of its type, no node the mask leaves
    # out): edge3 runs the channel loop inside the rare-capable launch, edge3_fold the folded form
    'edge3':     _case(ENV, ENV_MOLS, RARE, n_edge=3, rare_strips=0),
    'edge3_fold': _case(ENV, [12, 9, 5], RARE, n_edge=3, special='no_rare_bonds'),
    'edge7':     _case(ENV, ENV_MOLS, RARE, n_edge=7),           # the largest strip_rare_eligible accepts
    'edge8':     _case(ENV, ENV_MOLS, PLAIN, n_edge=8),
    'edge29_32channels': _case(ENV, ENV_MOLS, PLAIN, n_edge=29),   # 3 long + 29 = 32 channels in all
    'din128':    _case(ENV, ENV_MOLS, RARE, din=128),
    'general1':  _case(ENV, ENV_MOLS, RARE, din=1, general=True),    # padded to 64
    'general65': _case(ENV, ENV_MOLS, RARE, din=65, general=True),   # padded to 128
    'dout1':     _case(ENV, ENV_MOLS, RARE, dout=1, seed=3),
    'dout31':    _case(ENV, ENV_MOLS, RARE, dout=31),
    'layer1':    _case(ENV, ENV_MOLS, RARE, layers=1),
    'layer16':   _case(ENV, ENV_MOLS, RARE, layers=16),
    # dense channels touch every row: never cheaper folded, the strip keeps the channel loop
    'any_operator': _case(ENV, ENV_MOLS, RARE, n_edge=5, special='any_operator', rare_strips=0),
    # non-symmetric entries without a mirror on top of the bond-type channels: the folded form on an operator
    # that is no Laplacian (a row is touched through its row OR its column)
    'sparse_operator': _case(ENV, ENV_MOLS, RARE, n_edge=5, special='sparse_operator'),
    'any_V':     _case(ENV, ENV_MOLS, RARE, special='any_V'),
    'train_act': _case(ENV, [28, 20, 9, 5, 3], PLAIN, n_edge=7, S=8, act=True),   # act_out: every act/l
    'split':     _case(ENV, ENV_MOLS, SPLIT, gemm='f16x3'),
    # (two layers: at three the yardstick's own bar, 4 e_split = 4.7e-6 .. 4.8e-6 depending on the host's BLAS
    # threading, leaves no margin under the 5e-6 cap)
    'split_qm8_channels': _case(ENV, [28, 20, 9, 5], SPLIT, gemm='f16x3', S=8, n_edge=7),
}
STRIP_CASES = dict(STRIP_GEOMETRY, **STRIP_ENVELOPE)

# ------------------------------------------------------------------------------------------- tiles
# The five instantiations of lanczosnet_forward_kernel: (waves per half, filter kind, ring depth) and a model
# that reaches it once the launch carries no strip plan.
TILE_MODELS = {
    'w128_in32':  dict(dhid=128, din=32, dense=False, kernel=TILE % (4, 0, -1)),
    'w64':        dict(dhid=64, din=32, dense=False, kernel=TILE % (2, 0, -1)),
    'w128_in64':  dict(dhid=128, din=64, dense=False, kernel=TILE % (4, 0, 1)),
    'w128_dense': dict(dhid=128, din=64, dense=True, kernel=TILE % (4, 2, 0)),
    'w64_dense':  dict(dhid=64, din=32, dense=True, kernel=TILE % (2, 2, 0)),
}
# geometry -> (molecules, tiling, what the tile plan must contain)
TILE_GEOMETRY = {
    'none_B1': ([11], 'none', ()),
    'none_B4': ([11, 32, 5, 17], 'none', ()),
    'none_B5': ([11, 32, 5, 17, 1], 'none', ()),               # a second workgroup with one molecule
    'single':  ([8, 20, 16, 12, 32, 3], 'single', ('single',)),
    'auto':    ([8, 20, 16, 12, 32], 'auto', ('pair8_exact', 'pair16', 'lone32')),
}
TILE_CASES = {}
for _m, _mod in TILE_MODELS.items():
  for _g, (_mols, _tiling, _seams) in TILE_GEOMETRY.items():
    # (the 8-node molecule of the 8|24 pair keeps its eight nodes: no masked last node there)
    TILE_CASES['%s/%s' % (_m, _g)] = _case(ENV, _mols, _mod['kernel'], dhid=_mod['dhid'], din=_mod['din'],
                                            dense=_mod['dense'], tiling=_tiling, seams=_seams, plain=(0,))
for _m in TILE_MODELS:     # (width 128 with dense filters and K % 4 != 0: the strip launcher refuses it)
  for _K in (1, 3, 32):
    _mod = TILE_MODELS[_m]
    TILE_CASES['%s/K%d' % (_m, _K)] = _case(ENV, [8, 20, 16, 12, 32], _mod['kernel'], dhid=_mod['dhid'],
                                            din=_mod['din'], dense=_mod['dense'], tiling='auto', K=_K, plain=(0,),
                                            seams=('pair8_exact', 'pair16', 'lone32'))

CASES = dict(STRIP_CASES, **TILE_CASES)


def case_cfg(name):
  """the module configuration of a case"""
  c = CASES[name]
  return dict(num_atom=70, num_bond_type=c['n_edge'] - 1, short_diffusion_dist=list(c['short']),
              long_diffusion_dist=list(range(1, c['S'] + 1)), num_eig_vec=c['K'],
              spectral_filter_kind='None' if c['dense'] else 'MLP', input_dim=c['din'],
              hidden_dim=[c['dhid']] * c['layers'], output_dim=c['dout'], num_layer=c['layers'])


# ---------------------------------------------------------------------------------------- operands
def _graph(rs, n, n_types, rare=True):
  """a random spanning tree plus extra bonds, dealt over the bond types: (simple adjacency, typed [n,n,E])"""
  A = np.zeros((n, n))
  T = np.zeros((n, n, max(n_types, 0)))
  bonds = [(int(rs.randint(0, i)), i) for i in range(1, n)]
  for _ in range(n // 4):
    i, j = (int(x) for x in rs.randint(0, n, size=2))
    if i != j and (min(i, j), max(i, j)) not in bonds:
      bonds.append((min(i, j), max(i, j)))
  for i, j in bonds:
    A[i, j] = A[j, i] = 1.0
    if n_types > 0:
      # (type 0 most of the time: the rare types touch few rows, as in QM8)
      t = 0 if rs.rand() < 0.6 or not rare else int(rs.randint(0, n_types))
      T[i, j, t] = T[j, i, t] = 1.0
  return A, T


def _special_molecules(c):
  """(masked last node, interior hole, masked node 0): three different molecules of a batch of >= 4, or Nones.
  The masked last node stays inside the rows the kernels give its molecule (4-row padding), as in
  test_nodes_the_mask_leaves_out_but_the_operator_keeps; the extent the planner sees drops by one."""
  mols = c['mols']
  if len(mols) < 4:
    return None, None, None
  free = [b for b in range(len(mols)) if b not in c['plain']]
  last = next(b for b in free if mols[b] >= 3 and mols[b] % 4 != 1)
  hole = next(b for b in free if mols[b] >= 3 and b != last)
  zero = next(b for b in free if mols[b] >= 2 and b not in (last, hole))
  return last, hole, zero


def case_mask(name):
  c = CASES[name]
  mols = c['mols']
  mask = (np.arange(max(mols))[None, :] < np.array(mols)[:, None]).astype(np.uint8)
  last, hole, zero = _special_molecules(c)
  if last is not None:
    mask[last, mols[last] - 1] = 0
    mask[hole, mols[hole] // 2] = 0
    mask[zero, 0] = 0
  return mask


def case_extents(name):
  """last kept node + 1: what the planners see"""
  m = case_mask(name)
  return (m * np.arange(1, m.shape[1] + 1)).max(axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def forward_operands(name):
  """numpy / torch operands of a case: L [B,N,N,C] f32, V [B,N,K] f32, G [layers,B,S,K] (or DD
  [layers,B,S,K,K] symmetric) f32, feat (int64 [B,N] atom ids or f32 [B,N,din]), mask [B,N] u8, ext [B],
  params (oracle.make_lanczosnet_params), cfg."""
  import oracle
  c = CASES[name]
  cfg = case_cfg(name)
  rs = np.random.RandomState((sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 7919 * c['seed']) % (2 ** 31))
  mols, K, S, C_ = c['mols'], c['K'], c['S'], c['n_edge']
  B, N = len(mols), max(mols)
  mask = case_mask(name)
  ext = case_extents(name)
  L = np.zeros((B, N, N, C_))
  V = np.zeros((B, N, K), np.float32)
  for b, n in enumerate(mols):
    A, T = _graph(rs, n, C_ - 1, rare=c['special'] != 'no_rare_bonds')
    if C_ > 1:
      L[b, :n, :n] = oracle.laplacian_multi_l4(T)
    else:
      L[b, :n, :n, 0] = oracle.laplacian_l4(A)
    if c['special'] == 'any_operator':
      L[b, :n, :n, 1:] = rs.randn(n, n, C_ - 1) / np.sqrt(n)     # dense, non-symmetric
    if c['special'] == 'sparse_operator' and n >= 3:
      for ch in range(2, C_):
        i, j = (int(x) for x in rs.choice(n, size=2, replace=False))
        L[b, i, j, ch] += 0.25 + rs.rand()                         # (L[b, j, i, ch] stays as it is)
    e = int(ext[b])
    if e == n:
      d, v, _ = oracle.graph_laplacian_eigs(A, graph_laplacian_type='L4')
    else:  # the kernels' slot count is the extent: Ritz pairs of the block the mask keeps
      w, v = np.linalg.eigh(L[b, :e, :e, 0])
      order = np.argsort(-np.abs(w), kind='mergesort')
      d, v = w[order], v[:, order]
    _, Vb = oracle.collate_eigs([d], [v], N, K)
    V[b] = Vb[0]
    if c['special'] == 'any_V':
      kk = min(e, K)
      V[b, :e, :kk] = rs.randn(e, kk).astype(np.float32) / np.sqrt(e)
  L = L.astype(np.float32)
  if c['dense']:
    DD = 0.5 * rs.randn(c['layers'], B, S, K, K)
    G = (0.5 * (DD + DD.transpose(0, 1, 2, 4, 3))).astype(np.float32)
  else:
    G = (0.5 * rs.randn(c['layers'], B, S, K)).astype(np.float32)
  if c['general']:
    feat = rs.randn(B, N, c['din']).astype(np.float32)          # every row, padding included
  else:
    feat = rs.randint(0, 70, size=(B, N)).astype(np.int64)
  params = oracle.make_lanczosnet_params(cfg, 3, general=c['general'])
  return dict(L=L, V=V, G=G, feat=feat, mask=mask, ext=ext, params=params, cfg=cfg)


def _split_round(x):
  """x as the fp16 pieces hi + lo the split-precision products see"""
  hi = x.half().to(x.dtype)
  return hi + (x - hi).half().to(x.dtype)


def forward_eval(o, dtype, draw, split=False, G=None):
  """The reference model's forward in `dtype` on the CPU: {'score' [B,P], 'state' (final node state, the rows
  the mask keeps, concatenated in batch order), 'act/<l>' (every layer's post-ReLU state, the same rows)}.
  split: every operand of a conv-layer product (X, W, L, V and the messages) rounded to fp16 hi + lo first —
  the products include/lanczosnet_hip.h lists as split; gains, biases and the head stay exact.  G: the gains
  to use instead of the operands' (the dead-slot contract)."""
  cfg = o['cfg']
  q = _split_round if split else (lambda x: x)
  mask = torch.from_numpy(o['mask']).bool()
  B, N = mask.shape
  pb = _perm(draw, B, 11)
  rows = torch.stack([_perm(draw, N, 100 + int(b)) for b in range(B)])[pb]      # [B,N] node order per slot
  bi = pb[:, None]
  L = q(torch.from_numpy(o['L']).to(dtype)[bi[:, :, None], rows[:, :, None], rows[:, None, :]])
  V = q(torch.from_numpy(o['V']).to(dtype)[bi, rows])
  Gt = torch.from_numpy(o['G'] if G is None else G).to(dtype)[:, pb]
  mk = mask[bi, rows]
  P = {k: torch.from_numpy(v).to(dtype) for k, v in o['params'].items()}
  feat = torch.from_numpy(o['feat'])[bi, rows]
  state = feat.to(dtype) if feat.dtype != torch.int64 else P['embedding.weight'][feat]      # :154
  short = list(cfg['short_diffusion_dist'])
  S, E1 = len(cfg['long_diffusion_dist']), cfg['num_bond_type'] + 1
  acts = []
  for l in range(cfg['num_layer']):
    X = q(state)
    msg = []
    tmp = X
    for p in range(1, max(short, default=0) + 1):                                # :164-169
      tmp = q(L[..., 0] @ tmp)
      if p in short:
        msg.append(tmp)
    for s in range(S):                                                           # :114-117, :172-174
      g = Gt[l, :, s]
      Ls = (V @ g @ V.transpose(1, 2)) if g.dim() == 3 else ((V * g[:, None, :]) @ V.transpose(1, 2))
      msg.append(q(Ls) @ X)
    for e in range(E1):                                                          # :177-178
      msg.append(L[..., e] @ X)
    cat = q(torch.cat(msg, dim=2))                                               # :180
    state = torch.relu(cat @ q(P['filter.%d.weight' % l]).t() + P['filter.%d.bias' % l])      # :181
    acts.append(state)
  nl = cfg['num_layer']
  y = state @ P['filter.%d.weight' % nl].t() + P['filter.%d.bias' % nl]          # :186
  y = y * torch.sigmoid(state @ P['att_func.0.weight'].t() + P['att_func.0.bias'])      # :187-188
  w = mk.to(dtype).unsqueeze(2)
  score_p = (y * w).sum(dim=1) / w.sum(dim=1)                                    # :190-194
  score = torch.empty_like(score_p)
  score[pb] = score_p
  out = dict(score=score)
  for l, a in enumerate(acts):
    un = torch.empty_like(a)
    un[bi, rows] = a
    out['act/%d' % l] = un[mask]
  out['state'] = out['act/%d' % (nl - 1)]
  return out


@functools.lru_cache(maxsize=None)
def forward_reference(name):
  """(truth, e, spread) of a case; e is e_split for a gemm_mode 'f16x3' case and e32 otherwise"""
  o = forward_operands(name)
  if CASES[name]['gemm'] == 'f16x3':
    truth = forward_eval(o, torch.float64, 0)
    _, e, spread = reference(lambda dtype, draw: truth if dtype == torch.float64
                             else forward_eval(o, dtype, draw, split=True))
    return truth, e, spread
  return reference(lambda dtype, draw: forward_eval(o, dtype, draw))


def forward_bars(name):
  """{tensor: the bar, in units of max|truth|}"""
  _, e, _ = forward_reference(name)
  return {t: bar(v, forward_k(name)) for t, v in e.items()}


# ------------------------------------------------------------------------------------------- seams
def _rows4(n):
  return 4 if n <= 4 else (n + 3) // 4 * 4


def strip_seams(plan):
  """The seams a strip plan holds, as names; plan in strip_mirror's form [(molecules [(b, first row, extent)],
  subtiles)]."""
  found = set()
  if len({int(sub) for _, sub in plan}) > 1:
    found.add('two_heights')
  if sum(len(m) for m, _ in plan) == 1:
    found.add('B1')
  for mols, sub in plan:
    found.add('h%d' % sub)
    taken = np.zeros(16 * int(sub), bool)
    per_sub = np.zeros(int(sub), int)
    for _, st, n in mols:
      r = _rows4(n)
      taken[st:st + r] = True
      if st % 16 in (4, 8, 12):
        found.add('start%d' % (st % 16))
      if st // 16 != (st + r - 1) // 16:
        found.add('straddle')
        if st + n - 16 * (st // 16 + 1) == 2:
          found.add('two_rows_across')       # only two node rows reach into the second subtile
      else:
        per_sub[st // 16] += 1
      if st % 16 == 12 and r == 20:
        found.add('rows12_31')               # ends exactly on a subtile boundary
      if st % 16 == 0 and r == 32:
        found.add('two_full_subtiles')
      if n == 5:
        found.add('pad5')
      if n <= 4:
        found.add('n%d' % n)
    if len(mols) == 24:
      found.add('mol24')
    for k in (2, 3):
      if (per_sub >= k).any():
        found.add('mols_in_subtile_%d' % k)
    end = max(st + _rows4(n) for _, st, n in mols)
    if not taken[:end].all():
      found.add('skip_dead')
    if end < 16 * int(sub):
      found.add('tail_dead')
  return found


def expected_rare_strips(name, plan):
  """Strips of `plan` (strip_mirror's form) that take the folded form in the case's default launch: the
  kernel's cost rule (utils/flop_model.py) on the touched rows of the host-drawn L."""
  from lanczosnet_amd.utils import flop_model as fm
  c = CASES[name]
  if c['kernel'] != RARE or c['act']:
    return 0
  o = forward_operands(name)
  touch = fm.touch_masks(o['L'], o['mask'])
  nf = c['n_edge'] - 2
  took = 0
  for mols, sub in plan:
    cnt = [sum(bin(int(touch[b][2 + f]) & ((1 << _rows4(n)) - 1)).count('1') for b, _, n in mols) for f in range(nf)]
    took += int(fm.strip_takes_rare(int(sub), cnt, nf))
  return took


def plan_from_device(words, n_strips):
  """the int32 words of lnz_plan_strips -> strip_mirror's form"""
  out = []
  for s in range(int(n_strips)):
    e = [int(x) for x in words[80 * s:80 * (s + 1)]]
    out.append(([tuple(e[2 + 3 * i:5 + 3 * i]) for i in range(e[0])], e[1]))
  return out


def tile_seams(words, n_wg, ext):
  """The seams of a tile plan (lnz_plan_tiles: per workgroup 4 slots of (molecule A, molecule B | -1, split
  row)) as names."""
  found = set()
  slots = np.asarray(words[:12 * int(n_wg)]).reshape(-1, 3)
  used = slots[slots[:, 0] >= 0]
  if len(used) and (used[:, 1] < 0).all():
    found.add('single')
  for ta, tb, split in used:
    if tb >= 0 and split == 8 and ext[ta] == 8 and 16 < ext[tb] <= 24:
      found.add('pair8_exact')
    if tb >= 0 and split == 16:
      found.add('pair16')
    if tb < 0 and ext[ta] == 32:
      found.add('lone32')
  return found


def reorder_operands(o, order, N):
  """the operands with the molecules in `order` (indices into the batch) and the node axis padded to N"""
  B, N0 = len(order), o['mask'].shape[1]
  assert N >= N0
  L = np.zeros((B, N, N, o['L'].shape[3]), np.float32)
  L[:, :N0, :N0] = o['L'][order]
  V = np.zeros((B, N, o['V'].shape[2]), np.float32)
  V[:, :N0] = o['V'][order]
  feat = np.zeros((B, N) + o['feat'].shape[2:], o['feat'].dtype)
  feat[:, :N0] = o['feat'][order]
  mask = np.zeros((B, N), np.uint8)
  mask[:, :N0] = o['mask'][order]
  return dict(o, L=L, V=V, G=np.ascontiguousarray(o['G'][:, order]), feat=feat, mask=mask, ext=o['ext'][order])


def poisoned_gains(name, value):
  """the case's G (or DD) with every slot k >= extent of its molecule set to `value`"""
  c = CASES[name]
  o = forward_operands(name)
  dead = np.arange(c['K'])[None, :] >= np.minimum(o['ext'], c['K'])[:, None]
  assert dead.any()
  G = o['G'].copy()
  if c['dense']:
    G[:, dead[:, None, :, None] | dead[:, None, None, :] | np.zeros_like(G[0], bool)] = value
  else:
    G[:, dead[:, None, :] | np.zeros_like(G[0], bool)] = value
  return G


# ------------------------------------------------------------------------------------- device side
# (used by the two GPU files only; nothing above imports the package)
_NETS = {}


def device_model(name):
  """one module per configuration, its plan cached by the module"""
  c = CASES[name]
  cfg = case_cfg(name)
  key = (repr(sorted(cfg.items())), c['general'], c['dense'], c['gemm'])
  if key not in _NETS:
    from lanczosnet_amd.model import LanczosNet, LanczosNetGeneral
    from lanczosnet_amd.utils.arg_helper import make_model_config
    cls = LanczosNetGeneral if c['general'] else LanczosNet
    net = cls(make_model_config(cfg, general=c['general'])).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in forward_operands(name)['params'].items()})
    net = net.to('cuda')
    if c['dense']:
      net.filter_kind = 1          # the dense filters of AdaLanczosNet as an operand of this forward
    net.gemm_mode = c['gemm']
    _NETS[key] = net
  return _NETS[key]


def narrow_plan(net, plan):
  """The module pads a width-128 model's input to 64 columns; the kernel's own limit is 32 (hidden width 128
  with input width 32 is lanczosnet_forward_kernel<4,10,0,0,-1>): the same plan with layer 0 packed unpadded."""
  from lanczosnet_amd import ops
  assert plan['din0_raw'] == 32 and plan['din0'] == 64 and plan['num_layer'] > 1 and plan['dhid'] == 128
  wp0 = ops.pack_rows_k8(net._mix_weight(0).detach().float().contiguous())
  old1 = int(plan['w_off'][1])
  out = dict(plan, din0=32, Wp=torch.cat([wp0, plan['Wp'][old1:]]).contiguous(), Wf=None,
             w_off=[0] + [int(x) - old1 + wp0.numel() for x in plan['w_off'][1:]],
             embedding=net.embedding.weight.detach().float().contiguous())
  out.pop('_ext_consts', None)
  return out


def device_run(name, o=None, fold=True, packed_fold=True, G=None, act=False, fast=False):
  """The case's launch through ops.lanczosnet_forward -> dict(score [B,P], state [B,32,dhid], act
  [layers,B,32,dhid] | None, kernel, rare_strips, strip_plan | None ([(molecules, subtiles)], strips in use,
  entries), tile_plan | None (words, workgroups in use))."""
  from lanczosnet_amd import ops
  c = CASES[name]
  o = forward_operands(name) if o is None else o
  net = device_model(name)
  plan = net._plan()
  if c['dhid'] == 128 and c['din'] == 32:
    plan = narrow_plan(net, plan)
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
  mk, V, feat = t(o['mask']), t(o['V']), t(o['feat'])
  Lp = ops.pack_laplacian_for(plan, t(o['L']))
  Gd = t(o['G'] if G is None else G) if c['S'] > 0 else None
  tiling = c.get('tiling')
  out = dict(strip_plan=None, tile_plan=None)
  if tiling is None:
    tiles = ops.plan_tiles(mk, True, n_cu=c['n_cu'])
    words = tiles[0].strips.cpu().numpy()
    scap = (words.size - 1) // 80
    out['strip_plan'] = (plan_from_device(words, words[80 * scap]), int(words[80 * scap]), scap)
  elif tiling == 'none':
    tiles = 'none'
  else:
    buf, cap = ops.plan_tiles(mk, tiling == 'auto', n_cu=1)
    tiles = (buf.clone(), cap)                     # (a copy: without the strip plan that rides on the buffer)
    words = buf.cpu().numpy()
    out['tile_plan'] = (words, int(words[12 * cap]))
  B = mk.shape[0]
  cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
  acts = torch.zeros((c['layers'], B, 32, c['dhid']), dtype=torch.float32, device='cuda') if act else None
  with torch.no_grad():
    score, state = ops.lanczosnet_forward(plan, feat, Lp, V, Gd, mk, tiling=tiles, return_state=True, act_out=acts,
                                          fold=fold, packed_fold=packed_fold, rare_strips=cnt)
    out['kernel'] = ops.last_kernel()
    if fast:    # the scores-only launch (torch.ops.lanczosnet.forward: the path the benchmark times)
      out['fast'] = ops.lanczosnet_forward(plan, feat, Lp, V, Gd, mk, tiling=tiles, packed_fold=packed_fold).cpu()
      out['fast_kernel'] = ops.last_kernel()
  torch.cuda.synchronize()
  out.update(score=score.cpu(), state=state.cpu(), act=None if acts is None else acts.cpu(),
             rare_strips=int(cnt.item()))
  return out


def device_tensors(o, out):
  """the launch's results in the form of forward_eval's"""
  mask = torch.from_numpy(o['mask']).bool()
  N = mask.shape[1]
  got = dict(score=out['score'].double(), state=out['state'][:, :N][mask].double())
  if out['act'] is not None:
    for l in range(out['act'].shape[0]):
      got['act/%d' % l] = out['act'][l][:, :N][mask].double()
  return got


def hold_to_bars(name, got, truth=None, rows=None, what=''):
  """Print error, yardstick and bar of every tensor of `got`, then assert that each is within its bar.
  rows: {tensor: index} — compare these rows of the truth only (the scale stays the whole tensor's)."""
  truth_, e, _ = forward_reference(name)
  truth = truth_ if truth is None else truth
  k = forward_k(name)
  bad = []
  for t in sorted(got):
    ref = truth[t] if rows is None else truth[t][rows[t]]
    err = float((got[t] - ref).abs().max()) / float(truth[t].abs().max())
    b = bar(e[t], k)
    print('%s%s %-7s err %.2e  %s %.2e  bar %.2e  err / bar %.2f'
          % (name, what, t, err, 'e_split' if CASES[name]['gemm'] == 'f16x3' else 'e32', e[t], b, err / b))
    if not (err <= b and bool(torch.isfinite(got[t]).all())):
      bad.append((t, err, b))
  assert not bad, (name, what, bad)
