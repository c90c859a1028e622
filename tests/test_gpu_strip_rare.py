"""The folded form of the rare bond-type channels in the strip forward (csrc/conv_strip.hip,
strip_forward RARE): L_e = I + D_e for e >= 2, one GEMM1 on the summed weights and X W_e^T on the rows
channel e touches only.  Every case is ONE strip built by hand (a one-unit plan puts the whole batch into
one strip, molecules by falling size) so that a seam of the form occurs; the touched rows the test expects
are derived from the plan the device made and the numpy restatement of the touch rule
(utils/flop_model.py), and the lists, counts and virtual subtiles the strip built on the device
(lnz_forward_args.rare_debug) are held bit-equal to them.  Scores and final node states of the folded form and of the channel loop
(fold=False: the kernel as it was, the in-build reference) are held to the float64 oracle at the
project's 1e-5 relative bar at full depth (7 layers, 64 -> 128).

Deviation between the two forms (re-association of fp32 sums), largest over the cases below on an
MI355X: see DESIGN.md section 7."""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RARE = 'lanczosnet_strip_kernel<0,0,1,false,false>'
PLAIN = 'lanczosnet_strip_kernel<0,0,false,false>'


def _chain(n):
  return [(i, i + 1, 0) for i in range(n - 1)]


def _pairs(lo, hi, typ):
  """bonds (lo, lo+1), (lo+2, lo+3), ... below hi: every atom of [lo, hi) touched once"""
  return [(i, i + 1, typ) for i in range(lo, hi - 1, 2)]


# name -> (molecules [(atoms, extra bonds (i, j, bond type))], what the strip must look like)
CASES = {
    # no rare bond at all | a rare channel on every atom | one touched pair (the smallest D_e)
    'none_all_one': ([(12, []), (16, _pairs(0, 16, 1)), (8, [(2, 5, 3)])], dict(sub=3, counts={2: 16, 4: 2})),
    # exactly 16 touched rows of channel 2: one full virtual subtile
    'seam16': ([(8, _pairs(0, 8, 1)), (8, _pairs(0, 8, 1)), (10, [])], dict(sub=2, counts={2: 16}, nv=1)),
    # 17: the second virtual subtile holds one slot; the 8-atom molecule lies on rows 12 .. 19 (two
    # node subtiles) and its slots 9 .. 16 lie in both virtual subtiles
    'seam17_straddle': ([(12, [(0, 1, 1), (1, 2, 1)] + _pairs(3, 9, 1)), (8, _pairs(0, 8, 1))],
                        dict(sub=2, counts={2: 17}, nv=2)),
    # a 26-atom molecule next to small ones: five subtiles, padding rows between the molecules
    'five_subtiles': ([(26, _pairs(0, 10, 2) + [(20, 25, 5), (3, 17, 4)]), (7, [(0, 6, 3)]), (7, _pairs(0, 6, 1)),
                       (6, []), (5, [(0, 4, 5)]), (7, [(1, 3, 2), (3, 5, 2)]), (3, [])],
                      dict(sub=5)),
    # six subtiles: the channel loop
    'six_subtiles': ([(26, _pairs(0, 10, 2)), (26, [(3, 17, 4)]), (8, _pairs(0, 8, 1)), (8, []), (8, [(0, 7, 5)]),
                      (7, [(0, 6, 3)])], dict(sub=6, plain=True)),
}


def _batch(mols, seed, masked=()):
  """masked: (molecule, node) pairs the mask leaves out although the adjacency (and so every operator)
  keeps them."""
  rs = np.random.RandomState(seed)
  B, N = len(mols), max(n for n, _ in mols)
  adjs = np.zeros((B, N, N, 6), np.float32)
  nf = np.zeros((B, N), np.int64)
  mask = np.zeros((B, N), np.uint8)
  for b, (n, extra) in enumerate(mols):
    for i, j, typ in _chain(n) + list(extra):
      adjs[b, i, j, typ] = adjs[b, j, i, typ] = 1.0
    nf[b, :n] = rs.randint(0, 70, size=n)
    mask[b, :n] = 1
  for b, i in masked:
    mask[b, i] = 0
  return dict(adjs=adjs, node_feat=nf, node_mask=mask, n_nodes=np.array([n for n, _ in mols], np.int32))


_NET = {}


def _net():
  if not _NET:
    from lanczosnet_amd.model import LanczosNet
    from lanczosnet_amd.utils.arg_helper import make_model_config
    cfg = dict(oracle.DEFAULT_QM8_CFG)
    P = oracle.make_lanczosnet_params(cfg, 3)
    net = LanczosNet(make_model_config(cfg)).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    _NET.update(cfg=cfg, P=P, net=net.to(DEV))
  return _NET['cfg'], _NET['P'], _NET['net']


def _run(b, L=None):
  """-> dict: the folded form (twice), the channel loop, the oracle, the strip's touched-row counts."""
  from lanczosnet_amd import ops
  from lanczosnet_amd.utils import flop_model as fm
  cfg, P, net = _net()
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
  n = t(b['n_nodes'])
  if L is None:
    L = ops.laplacian_l4(t(b['adjs']), n)
  # (Ritz pairs on the extent the mask gives, last real node + 1: the kernels' slot count)
  ext = (b['node_mask'] * np.arange(1, b['node_mask'].shape[1] + 1)).max(axis=1).astype(np.int32)
  D, V = ops.lanczos_ritz(L[..., 0].contiguous(), t(ext), 20)
  plan = net._plan()
  Lp = ops.pack_laplacian_for(plan, L)
  G = ops.spectral_gains(D, cfg['long_diffusion_dist'], cfg['num_layer'], plan['mlp_pack'])
  nf, mk = t(b['node_feat']), t(b['node_mask'])
  tiles = ops.plan_tiles(mk, True, n_cu=1)
  out = {}
  with torch.no_grad():
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    scap = (tiles[0].strips.numel() - 1) // 80
    dbg = torch.zeros((scap, ops.RARE_DEBUG_INTS), dtype=torch.int32, device=DEV)
    out['rare'] = ops.lanczosnet_forward(plan, nf, Lp, V, G, mk, tiling=tiles, return_state=True, rare_strips=cnt,
                                         rare_debug=dbg)
    out['kernel'] = ops.last_kernel()
    out['again'] = ops.lanczosnet_forward(plan, nf, Lp, V, G, mk, tiling=tiles, return_state=True)
    out['fast'] = ops.lanczosnet_forward(plan, nf, Lp, V, G, mk, tiling=tiles)
    out['noident'] = ops.lanczosnet_forward(plan, nf, Lp, V, G, mk, tiling=tiles, use_ident=False)
    out['plain'] = ops.lanczosnet_forward(plan, nf, Lp, V, G, mk, tiling=tiles, return_state=True, fold=False)
    out['plain_kernel'] = ops.last_kernel()
  out['rare_strips'] = int(cnt.item())
  Lh = L.cpu().numpy()
  out['ref'] = oracle.lanczos_net_forward(P, cfg, b['node_feat'], Lh, D.cpu().numpy(), V.cpu().numpy(),
                                          b['node_mask'], dtype=np.float64, return_state=True)
  out['touch'] = fm.touch_masks(Lh, b['node_mask'])
  out['ident'] = Lp.ident.cpu().numpy()
  strips = tiles[0].strips.cpu().numpy()
  out['strips'] = fm.strips_from_plan(strips, out['ident'])
  out['counts'] = fm.strip_touch_counts(strips, out['touch'], 7)
  out['real'] = b['node_mask'].astype(bool)
  out['debug'] = dbg.cpu().numpy()
  out['plan'] = strips
  return out


def _check_device_lists(o, n_virtual=None):
  """What the strip found on the device (lnz_forward_args.rare_debug) against the numpy restatement:
  per folded channel the touched strip rows, ascending, bit for bit; their counts; the virtual
  subtiles (16 slots each, channel by channel) and the decision."""
  from lanczosnet_amd.utils import flop_model as fm
  e, d = o['plan'][:80], o['debug'][0]
  sub = int(e[1])
  want = [[] for _ in range(5)]
  for i in range(int(e[0])):
    bmol, st, n = (int(x) for x in e[2 + 3 * i:5 + 3 * i])
    rows = 4 if n <= 4 else (n + 3) // 4 * 4
    for f in range(5):
      want[f] += [st + r for r in range(rows) if (int(o['touch'][bmol][2 + f]) >> r) & 1]
  if sub > 5:
    assert not d.any()           # a six-subtile strip builds no lists
    return
  chans = []
  for f in range(5):
    assert int(d[2 + f]) == len(want[f]) == o['counts'][0][f], (f, d[2:7], want[f])
    assert d[16 + 96 * f:16 + 96 * f + len(want[f])].tolist() == sorted(want[f]), f
    assert not d[16 + 96 * f + len(want[f]):16 + 96 * (f + 1)].any()
    chans += [2 + f] * ((len(want[f]) + 15) // 16)
  assert int(d[1]) == len(chans) and d[8:8 + min(8, len(chans))].tolist() == chans[:8]
  assert int(d[0]) == int(fm.strip_takes_rare(sub, o['counts'][0], 5)) == o['rare_strips']
  if n_virtual is not None:
    assert int(d[1]) == n_virtual


def _check_against_oracle(o):
  ref_s, ref_x = o['ref']
  real = o['real']
  N = real.shape[1]
  dev = {}
  for form in ('rare', 'plain'):
    s, x = (v.cpu().numpy().astype(np.float64) for v in o[form])
    es = np.abs(s - ref_s).max() / np.abs(ref_s).max()
    ex = np.abs(x[:, :N][real] - ref_x[real]).max() / np.abs(ref_x[real]).max()
    print('%s: score rel err %.2e, state rel err %.2e' % (form, es, ex))
    assert es <= 1e-5 and ex <= 1e-5, (form, es, ex)
    dev[form] = (s, x[:, :N][real])
  d = max(np.abs(dev['rare'][0] - dev['plain'][0]).max() / np.abs(ref_s).max(),
          np.abs(dev['rare'][1] - dev['plain'][1]).max() / np.abs(ref_x[real]).max())
  print('folded form vs channel loop: %.2e' % d)
  # two launches of the folded form: the same bits (scores; states of every row the launch writes)
  assert torch.equal(o['rare'][0], o['again'][0]) and torch.equal(o['rare'][1], o['again'][1])
  assert torch.equal(o['rare'][0], o['fast'])
  # ... and the same bits without the pack's identity-channel bits (the touched rows come from the pack)
  assert torch.equal(o['rare'][0], o['noident'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_folded_form_on_hand_built_strips(name):
  from lanczosnet_amd.utils import flop_model as fm
  mols, want = CASES[name]
  o = _run(_batch(mols, seed=len(name)))
  assert len(o['strips']) == 1 and o['strips'][0]['sub'] == want['sub'], o['strips']
  counts = o['counts'][0]
  for e, c in want.get('counts', {}).items():
    assert counts[e - 2] == c, (e, counts)
  takes = fm.strip_takes_rare(want['sub'], counts, 5)
  assert takes == (not want.get('plain', False))
  # the launcher names the kernel with the folded form (it is the strip that decides); the counter
  # tells which form the strip took
  assert o['kernel'] == RARE and o['plain_kernel'] == PLAIN, (o['kernel'], o['plain_kernel'])
  assert o['rare_strips'] == (1 if takes else 0)
  _check_device_lists(o, want.get('nv'))
  # ident bit c <=> no touched row in channel c (the masks are the ones the device's lists equal)
  for bmol in range(len(mols)):
    for c in range(7):
      assert bool((int(o['ident'][bmol]) >> c) & 1) == (int(o['touch'][bmol][c]) == 0), (bmol, c)
  _check_against_oracle(o)


def test_operator_without_identity_rows_takes_the_channel_loop():
  """Every bond-type channel replaced by a dense operator (the simple graph's, scaled): every row is
  touched in every folded channel, the folded form would issue more — the strip keeps the channel loop."""
  from lanczosnet_amd import ops
  from lanczosnet_amd.utils import flop_model as fm
  b = _batch([(12, []), (9, []), (8, []), (16, [])], seed=5)
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
  L = ops.laplacian_l4(t(b['adjs']), t(b['n_nodes']))
  for e in range(2, 7):
    L[..., e] = L[..., 0] * (0.5 + 0.1 * e)
  o = _run(b, L=L)
  assert not fm.strip_takes_rare(o['strips'][0]['sub'], o['counts'][0], 5)
  assert o['kernel'] == RARE and o['rare_strips'] == 0
  _check_device_lists(o)
  _check_against_oracle(o)


def test_non_symmetric_channel_touches_row_and_column():
  """One element L_e[i][j] without its mirror: row i AND column j are touched (the row | column rule)."""
  from lanczosnet_amd import ops
  b = _batch([(12, [(0, 5, 2)]), (9, []), (8, [(1, 2, 4)])], seed=6)
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
  L = ops.laplacian_l4(t(b['adjs']), t(b['n_nodes']))
  L[1, 2, 7, 4] = 0.375          # molecule 1 had no bond of that type: rows 2 and 7 become touched
  L[0, 9, 3, 5] = -0.25
  o = _run(b, L=L)
  assert int(o['touch'][1][4]) == (1 << 2) | (1 << 7) and int(o['touch'][0][5]) == (1 << 9) | (1 << 3)
  assert o['rare_strips'] == 1
  _check_device_lists(o)
  _check_against_oracle(o)


def test_nodes_the_mask_leaves_out_but_the_operator_keeps():
  """A hole in the mask and a trailing masked node: L4 (built from n_nodes) keeps both as nodes, unit
  diagonal in every bond-type channel without their bond; only the read-out skips them.  They go on
  feeding their neighbours through channels 0 and 1, so their own state must be right: such a row is
  touched (its diagonal is not the 0 the folded GEMM1 supplies on a masked row) and gets Z_e through
  the scatter.  Both forms against the float64 oracle."""
  mols = [(12, [(0, 5, 2), (7, 8, 1)]), (10, [(2, 3, 3)]), (8, _pairs(0, 8, 1)), (9, [])]
  masked = [(0, 4), (0, 7), (1, 9), (3, 2)]      # holes (one on a rare bond), a trailing node, a hole
  o = _run(_batch(mols, seed=9, masked=masked))
  assert len(o['strips']) == 1
  # the hole (0, 4) has no rare bond: touched by its diagonal in all five folded channels
  for c in range(2, 7):
    assert (int(o['touch'][0][c]) >> 4) & 1 and (int(o['touch'][1][c]) >> 9) & 1 and (int(o['touch'][3][c]) >> 2) & 1
  assert o['rare_strips'] == 1
  _check_device_lists(o)
  _check_against_oracle(o)


def test_default_forward_of_a_drawn_batch_takes_the_folded_form():
  """48 drawn molecules through the module's own forward (the path bench.py times)."""
  from lanczosnet_amd import ops
  from lanczosnet_amd.synthetic import draw_batch
  cfg, P, net = _net()
  b = draw_batch(48, seed=2)
  t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
  n = t(b['n_nodes'])
  L = ops.laplacian_l4(t(b['adjs']), n)
  D, V = ops.lanczos_ritz(L[..., 0], n, 20)
  with torch.no_grad():
    score, _ = net(t(b['node_feat']), L, D, V, label=t(b['label']), mask=t(b['node_mask']))
  assert ops.last_kernel() == RARE
  ref = oracle.lanczos_net_forward(P, cfg, b['node_feat'], L.cpu().numpy(), D.cpu().numpy(), V.cpu().numpy(),
                                   b['node_mask'], dtype=np.float64)
  err = np.abs(score.cpu().numpy() - ref).max() / np.abs(ref).max()
  print('score rel err %.2e' % err)
  assert err <= 1e-5
