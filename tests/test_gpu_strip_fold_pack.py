"""The packed folded weights of the strip forward (csrc/conv_strip.hip, strip_forward RARE = 2;
lnz_pack_fold_weights, lnz_forward_args.Wf): W_F = sum_{e >= 2} W_e is packed once per weight set and read
through the weight ring, which jumps from edge type 1 to the block and from there to the first virtual
subtile's channel (or nowhere, when the strip has none).  The launch that withholds the block
(packed_fold=False) runs the instantiation that sums W_F in registers — the in-build reference.  Both evaluate, per accumulator, the same MFMAs on the same bits in
the same order, so everything here is held BIT-equal; one case is also held to the float64 oracle at the
project's 1e-5 bar.  Every case is one strip built by hand (a one-unit plan), as in
test_gpu_strip_rare.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from test_gpu_strip_rare import CASES as RARE_CASES, _chain, _pairs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RARE = 'lanczosnet_strip_kernel<0,0,1,false,false>'

# name -> (bond types of the model, molecules [(atoms, extra bonds (i, j, bond type))], what the strip
# must look like: subtiles, channel of every virtual subtile (bond type t is channel t + 1))
CASES = {
    'seam16': (6, RARE_CASES['seam16'][0], dict(sub=2, chans=[2])),
    # two virtual subtiles of one channel, the second holds one slot
    'seam17_straddle': (6, RARE_CASES['seam17_straddle'][0], dict(sub=2, chans=[2, 2])),
    'five_subtiles': (6, RARE_CASES['five_subtiles'][0], dict(sub=5)),
    # 40 touched rows of channel 2: three virtual subtiles of one channel
    'three_of_one_channel': (6, [(16, _pairs(0, 16, 1)), (16, _pairs(0, 16, 1)), (8, _pairs(0, 8, 1))],
                             dict(sub=3, chans=[2, 2, 2])),
    # RARE_MAXV virtual subtiles: three of channel 2 (36 rows), two of channel 3 (20 rows), channels 4, 5,
    # 6 one each
    'eight_subtiles': (6, [(16, _pairs(0, 16, 1) + _pairs(0, 16, 2) + [(0, 1, 3)]),
                           (16, _pairs(0, 16, 1) + _pairs(0, 4, 2) + _pairs(4, 8, 4) + [(10, 11, 5)]),
                           (12, _pairs(0, 4, 1))],
                       dict(sub=3, chans=[2, 2, 2, 3, 3, 4, 5, 6])),
    # no touched row at all: the folded GEMM1 only, the ring goes straight on to the next layer
    'no_touched_row': (6, [(12, []), (10, []), (8, [])], dict(sub=2, chans=[])),
    'one_subtile': (6, [(8, [(2, 5, 3)]), (6, [])], dict(sub=1, chans=[4])),
    # six subtiles: both forms run the channel loop
    'six_subtiles': (6, RARE_CASES['six_subtiles'][0], dict(sub=6, plain=True)),
    # fewer bond types: n_edge = 3 (ONE folded channel, W_F = 0 + W_2: by the cost rule such a strip folds
    # only when the channel touches no row: 32 S + nv (32 + 4 S) < 32 S + 4 (3 S - 2) needs nv = 0) and
    # n_edge = 5 (three folded channels: two virtual subtiles of channel 2, one of 3, one of 4)
    'n_edge3': (2, [(12, []), (9, []), (8, [])], dict(sub=2, chans=[])),
    'n_edge5': (4, [(16, _pairs(0, 16, 1) + [(3, 9, 3)]), (10, _pairs(0, 4, 1) + [(1, 7, 2)]), (7, [(0, 6, 3)])],
                dict(sub=3, chans=[2, 2, 3, 4])),
}


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _batch(mols, seed, n_type):
  rs = np.random.RandomState(seed)
  B, N = len(mols), max(n for n, _ in mols)
  adjs = np.zeros((B, N, N, n_type), np.float32)
  nf = np.zeros((B, N), np.int64)
  mask = np.zeros((B, N), np.uint8)
  for b, (n, extra) in enumerate(mols):
    for i, j, typ in _chain(n) + list(extra):
      adjs[b, i, j, typ] = adjs[b, j, i, typ] = 1.0
    nf[b, :n] = rs.randint(0, 70, size=n)
    mask[b, :n] = 1
  return dict(adjs=adjs, node_feat=nf, node_mask=mask, n_nodes=np.array([n for n, _ in mols], np.int32))


_NETS = {}


def _net(n_type):
  if n_type not in _NETS:
    from lanczosnet_amd.model import LanczosNet
    from lanczosnet_amd.utils.arg_helper import make_model_config
    cfg = dict(oracle.DEFAULT_QM8_CFG, num_bond_type=n_type)
    P = oracle.make_lanczosnet_params(cfg, 3)
    net = LanczosNet(make_model_config(cfg)).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    _NETS[n_type] = (cfg, P, net.to(DEV))
  return _NETS[n_type]


def _operands(net, cfg, b):
  from lanczosnet_amd import ops
  n = _t(b['n_nodes'])
  L = ops.laplacian_l4(_t(b['adjs']), n)
  D, V = ops.lanczos_ritz(L[..., 0].contiguous(), n, 20)
  plan = net._plan()
  Lp = ops.pack_laplacian_for(plan, L)
  G = ops.spectral_gains(D, cfg['long_diffusion_dist'], cfg['num_layer'], plan['mlp_pack'])
  nf, mk = _t(b['node_feat']), _t(b['node_mask'])
  tiles = ops.plan_tiles(mk, True, n_cu=1)
  return dict(L=L, D=D, V=V, Lp=Lp, G=G, nf=nf, mk=mk, tiles=tiles)


def _launches(net, o):
  """-> {(packed, use_ident): (score, state, fast-path score, rare_debug, rare_strips, kernel)}"""
  from lanczosnet_amd import ops
  plan = net._plan()
  scap = (o['tiles'][0].strips.numel() - 1) // 80
  out = {}
  with torch.no_grad():
    for packed in (True, False):
      for ident in (True, False):
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        dbg = torch.zeros((scap, ops.RARE_DEBUG_INTS), dtype=torch.int32, device=DEV)
        kw = dict(tiling=o['tiles'], use_ident=ident, packed_fold=packed)
        s, x = ops.lanczosnet_forward(plan, o['nf'], o['Lp'], o['V'], o['G'], o['mk'], return_state=True,
                                      rare_strips=cnt, rare_debug=dbg, **kw)
        kernel = ops.last_kernel()
        fast = ops.lanczosnet_forward(plan, o['nf'], o['Lp'], o['V'], o['G'], o['mk'], **kw)
        out[packed, ident] = (s, x, fast, dbg.cpu().numpy(), int(cnt.item()), kernel)
  return out


def _hold_bit_equal(r, folds):
  for key, (s, x, fast, dbg, cnt, kernel) in r.items():
    ref = r[False, key[1]]   # the withheld form with the same use_ident
    assert torch.equal(s, ref[0]) and torch.equal(x, ref[1]), key
    assert torch.equal(s, r[False, True][0]), key  # scores: the same with and without the identity bits
    assert torch.equal(fast, ref[0]), key          # the fast path (scores only)
    assert kernel == RARE, (key, kernel)           # the launcher notes one name for both forms
    assert cnt == ref[4] == (1 if folds else 0), (key, cnt)
    d = dbg.copy()
    assert int(d[0, 7]) == (1 if key[0] and folds else 0), (key, d[0, :8])
    d[0, 7] = 0
    assert np.array_equal(d, ref[3]), key


@pytest.mark.parametrize('name', sorted(CASES))
def test_packed_and_withheld_forms_give_the_same_bits(name):
  n_type, mols, want = CASES[name]
  cfg, P, net = _net(n_type)
  plan = net._plan()
  assert plan['n_edge'] == n_type + 1 and plan['Wf'] is not None
  o = _operands(net, cfg, _batch(mols, seed=len(name), n_type=n_type))
  strips = o['tiles'][0].strips.cpu().numpy()
  assert int(strips[-1]) == 1 and int(strips[1]) == want['sub'], strips[:2]
  r = _launches(net, o)
  folds = not want.get('plain', False)
  _hold_bit_equal(r, folds)
  d = r[True, True][3][0]
  assert int(d[0]) == (1 if folds else 0)
  if 'chans' in want:    # the virtual subtiles, channel by channel
    assert int(d[1]) == len(want['chans']) and d[8:8 + len(want['chans'])].tolist() == want['chans'], d[:16]


def _fold_numpy(plan):
  """lnz_pack_fold_weights restated on the host from the conv pack: float32, + 0.0 first, e ascending."""
  Wp = plan['Wp'].cpu().numpy()
  C_ = plan['n_long'] + plan['n_edge']
  parts = []
  for l in range(plan['num_layer']):
    din = plan['din0'] if l == 0 else plan['dhid']
    RT, Q = plan['dhid'] // 32, din // 8
    blk = Wp[plan['w_off'][l]:plan['w_off'][l] + RT * C_ * Q * 256].reshape(RT, C_, Q * 256)
    s = np.zeros((RT, Q * 256), np.float32)
    for e in range(2, plan['n_edge']):
      s = s + blk[:, plan['n_long'] + e]
    assert s.dtype == np.float32
    parts.append(s.reshape(-1))
  return np.concatenate(parts + [np.zeros(2048, np.float32)])


@pytest.mark.parametrize('n_type', [2, 4, 6])
def test_pack_kernel_against_the_numpy_restatement(n_type):
  """QM8 config: layer 0 is 64 wide (four ring steps), the others 128 (eight); n_edge 3 (one folded
  channel), 5 and 7.  Bit for bit, slack zero."""
  from lanczosnet_amd import _lib
  cfg, P, net = _net(n_type)
  plan = net._plan()
  got = plan['Wf'].cpu().numpy()
  want = _fold_numpy(plan)
  assert got.size == want.size == _lib.load().lnz_pack_fold_weights_size(plan['num_layer'], plan['din0'], plan['dhid'])
  assert got.size == 128 * 64 + 6 * 128 * 128 + 2048
  assert np.array_equal(got.view(np.int32), want.view(np.int32))
  assert not got[-2048:].any() and got[:-2048].any()


def test_packed_form_against_the_float64_oracle():
  n_type, mols, want = CASES['eight_subtiles']
  cfg, P, net = _net(n_type)
  b = _batch(mols, seed=11, n_type=n_type)
  o = _operands(net, cfg, b)
  r = _launches(net, o)
  ref_s, ref_x = oracle.lanczos_net_forward(P, cfg, b['node_feat'], o['L'].cpu().numpy(), o['D'].cpu().numpy(),
                                            o['V'].cpu().numpy(), b['node_mask'], dtype=np.float64,
                                            return_state=True)
  real = b['node_mask'].astype(bool)
  N = real.shape[1]
  s, x = (v.cpu().numpy().astype(np.float64) for v in r[True, True][:2])
  es = np.abs(s - ref_s).max() / np.abs(ref_s).max()
  ex = np.abs(x[:, :N][real] - ref_x[real]).max() / np.abs(ref_x[real]).max()
  print('packed form: score rel err %.2e, state rel err %.2e' % (es, ex))
  assert int(r[True, True][3][0, 7]) == 1 and int(r[True, True][3][0, 1]) == 8
  assert es <= 1e-5 and ex <= 1e-5, (es, ex)


def test_raw_abi_launch_with_the_block_equals_the_extension_launch():
  """lnz_forward_args filled by hand with Wf set, against ops.lanczosnet_forward."""
  from lanczosnet_amd import _lib
  lib = _lib.load()
  n_type, mols, want = CASES['three_of_one_channel']
  cfg, P, net = _net(n_type)
  b = _batch(mols, seed=7, n_type=n_type)
  o = _operands(net, cfg, b)
  r = _launches(net, o)
  plan = net._plan()
  B, N, K = o['V'].shape
  fa = _lib.ForwardArgs()
  fa.B, fa.N, fa.K, fa.num_layer = B, N, K, plan['num_layer']
  fa.din0, fa.dhid, fa.dout = plan['din0'], plan['dhid'], plan['dout']
  fa.n_short, fa.n_long, fa.n_edge = 0, plan['n_long'], plan['n_edge']
  fa.node_feat, fa.embedding, fa.num_atom = o['nf'].data_ptr(), plan['embedding'].data_ptr(), plan['embedding'].shape[0]
  V = o['V'].contiguous()
  fa.mask, fa.Lp, fa.V, fa.G = o['mk'].data_ptr(), o['Lp'].data_ptr(), V.data_ptr(), o['G'].data_ptr()
  fa.ident = o['Lp'].ident.data_ptr()
  fa.Wp, fa.bias, fa.Wf = plan['Wp'].data_ptr(), plan['bias'].data_ptr(), plan['Wf'].data_ptr()
  for i in range(plan['num_layer']):
    fa.w_off[i], fa.b_off[i] = plan['w_off'][i], plan['b_off'][i]
  fa.Wp_head, fa.bias_head = plan['Wp_head'].data_ptr(), plan['bias_head'].data_ptr()
  tiles, cap = o['tiles']
  fa.plan, fa.n_wg, fa.plan_wg_cap = tiles.data_ptr(), tiles.data_ptr() + 48 * cap, cap
  strips = tiles.strips
  scap = (strips.numel() - 1) // 80
  fa.strips, fa.n_strips, fa.strip_cap = strips.data_ptr(), strips.data_ptr() + 4 * 80 * scap, scap
  score = torch.empty((B, plan['dout']), device=DEV)
  state = torch.zeros((B, 32, plan['dhid']), device=DEV)
  dbg = torch.zeros((scap, 512), dtype=torch.int32, device=DEV)
  fa.score, fa.state_out, fa.rare_debug = score.data_ptr(), state.data_ptr(), dbg.data_ptr()
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  _lib.check(lib.lnz_lanczosnet_forward(C.byref(fa), st))
  torch.cuda.synchronize()
  assert int(dbg[0, 7]) == 1
  assert torch.equal(score, r[True, True][0]) and torch.equal(state, r[True, True][1])
  assert np.array_equal(dbg.cpu().numpy(), r[True, True][3])


def test_the_block_follows_the_weights():
  """A weight change that bumps no tensor version plus invalidate_plan(): the plan is rebuilt with a new
  block, and the packed and withheld forms are bit-equal again (on other scores than before)."""
  from lanczosnet_amd.model import LanczosNet
  from lanczosnet_amd.utils.arg_helper import make_model_config
  n_type, mols, want = CASES['seam17_straddle']
  cfg, P, _ = _net(n_type)
  net = LanczosNet(make_model_config(cfg)).eval()       # (its own module: the shared one keeps its weights)
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV)
  o = _operands(net, cfg, _batch(mols, seed=4, n_type=n_type))
  before = _launches(net, o)
  wf_before = net._plan()['Wf'].clone()
  rs = np.random.RandomState(12)
  with torch.no_grad():
    for t in range(cfg['num_layer']):
      w = net.filter[t].weight
      w.data.add_(_t((0.05 * rs.standard_normal(tuple(w.shape))).astype(np.float32)))
  net.invalidate_plan()
  plan = net._plan()
  assert not torch.equal(plan['Wf'], wf_before)
  assert np.array_equal(plan['Wf'].cpu().numpy().view(np.int32), _fold_numpy(plan).view(np.int32))
  after = _launches(net, o)
  _hold_bit_equal(after, True)
  assert not torch.equal(after[True, True][0], before[True, True][0])
