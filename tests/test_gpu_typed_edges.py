"""GPU checks of several edge types on the large-graph sparse path (csrc/edge_image.hip:
lnz_laplacian_l4_typed_edges_images; csrc/conv_sparse.hip: lnz_large_sparse_image_channels,
lnz_large_sparse_conv_channels[_f32]; ops.lanczos_ritz_edges / sparse_laplacian_from_edges with
edge_type, dataset.collate_graph_edges with num_edge_type, the module on a typed SparseLaplacian)
against the DENSE route on the same typed graphs: typed adjs [B,N,N,E] -> ops.laplacian_l4 ->
L [B,N,N,E+1] -> the existing one-operator entries on its slices.  Graphs: tests/typed_edge_graphs.py
(tests/test_typed_edges_cpu.py shows that they stay inside both row capacities)."""
import contextlib
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import edge_graphs as eg  # noqa: E402
import oracle  # noqa: E402
import typed_edge_graphs as tg  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'typed_edges.npz')


@contextlib.contextmanager
def _no_densify():
  with warnings.catch_warnings():
    warnings.filterwarnings('error', message='.*densified.*')
    yield


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _packed(graphs):
  """-> edges, edge_off, n_nodes, edge_type on the device."""
  return tuple(_t(a) for a in tg.pack(graphs))


def _typed(graphs, E):
  e, off, n, ty = _packed(graphs)
  return (e, off, n), dict(edge_type=ty, num_edge_type=E)


@functools.lru_cache(maxsize=None)
def _dense(name, E):
  """typed graphs, N and the dense route's L [B,N,N,E+1] (computed once, shared, left unchanged)."""
  from lanczosnet_amd import ops
  graphs, N = tg.layer_case(E) if name == 'layer' else tg.case(name, E)
  L = ops.laplacian_l4(_t(tg.dense_adjs(graphs, N, E)), _t(tg.pack(graphs)[2]))
  return graphs, N, L


def _three(E):
  """Three non-empty typed graphs padded to 301 nodes (the validation and module checks)."""
  graphs, N = eg.case('n301')
  rs = np.random.RandomState(31)
  n = 150
  graphs = graphs[:2] + [dict(n=n, edges=eg.with_special_rows(n, eg.gnp_edges(n, 0.03, rs), eg.conv_cap(N)))]
  return tg.add_types(graphs, E, 200 + E), N


def _used(counts, cap):
  """mask of each row's first ceil(count / 8) * 8 slots (the slots the gather reads)."""
  return torch.arange(cap, device=counts.device) < ((counts + 7) // 8 * 8)[..., None]


def _same_image(a, b):
  assert a.cap == b.cap and torch.equal(a.counts, b.counts)
  m = _used(a.counts, a.cap)
  assert torch.equal(a.entries[m], b.entries[m])
  assert torch.equal(a.values[m], b.values[m])


def _rel(a, b):
  return float((a - b).abs().max()) / float(b.abs().max())


# ---- 1. the images ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,E', [('n301', 2), ('n301', 3), ('n256', 2), ('n256', 3), ('n256', 7), ('n2100', 2)])
def test_typed_images_are_the_dense_compaction_of_every_channel(name, E):
  from lanczosnet_amd import ops
  graphs, N, L = _dense(name, E)
  args, kw = _typed(graphs, E)
  sl = ops.sparse_laplacian_from_edges(*args, N, **kw)
  assert sl.channels == E + 1 and tuple(sl.shape) == tuple(L.shape) and sl.images.R == E + 1
  assert int(sl.images.flags.item()) == 0 and sl.images.cap == ops.large_sparse_row_cap(N)
  once = ops.large_sparse_image_channels(L)
  assert int(once.flags.item()) == 0
  worst = 0.0
  for c in range(E + 1):
    ref = ops.large_sparse_image(L[..., c:c + 1], values=True)
    assert int(ref.flags.item()) == 0
    _same_image(sl.images.channel(c), ref)
    _same_image(once.channel(c), ref)
    counts, ent, val = (x.cpu().numpy() for x in (sl.images.counts[c], sl.images.entries[c], sl.images.values[c]))
    for b, g in enumerate(graphs):
      assert (counts[b, g['n']:] == 0).all()                                 # rows >= n_b are empty
      for i, (cols, v64) in enumerate(tg.channel_rows_fp64(g, c)):
        k = counts[b, i]
        assert k == cols.shape[0]
        assert (ent[b, i, :k] & 0xffff == cols).all()                        # ascending columns
        worst = max(worst, float(np.abs(val[b, i, :k].astype(np.float64) - v64).max()))
        pad = (k + 7) // 8 * 8
        assert (ent[b, i, k:pad] == 0).all() and (val[b, i, k:pad] == 0).all()
      if g['n'] and c < 3:   # the engineered rows: n - 4 (all type 0), n - 3 (all type 1), n - 2 (1 + 7), n - 1
        want = {0: [sl.images.cap, 8, 9, 1], 1: [sl.images.cap, 1, 2, 1], 2: [1, 8, 8, 1]}[c]
        assert list(counts[b, g['n'] - 4:g['n']]) == want
  assert torch.equal(sl.image.entries, sl.images.entries[0])
  print('%s E %d: values against the fp64 formula, max abs %.2e' % (name, E, worst))
  assert worst < 1e-7
  assert torch.equal(sl.to_dense(), L)
  if E == 3:   # graph 1 has no edge of type 2: channel 3 is the identity on its live rows
    n1 = graphs[1]['n']
    assert (sl.images.counts[3, 1, :n1] == 1).all() and (sl.images.values[3, 1, :n1, 0] == 1.0).all()


# ---- 2. a pure function of the typed edge set -----------------------------------------------------------
def test_edge_order_endpoint_order_and_a_second_call_do_not_change_a_bit():
  from lanczosnet_amd import ops
  graphs, N, L = _dense('n301', 2)

  def run(gs):
    args, kw = _typed(gs, 2)
    return ops.lanczos_ritz_edges(*args, N, 20, return_info=True, **kw)
  with _no_densify():
    base, again, mixed = run(graphs), run(graphs), run(tg.shuffled(graphs, 41))
  for other in (again, mixed):
    assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1]) and torch.equal(base[3], other[3])
    for c in range(3):
      _same_image(base[2].images.channel(c), other[2].images.channel(c))


# ---- 3. Ritz pairs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,E,M,K,wide', [('n301', 3, 20, 20, False), ('n2100', 2, 8, 8, True)])
def test_typed_ritz_pairs_equal_the_dense_route_on_channel_0(name, E, M, K, wide):
  from lanczosnet_amd import ops
  graphs, N, L = _dense(name, E)
  args, kw = _typed(graphs, E)
  with _no_densify():
    D, V, sl, info = ops.lanczos_ritz_edges(*args, N, K, lanczos_steps=M, return_info=True, **kw)
    Dr, Vr, infor = ops.lanczos_ritz_kstep(L[..., 0], args[2], M, K, return_info=True)
  assert ('wide' in ops.last_kernel()) == wide
  print('%s E %d M %d K %d: max |D - D_dense| %.2e  max |V - V_dense| %.2e' %
        (name, E, M, K, float((D - Dr).abs().max()), float((V - Vr).abs().max())))
  assert torch.equal(info, infor) and torch.equal(D, Dr) and torch.equal(V, Vr)
  assert sl.channels == E + 1 and int(sl.images.flags.item()) == 0
  for c in range(E + 1):
    _same_image(sl.images.channel(c), ops.large_sparse_image(L[..., c:c + 1], values=True))


# ---- 4. validation on the device --------------------------------------------------------------------------
GUARD = 256


class _Guarded:
  """Device arrays with 256 sentinel bytes in front of and behind each."""

  def __init__(self):
    self.bufs = []

  def __call__(self, shape, dtype):
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    self.bufs.append((buf, nbytes))
    return buf[GUARD:GUARD + nbytes].view(dtype).view(shape)

  def intact(self):
    return all(bool((b[:GUARD] == 0xA5).all()) and bool((b[GUARD + n:] == 0xA5).all()) for b, n in self.bufs)


def _c_call(edges, off, n, ty, N, E):
  """lnz_laplacian_l4_typed_edges_images with every output and the workspace between sentinels."""
  from lanczosnet_amd import ops
  B, cap = n.shape[0], ops.large_sparse_row_cap(N)
  need = ops._abi().laplacian_l4_typed_edges_images_workspace_bytes(B, N, E, cap)
  g = _Guarded()
  o = dict(ws=g((need,), torch.uint8), entries=g((E + 1, B, N, cap), torch.int32),
           values=g((E + 1, B, N, cap), torch.float32), counts=g((E + 1, B, N), torch.int32),
           flags=g((1,), torch.int32), status=g((B,), torch.int32))
  ops._abi().laplacian_l4_typed_edges_images(edges, ty, edges.shape[0], off, n, B, N, E, o['ws'], need, o['entries'],
                                             o['values'], o['counts'], cap, o['flags'], o['status'])
  torch.cuda.synchronize()
  assert g.intact()
  return o


@functools.lru_cache(maxsize=None)
def _clean_three():
  graphs, N = _three(2)
  return _c_call(*_packed(graphs), N, 2)


@pytest.mark.parametrize('what,bit,reason', [('two types', 4, 'duplicate'), ('type E', 32, 'edge type'),
                                             ('negative', 32, 'edge type')])
def test_bad_typed_graph_is_flagged_alone_and_nothing_else_moves(what, bit, reason):
  from lanczosnet_amd import ops
  E, bad = 2, 1
  graphs, N = _three(E)
  graphs = [dict(g, edges=g['edges'].copy(), types=g['types'].copy()) for g in graphs]
  g = graphs[bad]
  if what == 'two types':                       # the same pair again, the other way round, with the other type
    g['edges'] = np.concatenate([g['edges'], g['edges'][:1, ::-1]], axis=0)
    g['types'] = np.concatenate([g['types'], 1 - g['types'][:1]])
  elif what == 'type E':
    g['types'][3] = E
  else:
    g['types'][3] = -1
  edges, off, n, ty = _packed(graphs)
  clean, got = _clean_three(), _c_call(edges, off, n, ty, N, E)
  assert got['status'].tolist() == [bit if b == bad else 0 for b in range(3)]
  assert int(clean['flags'].item()) == 0 and clean['status'].tolist() == [0, 0, 0]
  for key in ('counts', 'entries', 'values'):
    assert not got[key][:, bad].any(), key                                    # its rows are empty in every channel
  used = _used(clean['counts'], clean['entries'].shape[3])
  for b in (b for b in range(3) if b != bad):
    assert torch.equal(got['counts'][:, b], clean['counts'][:, b])
    for key in ('entries', 'values'):
      assert torch.equal(got[key][:, b][used[:, b]], clean[key][:, b][used[:, b]]), key
  with pytest.raises(ValueError, match='graph %d .*%s' % (bad, reason)):
    ops.lanczos_ritz_edges(edges, off, n, N, 20, edge_type=ty, num_edge_type=E)
  with pytest.raises(ValueError, match='graph %d .*%s' % (bad, reason)):
    ops.sparse_laplacian_from_edges(edges, off, n, N, edge_type=ty, num_edge_type=E)


# ---- 5. the gather over several operators, layer level -------------------------------------------------------
def _bf16(x):
  return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@pytest.mark.parametrize('name,K,din,S', [('layer', 20, 16, 2), ('n301', 40, 10, 3), ('n2100', 8, 128, 2)])
def test_channels_layer_matches_the_streamed_layer_and_fp64(name, K, din, S):
  """Three distinct operator channels (E = 2).  bf16: the same rounded operands as the streamed layer on all
  channels packed, another summation order (1e-5 of the largest output), and an fp64 sum over the launch's
  own Z (1e-5); fp32: a float64 einsum on the unrounded operands (1e-5 relative); two calls are equal."""
  from lanczosnet_amd import ops
  graphs, N, L = _dense(name, 2)
  B, R = len(graphs), 3
  rs = np.random.RandomState(N)
  V = (rs.randn(B, N, K) / np.sqrt(N)).astype(np.float32)
  G = rs.rand(B, S, K).astype(np.float32)
  X = rs.randn(B, N, din).astype(np.float32)
  W = (rs.randn(128, S + R, din) / np.sqrt(din * (S + R))).astype(np.float32)
  bias = (rs.randn(128) * 0.1).astype(np.float32)
  dinp = (din + 15) // 16 * 16
  Wc = np.pad(W, ((0, 0), (0, 0), (0, dinp - din)))
  Wn = _t(Wc[:, S:].transpose(1, 0, 2).reshape(R * 128, dinp))                # channel blocks, not summed
  Wf = ops.large_weight_fragments(ops.split_bf16_planes(Wn, 1))
  Wt = ops.pack_rows_k8(_t(Wc[:, :S].reshape(128, S * dinp)))
  Xd, Vd, Gd, bd = _t(X), _t(V), _t(G), _t(bias)
  args, kw = _typed(graphs, 2)
  imgs = ops.sparse_laplacian_from_edges(*args, N, **kw).images
  assert int(imgs.flags.item()) == 0 and imgs.R == R
  Lb, Vb = ops.large_pack_operators(L, Vd, 1)
  Vb1 = ops.large_pack_vectors(Vd, 1)
  for relu in (True, False):
    # (the projection's fp32 atomics: the sparse layer is handed the streamed layer's T, as in
    # test_sparse_layer_matches_the_streamed_layer_and_fp64)
    dwork = ops.large_work_buffers(Lb)
    dense = ops.large_conv_layer(Xd, din, Lb, Vb, Vd, Wf, Wt, Gd, bd, dwork, relu=relu)
    swork = ops.large_sparse_work_buffers(B, N, DEV, R=R)
    swork[1].copy_(dwork[1])
    sparse = ops.large_sparse_conv_layer(Xd, din, imgs, Vb1, Vd, Wf, None, None, bd, swork, relu=relu)
    assert ops.last_kernel() == 'sparse_conv_channels_kernel'
    err = _rel(sparse, dense)
    print('%s bf16 relu %d: against the streamed layer %.2e' % (name, relu, err))
    assert err <= 1e-5
  # without long scales, against the launch's own Z in fp64
  A = L.cpu().numpy()
  work0 = ops.large_sparse_work_buffers(B, N, DEV, R=R)
  sparse0 = ops.large_sparse_conv_layer(Xd, din, imgs, Vb1, Vd, Wf, None, None, bd, work0)
  again0 = ops.large_sparse_conv_layer(Xd, din, imgs, Vb1, Vd, Wf, None, None, bd,
                                       ops.large_sparse_work_buffers(B, N, DEV, R=R))
  assert torch.equal(sparse0, again0)
  Zdev = work0[0].float().cpu().numpy().astype(np.float64)
  ref0 = sum(np.einsum('bnm,bmo->bno', _bf16(A[..., c]).astype(np.float64), Zdev[c]) for c in range(R)) + bias
  ref0 = np.maximum(ref0, 0.0)
  err = np.abs(sparse0.cpu().numpy() - ref0).max() / np.abs(ref0).max()
  print('%s bf16 without long scales: against fp64 on the launch\'s Z %.2e' % (name, err))
  assert err <= 1e-5
  # exact fp32
  ldx = (din + 31) // 32 * 32
  X32 = _t(np.pad(X, ((0, 0), (0, 0), (0, ldx - din))))
  Wn32 = _t(np.pad(W[:, S:], ((0, 0), (0, 0), (0, ldx - din))).transpose(1, 0, 2).reshape(R * 128, ldx))
  Vb3 = ops.large_pack_vectors(Vd, 3)

  def work32():
    return ops.large_sparse_work_buffers(B, N, DEV, R=R, planes=3)
  s32 = ops.large_sparse_conv_layer(X32, din, imgs, Vb3, Vd, Wn32, None, None, bd, work32(), 3)
  assert ops.last_kernel() == 'sparse_conv_channels_f32_kernel'
  t32 = ops.large_sparse_conv_layer(X32, din, imgs, Vb3, Vd, Wn32, None, None, bd, work32(), 3)
  assert torch.equal(s32, t32)
  Z64 = np.einsum('bnd,ocd->cbno', X.astype(np.float64), W[:, S:].astype(np.float64))
  ref32 = sum(np.einsum('bnm,bmo->bno', A[..., c].astype(np.float64), Z64[c]) for c in range(R)) + bias
  ref32 = np.maximum(ref32, 0.0)
  err = np.abs(s32.cpu().numpy() - ref32).max() / np.abs(ref32).max()
  print('%s fp32: against the float64 einsum %.2e' % (name, err))
  assert err <= 1e-5


# ---- 6. the module ---------------------------------------------------------------------------------------------
def _cfg(K, E, num_layer=2):
  from large_fixture import general_cfg
  return dict(general_cfg(K, num_layer), long_diffusion_dist=[1, 2, 3], num_bond_type=E)


def _net(cfg, P, gemm_mode, **attrs):
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  net = LanczosNetGeneral(make_model_config(cfg, general=True)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV)
  net.gemm_mode = gemm_mode
  for k, v in attrs.items():
    setattr(net, k, v)
  return net


def _forward(net, b, L=None):
  return net(b['node_feat'], b['L'] if L is None else L, b['D'], b['V'], mask=b['node_mask'])


# The forward's spectral term sums its row chunks with float atomics (csrc/conv_large.hip, large_project_kernel):
# with three workgroups per graph at B 3, N 301 two runs of the SAME route on identical inputs may round an
# entry of the bf16 T differently (measured here: typed against 'each' on bit-identical images 0.0 in one run,
# 1.01e-5 in the next, bf16 mode, E = 3).  As in tests/test_gpu_edge_collate.py the module check therefore runs
# in a process of its own with LNZ_LARGE_PROJECT_WGS=1 (the library's knob, read once per process: one
# workgroup per graph, one adder per sum); the bars stay as they are.
def _check_module(E):
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_edges
  graphs, N = _three(E)
  cfg = _cfg(20, E)
  P = oracle.make_lanczosnet_params(cfg, 17, general=True)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    b = collate_graph_edges(tg.items(graphs, E), 20, device=DEV, num_edge_type=E)
  sl = b['L']
  assert isinstance(sl, ops.SparseLaplacian) and sl.channels == E + 1
  Ld = sl.to_dense()
  idx = torch.device(DEV).index
  with torch.no_grad():
    for mode, attrs, kernel, bar in (('fp32', dict(large_split_planes=2), 'sparse_conv_channels_f32_kernel', 1e-5),
                                     ('fp32', dict(large_split_planes=3), 'sparse_conv_channels_f32_kernel', 1e-5),
                                     ('bf16', {}, 'sparse_conv_channels_kernel', 2e-2)):
      net = _net(cfg, P, mode, **attrs)
      with _no_densify():
        se = _forward(net, b)
      st = net._large_sparse_state[idx]
      assert ops.last_kernel() == kernel and st['image_from'] == 'edges' and st['last_flags'] == 0
      off = _net(cfg, P, mode, large_sparse=False, **attrs)
      sd = _forward(off, b, Ld)
      assert not getattr(off, '_large_sparse_state', {})                      # the streamed kernels served it
      each = _net(cfg, P, mode, large_sparse_channels='each', **attrs)
      sc = _forward(each, b, Ld)
      assert ops.last_kernel() == kernel and each._large_sparse_state[idx]['last_flags'] == 0
      print('E %d %s %s: typed sparse against the streamed kernels %.2e, against \'each\' on the dense tensor %.2e'
            % (E, mode, attrs, _rel(se, sd), _rel(sc, se)))
      assert _rel(se, sd) <= bar
      assert _rel(sc, se) <= 1e-5
  wrong = dict(cfg, num_bond_type=E + 1)
  net = _net(wrong, oracle.make_lanczosnet_params(wrong, 17, general=True), 'fp32')
  with torch.no_grad(), pytest.raises(ValueError, match='operator channels'):
    _forward(net, b)


@functools.lru_cache(maxsize=None)
def _module_checks():
  """Both edge-type counts in ONE child process (fixed summation order, see above) -> {E: (ok, output)}."""
  import subprocess
  env = dict(os.environ, LNZ_LARGE_PROJECT_WGS='1')
  r = subprocess.run([sys.executable, os.path.abspath(__file__), '2', '3'], env=env, capture_output=True, text=True,
                     timeout=600)
  return {E: ('CHECK %d OK' % E in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]) for E in (2, 3)}


@pytest.mark.parametrize('E', [2, 3])
def test_module_takes_the_typed_sparse_laplacian(E):
  """LanczosNetGeneral with num_edge_type E on the typed SparseLaplacian: fp32 mode (planes 2 and 3) within 1e-5
  and bf16 mode within 2e-2 of a module with the sparse layers off on `sl.to_dense()`; last_kernel() names the
  new gather, no densify warning; a dense L with large_sparse_channels = 'each' gives the typed scores within
  1e-5; a num_edgetype that does not match the batch raises."""
  ok, text = _module_checks()[E]
  print(text)
  assert ok


# ---- 7. one edge type ---------------------------------------------------------------------------------------------
def test_num_edge_type_1_is_the_untyped_collate():
  from lanczosnet_amd import ops
  from lanczosnet_amd.dataset import collate_graph_edges
  graphs, N = eg.case('n301')
  its = eg.items(graphs)
  zero = [dict(it, edge_type=np.zeros(g['edges'].shape[0], np.int64)) for it, g in zip(its, graphs)]
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    a = collate_graph_edges(its, 20, device=DEV)
    b = collate_graph_edges(zero, 20, device=DEV, num_edge_type=1)
  assert set(a) == set(b)
  for key in a:
    if key != 'L':
      assert torch.equal(a[key], b[key]), key
  la, lb = a['L'], b['L']
  assert isinstance(lb, ops.SparseLaplacian) and lb.channels == la.channels == 2 and lb.images is None
  assert lb.edge_type is None and torch.equal(la.edges, lb.edges) and torch.equal(la.edge_off, lb.edge_off)
  assert torch.equal(la.image.counts, lb.image.counts) and int(lb.image.flags.item()) == 0
  _same_image(la.image, lb.image)


# ---- 8. the unmodified reference ------------------------------------------------------------------------------------
def test_typed_module_matches_the_reference_scores():
  """tests/golden/typed_edges.npz (tests/golden/make_golden_typed_edges.py): two typed graphs padded to 301
  nodes, E = 2, the reference's get_laplacian / get_graph_laplacian_eigs / LanczosNetGeneral on CPU.  The HIP
  module on the typed SparseLaplacian with the fixture's (D, V), fp32 mode: 1e-5 relative."""
  from lanczosnet_amd import ops
  z = np.load(GOLDEN)
  E, N, K = int(z['num_edge_type']), int(z['N']), int(z['K'])
  cfg = dict(_cfg(K, E, int(z['num_layer'])), long_diffusion_dist=[int(x) for x in z['long_diffusion_dist']])
  P = oracle.make_lanczosnet_params(cfg, int(z['param_seed']), general=True)
  sl = ops.sparse_laplacian_from_edges(_t(z['edges']), _t(z['edge_off']), _t(z['n_nodes']), N,
                                       edge_type=_t(z['edge_type']), num_edge_type=E)
  net = _net(cfg, P, 'fp32')
  with torch.no_grad(), _no_densify():
    score = net(_t(z['node_feat']), sl, _t(z['D']), _t(z['V']), mask=_t(z['node_mask']))
  assert ops.last_kernel() == 'sparse_conv_channels_f32_kernel'
  ref = _t(z['score'])
  print('typed module against the reference scores: %.2e relative' % _rel(score, ref))
  assert _rel(score, ref) <= 1e-5


if __name__ == '__main__':
  import traceback
  for arg in sys.argv[1:]:
    try:
      _check_module(int(arg))
      print('CHECK %s OK' % arg)
    except Exception:   # noqa: BLE001  (reported to the parent, check by check)
      traceback.print_exc()
      print('CHECK %s FAILED' % arg)
