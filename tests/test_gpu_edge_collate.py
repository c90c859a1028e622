"""GPU checks of large graphs from edge lists (csrc/edge_image.hip; lnz_lanczos_ritz_kstep_edges,
lnz_lanczos_ritz_kstep_wide_edges, lnz_laplacian_l4_edges_image; ops.lanczos_ritz_edges,
dataset.collate_graph_edges, the module's SparseLaplacian input) against the DENSE route on the same
graphs: dense adjs -> ops.laplacian_l4 -> the existing entries with the same row_cap.  The step and
gather kernels are the same code on an image that must be the same bits: the bar is torch.equal.
Graphs: tests/edge_graphs.py (tests/test_edge_collate_cpu.py shows that the no-overflow cases stay
inside both row capacities, so none of them passes through the densifying fallback)."""
import contextlib
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the module checks run this file as a script)
  sys.path.insert(0, ROOT)

import edge_graphs as eg  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@contextlib.contextmanager
def _no_densify():
  """The densifying fallbacks announce themselves: inside, that warning is an error."""
  with warnings.catch_warnings():
    warnings.filterwarnings('error', message='.*densified.*')
    yield


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _packed(graphs):
  return tuple(_t(a) for a in eg.pack(graphs))


@functools.lru_cache(maxsize=None)
def _dense(name):
  """graphs, N, the dense route's L [B,N,N,2] and its image (computed once, shared, left unchanged)."""
  from lanczosnet_amd import ops
  graphs, N = eg.star_case() if name == 'star' else eg.case(name)
  L = ops.laplacian_l4(_t(eg.dense_adjs(graphs, N)), _t(eg.pack(graphs)[2]))
  return graphs, N, L, ops.large_sparse_image(L, values=True)


def _three():
  """Three non-empty graphs padded to 301 nodes (the validation and module checks)."""
  graphs, N = eg.case('n301')
  rs = np.random.RandomState(31)
  n = 150
  return graphs[:2] + [dict(n=n, edges=eg.with_special_rows(n, eg.gnp_edges(n, 0.03, rs), eg.conv_cap(N)))], N


def _used(counts, cap):
  """[B,N,cap] mask of each row's first ceil(count / 8) * 8 slots (the slots the gather reads)."""
  return torch.arange(cap, device=counts.device)[None, None, :] < ((counts + 7) // 8 * 8)[:, :, None]


def _same_image(a, b):
  assert a.cap == b.cap and torch.equal(a.counts, b.counts)
  m = _used(a.counts, a.cap)
  assert torch.equal(a.entries[m], b.entries[m])
  assert torch.equal(a.values[m], b.values[m])


# ---- 1. the image -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['n301', 'n256', 'n200'])
def test_image_from_edges_is_the_dense_compaction_bit_for_bit(name):
  from lanczosnet_amd import ops
  graphs, N, L, ref = _dense(name)
  sl = ops.sparse_laplacian_from_edges(*_packed(graphs), N)
  img = sl.image
  assert int(img.flags.item()) == 0 and int(ref.flags.item()) == 0 and img.cap == ops.large_sparse_row_cap(N)
  _same_image(img, ref)
  counts, ent, val = img.counts.cpu().numpy(), img.entries.cpu().numpy(), img.values.cpu().numpy()
  worst = 0.0
  for b, g in enumerate(graphs):
    assert (counts[b, g['n']:] == 0).all()                                   # rows >= n_b are empty
    for i, (cols, v64) in enumerate(eg.l4_rows_fp64(g)):
      c = counts[b, i]
      assert c == cols.shape[0]
      got = ent[b, i, :c] & 0xffff
      at = np.argsort(got, kind='stable')                                    # (the entry order is the dense route's)
      assert (got[at] == cols).all()                                         # the neighbours and the diagonal, once each
      worst = max(worst, float(np.abs(val[b, i, :c][at].astype(np.float64) - v64).max()))
      pad = (c + 7) // 8 * 8
      assert (ent[b, i, c:pad] == 0).all() and (val[b, i, c:pad] == 0).all()
    if g['n']:
      assert list(counts[b, g['n'] - 4:g['n']]) == [img.cap, 8, 9, 1]        # at the capacity, 8, 9, isolated
  print('%s: values against the fp64 formula, max abs %.2e' % (name, worst))
  assert worst < 1e-7
  assert torch.equal(sl.to_dense(), L)


# ---- 2. a pure function of the edge set ---------------------------------------------------------------
def test_edge_and_endpoint_order_do_not_change_a_bit():
  from lanczosnet_amd import ops
  graphs, N, L, ref = _dense('n301')
  with _no_densify():
    base = ops.lanczos_ritz_edges(*_packed(graphs), N, 20, return_info=True)
    again = ops.lanczos_ritz_edges(*_packed(graphs), N, 20, return_info=True)
    mixed = ops.lanczos_ritz_edges(*_packed(eg.shuffled(graphs, 41)), N, 20, return_info=True)
  for other in (again, mixed):
    assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1]) and torch.equal(base[3], other[3])
    _same_image(base[2].image, other[2].image)
  a = ops.sparse_laplacian_from_edges(*_packed(eg.shuffled(graphs, 42)), N)
  _same_image(a.image, ref)


# ---- 3. Ritz pairs ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,M,K,wide', [('n301', 20, 20, False), ('n256', 40, 20, False), ('n2100', 8, 8, True),
                                           ('n300', 72, 16, True)])
def test_ritz_pairs_equal_the_dense_route(name, M, K, wide):
  from lanczosnet_amd import ops
  graphs, N, L, ref = _dense(name)
  n = _packed(graphs)[2]
  with _no_densify():
    D, V, sl, info = ops.lanczos_ritz_edges(*_packed(graphs), N, K, lanczos_steps=M, return_info=True)
    kernel = ops.last_kernel()
    Dr, Vr, infor = ops.lanczos_ritz_kstep(L[..., 0], n, M, K, return_info=True)
  assert ('wide' in kernel) == wide and ('wide' in ops.last_kernel()) == wide
  assert wide or kernel == 'edge_rows_kernel, lanczos_ritz_large_kernel<2>'
  print('%s M %d K %d: max |D - D_dense| %.2e  max |V - V_dense| %.2e  steps %s' %
        (name, M, K, float((D - Dr).abs().max()), float((V - Vr).abs().max()), info.tolist()))
  assert torch.equal(info, infor) and torch.equal(D, Dr) and torch.equal(V, Vr)
  assert int(sl.image.flags.item()) == 0                                     # the conv image: narrow AND wide
  _same_image(sl.image, ref)


# ---- 4. a row beyond the capacities -------------------------------------------------------------------
def test_overflow_is_flagged_per_graph_and_ops_takes_the_dense_route():
  from lanczosnet_amd import ops
  graphs, N, L, _ = _dense('star')
  edges, off, n = _packed(graphs)
  B, Np, K = 2, 304, 20
  cap, ccap = ops.kstep_row_cap(Np), ops.large_sparse_row_cap(N)
  Dr, Vr = ops.lanczos_ritz_kstep(L[..., 0], n, K, K)
  need = ops._abi().lanczos_ritz_kstep_edges_workspace_bytes(B, Np, cap, ccap)
  ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
  D, V = torch.full((B, K), 7.0, device=DEV), torch.full((B, Np, K), 7.0, device=DEV)
  i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=DEV)   # noqa: E731
  info, over, status, counts, flags = i32(B), i32(B), i32(B), i32(B, Np), i32(1)
  row_order, conv_order = ops.dense_entry_orders(N)
  ops._abi().lanczos_ritz_kstep_edges(edges, edges.shape[0], off, n, B, Np, K, K, cap, row_order, ws, need, D, V, info,
                                      over, i32(B, Np, ccap), None, counts, ccap, conv_order, flags, status)
  assert over.tolist() == [1, 0] and status.tolist() == [0, 0] and int(flags.item()) == 2
  assert not D[0].any() and not V[0].any() and int(info[0]) == 0            # the star left at once
  assert torch.equal(D[1], Dr[1]) and torch.equal(V[1, :N], Vr[1]) and not V[1, N:].any()
  with pytest.warns(UserWarning, match='densified'):
    D2, V2, sl = ops.lanczos_ritz_edges(edges, off, n, N, K)
  assert torch.equal(D2, Dr) and torch.equal(V2, Vr) and int(sl.image.flags.item()) == 2


# ---- 5. validation on the device ------------------------------------------------------------------------
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


def _c_call(edges, off, n, N, K):
  """lnz_lanczos_ritz_kstep_edges with every output and the workspace between sentinels."""
  from lanczosnet_amd import ops
  B, Np = n.shape[0], (N + 3) // 4 * 4
  cap, ccap = ops.kstep_row_cap(Np), ops.large_sparse_row_cap(N)
  need = ops._abi().lanczos_ritz_kstep_edges_workspace_bytes(B, Np, cap, ccap)
  g = _Guarded()
  o = dict(ws=g((need,), torch.uint8), D=g((B, K), torch.float32), V=g((B, Np, K), torch.float32),
           info=g((B,), torch.int32), over=g((B,), torch.int32), entries=g((B, Np, ccap), torch.int32),
           values=g((B, Np, ccap), torch.float32), counts=g((B, Np), torch.int32), flags=g((1,), torch.int32),
           status=g((B,), torch.int32))
  row_order, conv_order = ops.dense_entry_orders(N)
  ops._abi().lanczos_ritz_kstep_edges(edges, edges.shape[0], off, n, B, Np, K, K, cap, row_order, o['ws'], need, o['D'],
                                      o['V'], o['info'], o['over'], o['entries'], o['values'], o['counts'], ccap,
                                      conv_order, o['flags'], o['status'])
  torch.cuda.synchronize()
  assert g.intact()
  return o


@functools.lru_cache(maxsize=None)
def _clean_three():
  graphs, N = _three()
  return _c_call(*_packed(graphs), N, 20)


@pytest.mark.parametrize('what,bad,bit', [('endpoint', 1, 1), ('self loop', 1, 2), ('duplicate', 1, 4), ('offsets', 2, 8)])
def test_bad_graph_is_flagged_alone_and_nothing_else_moves(what, bad, bit):
  from lanczosnet_amd import ops
  graphs, N = _three()
  graphs = [dict(g, edges=g['edges'].copy()) for g in graphs]
  e = graphs[1]['edges']
  if what == 'endpoint':
    e[3, 1] = graphs[1]['n']                 # inside the padded N, outside the graph
  elif what == 'self loop':
    e[3] = (5, 5)
  elif what == 'duplicate':
    graphs[1]['edges'] = np.concatenate([e, e[:1, ::-1]], axis=0)
  edges, off, n = eg.pack(graphs)
  if what == 'offsets':
    off[3] = off[2] - 1                      # the last graph's range runs backwards
  edges, off, n = _t(edges), _t(off), _t(n)
  clean, got = _clean_three(), _c_call(edges, off, n, N, 20)
  assert got['status'].tolist() == [bit if b == bad else 0 for b in range(3)]
  assert got['over'].tolist() == [0, 0, 0] and int(clean['flags'].item()) == 0
  for key in ('D', 'V', 'info', 'counts', 'entries', 'values'):
    assert not got[key][bad].any(), key                                       # its outputs are zeros
  used = _used(clean['counts'], clean['entries'].shape[2])
  for b in (b for b in range(3) if b != bad):
    for key in ('D', 'V', 'info', 'counts'):
      assert torch.equal(got[key][b], clean[key][b]), key
    for key in ('entries', 'values'):
      assert torch.equal(got[key][b][used[b]], clean[key][b][used[b]]), key
  with pytest.raises(ValueError, match='graph %d .*%s' % (bad, {1: 'endpoint', 2: 'self loop', 4: 'duplicate',
                                                                8: 'edge_off'}[bit])):
    ops.lanczos_ritz_edges(edges, off, n, N, 20)
  with pytest.raises(ValueError, match='graph %d' % bad):
    ops.sparse_laplacian_from_edges(edges, off, n, N)


# ---- 6. the module -----------------------------------------------------------------------------------------
def _net(K, gemm_mode):
  from large_fixture import general_cfg
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  cfg = dict(general_cfg(K, 2), long_diffusion_dist=[1, 2, 3])
  P = oracle.make_lanczosnet_params(cfg, 17, general=True)
  net = LanczosNetGeneral(make_model_config(cfg, general=True)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV)
  net.gemm_mode = gemm_mode
  return net


def _batches(graphs, K):
  from lanczosnet_amd.dataset import collate_graph_adjacency, collate_graph_edges
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    return (collate_graph_edges(eg.items(graphs), K, device=DEV),
            collate_graph_adjacency(eg.items(graphs, dense=True), K, device=DEV))


def _forward(net, b):
  return net(b['node_feat'], b['L'], b['D'], b['V'], mask=b['node_mask'])


# The forward's spectral term sums its row chunks with float atomics (csrc/conv_large.hip,
# large_project_kernel): with more than one workgroup per graph — three at B 3, N 301 — the scores of
# two runs of the SAME route differ in the last bit now and then (measured here: bf16 0, fp32 7.45e-9 =
# 1 ulp between the edge and the dense batch on identical inputs).  "Equal" is a property of a route
# only under a fixed summation order, so the two checks below run in a process of their own with
# LNZ_LARGE_PROJECT_WGS=1 (the library's knob: one workgroup per graph, one adder per sum); the bar
# stays torch.equal.
def _check_sparse_path():
  from lanczosnet_amd import ops
  be, bd = _batches(_three()[0], 20)
  assert isinstance(be['L'], ops.SparseLaplacian) and tuple(be['L'].shape) == tuple(bd['L'].shape)
  for key in ('node_feat', 'node_mask', 'label', 'n_nodes', 'D', 'V'):
    assert torch.equal(be[key], bd[key]), key
  calls, orig = [], ops.large_sparse_image

  def spy(*a, **kw):
    calls.append(1)
    return orig(*a, **kw)
  for mode, kernel in (('bf16', 'sparse_conv_kernel'), ('fp32', 'sparse_conv_f32_kernel')):
    net = _net(20, mode)
    with torch.no_grad(), _no_densify():
      ops.large_sparse_image = spy
      try:
        se = _forward(net, be)
        st = net._large_sparse_state[torch.device(DEV).index]
        assert not calls and st['image_from'] == 'edges' and st['last_flags'] == 0 and ops.last_kernel() == kernel
      finally:
        ops.large_sparse_image = orig
      sd = _forward(net, bd)
      assert st['image_from'] != 'edges' and ops.last_kernel() == kernel
    print('%s: max |score_edges - score_dense| %.2e' % (mode, float((se - sd).abs().max())))
    assert torch.equal(se, sd)


def _check_densify():
  be, bd = _batches(_three()[0], 20)
  star_e, star_d = _batches(eg.star_case()[0], 20)
  # a raised conv flag (the star's row): the streamed kernels on the densified L
  net = _net(20, 'bf16')
  with torch.no_grad():
    with pytest.warns(UserWarning, match='densified') as rec:
      se = _forward(net, star_e)
    assert len([w for w in rec if 'densified' in str(w.message)]) == 1
    with _no_densify():                                                        # once per module
      _forward(net, star_e)
    sd = _forward(_net(20, 'bf16'), star_d)
  assert torch.equal(se, sd)
  # parameters that want gradients: the differentiable route
  ne, nd = _net(20, 'fp32'), _net(20, 'fp32')
  with pytest.warns(UserWarning, match='densified'):
    se = _forward(ne, be)
  sd = _forward(nd, bd)
  assert se.requires_grad and torch.equal(se, sd)
  se.sum().backward()
  sd.sum().backward()
  for (k, pe), pd in zip(ne.named_parameters(), nd.parameters()):
    assert pe.grad is not None and torch.equal(pe.grad, pd.grad), k



_CHECKS = {'sparse_path': _check_sparse_path, 'densify': _check_densify}


@functools.lru_cache(maxsize=None)
def _module_checks():
  """Both checks in ONE child process (fixed summation order, see above) -> {name: (ok, output)}."""
  import subprocess
  env = dict(os.environ, LNZ_LARGE_PROJECT_WGS='1')
  r = subprocess.run([sys.executable, os.path.abspath(__file__)] + sorted(_CHECKS), env=env, capture_output=True,
                     text=True, timeout=600)
  out = {}
  for name in _CHECKS:
    out[name] = ('CHECK %s OK' % name in r.stdout, r.stdout[-4000:] + r.stderr[-4000:])
  return out


@pytest.mark.parametrize('name', sorted(_CHECKS))
def test_module_on_sparse_laplacian_batches(name):
  """sparse_path: forward with the SparseLaplacian batch equals forward with collate_graph_adjacency's, bf16 and
  fp32, on the carried image with no image launch.  densify: the star batch (conv flag raised) and parameters
  that want gradients warn once and give the dense batch's scores (and gradients)."""
  ok, text = _module_checks()[name]
  print(text)
  assert ok


# ---- 7. no dense tensor -----------------------------------------------------------------------------------------
def test_edge_route_allocates_no_dense_channel():
  """collate_graph_edges + forward (bf16) at B 2, N 4096, M = K = 8.  Expected peak, from the buffers:
  the wide workspace lnz_lanczos_ritz_kstep_wide_edges_workspace_bytes(2, 4096, 8, 256, 128) = 17.6 MB
  (ELL image 2 x 64 slabs x 256 x 64 x 6 B = 12.6 MB, staged columns 2 x 4096 x 256 x 2 B = 4.2 MB, basis and
  vectors 0.7 MB) + the conv image 2 x 4096 x 128 x 8 B = 8.4 MB + D, V, features, edges 0.9 MB = about
  27 MB during the collate; the forward holds the image and about 12 MB of layer states instead of the
  workspace.  One dense channel is 2 x 4096^2 x 4 B = 134 MB; the bar is half of it (67 MB), and the dense
  route needs three channels at least.  Measured: see DESIGN.md 4.5f."""
  from lanczosnet_amd.dataset import collate_graph_edges
  graphs, N = eg.case('n4096')
  net = _net(8, 'bf16')
  its = eg.items(graphs)
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  with torch.no_grad(), warnings.catch_warnings():
    warnings.simplefilter('ignore')
    b = collate_graph_edges(its, 8, device=DEV)
    after_collate = torch.cuda.max_memory_allocated() - before
    with _no_densify():
      score = _forward(net, b)
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - before
  print('peak allocation: collate %.1f MB, collate + forward %.1f MB (one dense channel: %.1f MB)'
        % (after_collate / 1e6, peak / 1e6, 2 * N * N * 4 / 1e6))
  assert net._large_sparse_state[torch.device(DEV).index]['image_from'] == 'edges'
  assert torch.isfinite(score).all()
  assert peak < 2 * N * N * 4 / 2


# ---- 8. small batches ----------------------------------------------------------------------------------------------
def test_small_batches_are_densified_to_the_adjacency_collate():
  graphs, N = eg.small_case()
  be, bd = _batches(graphs, 16)
  assert set(be) == set(bd) and isinstance(be['L'], torch.Tensor) and be['L'].shape == (4, N, N, 2)
  for key in bd:
    assert torch.equal(be[key], bd[key]), key


if __name__ == '__main__':
  import traceback
  for check in sys.argv[1:]:
    try:
      _CHECKS[check]()
      print('CHECK %s OK' % check)
    except Exception:   # noqa: BLE001  (reported to the parent, check by check)
      traceback.print_exc()
      print('CHECK %s FAILED' % check)
