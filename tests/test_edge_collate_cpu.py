"""Host-side checks of the edge-list surface (no GPU): the C ABI additions and their bindings, the
argument validation of dataset.collate_graph_edges, and the seeded graphs of tests/edge_graphs.py —
every "no overflow" case of tests/test_gpu_edge_collate.py stays inside BOTH row capacities (it cannot
pass through the densifying fallback unnoticed) and the overflow case exceeds them."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import edge_graphs as eg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('lnz_lanczos_ritz_kstep_edges', 'lnz_lanczos_ritz_kstep_edges_workspace_bytes',
       'lnz_lanczos_ritz_kstep_wide_edges', 'lnz_lanczos_ritz_kstep_wide_edges_workspace_bytes',
       'lnz_laplacian_l4_edges_image', 'lnz_laplacian_l4_edges_image_workspace_bytes')


def test_header_binding_and_extension_agree_on_the_new_entries():
  from lanczosnet_amd import _lib
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  assert re.search(r'#define LNZ_ABI_VERSION 7\b', hdr) and _lib.ABI_VERSION == 7
  inc = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'torch_ext_abi.inc')).read()
  sigs = open(os.path.join(ROOT, 'lanczosnet_amd', '_lib.py')).read()
  code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
  for name in NEW:
    m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, code, flags=re.S)
    assert m, name
    nargs = len(m.group(1).split(','))
    assert 'raw_' + name[4:] + '(' in inc, name
    row = re.search(r"'%s': \(C\.c_int(64)?, \[([^\]]*)\]\)" % name, sigs)
    assert row and len(row.group(2).split(',')) == nargs, name
    assert name.replace('_workspace_bytes', '') in hdr.split('#define LNZ_ABI_VERSION')[0], 'not in the change log'
  assert subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_torch_ext.py'), '--check']).returncode == 0


def test_library_checks_arguments_before_it_launches():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  assert lib.lnz_abi_version() == 7
  one, null = C.c_void_p(256), None
  wb = lib.lnz_lanczos_ritz_kstep_edges_workspace_bytes
  assert wb(0, 304, 64, 32) == 0 and wb(2, 304, 64, 32) > lib.lnz_lanczos_ritz_kstep_workspace_bytes(2, 304, 2, 64)
  assert wb(2, 304, 64, 128) > wb(2, 304, 64, 32) == wb(2, 304, 64, 0) > wb(1, 304, 64, 0)   # (staging: the larger capacity)
  wide = lib.lnz_lanczos_ritz_kstep_wide_edges_workspace_bytes
  assert wide(2, 2100, 8, 256, 72) > lib.lnz_lanczos_ritz_kstep_wide_workspace_bytes(2, 2100, 8, 256)
  assert lib.lnz_laplacian_l4_edges_image_workspace_bytes(3, 301, 32) >= 3 * 301 * (4 + 2 * 32)
  big = 1 << 40
  call = lambda N, M, K, cap, ccap, ent=one: lib.lnz_lanczos_ritz_kstep_edges(   # noqa: E731
      one, 10, one, one, 2, N, M, K, cap, 1, one, big, one, one, null, null, ent, null, one, ccap, 1, one, one, null)
  assert call(2052, 8, 8, 64, 32) == _lib.LNZ_ENOTSUP and b'2048' in lib.lnz_last_error()
  assert call(304, 65, 8, 64, 32) == _lib.LNZ_ENOTSUP
  assert call(301, 8, 8, 64, 32) == _lib.LNZ_ENOTSUP and b'N % 4' in lib.lnz_last_error()
  assert call(304, 8, 8, 60, 32) == _lib.LNZ_EINVAL and b'row_cap' in lib.lnz_last_error()
  assert call(304, 8, 8, 264, 32) == _lib.LNZ_EINVAL and b'row_cap' in lib.lnz_last_error()
  assert call(304, 8, 8, 64, 20) == _lib.LNZ_EINVAL and b'conv_row_cap' in lib.lnz_last_error()
  assert lib.lnz_lanczos_ritz_kstep_edges(one, 10, one, one, 2, 304, 8, 8, 64, 3, one, big, one, one, null, null, null,
                                          null, null, 0, 0, null, one, null) == _lib.LNZ_EINVAL
  assert b'LNZ_EDGE_ORDER' in lib.lnz_last_error()
  assert lib.lnz_lanczos_ritz_kstep_edges(one, 10, one, one, 2, 304, 8, 8, 64, 1, one, 1000, one, one, null, null, null,
                                          null, null, 0, 0, null, one, null) == _lib.LNZ_EINVAL
  assert b'workspace of 1000 bytes' in lib.lnz_last_error()
  assert lib.lnz_lanczos_ritz_kstep_edges(one, 10, one, one, 2, 304, 8, 8, 64, 1, one, big, one, one, null, null, null,
                                          null, null, 0, 0, null, null, null) == _lib.LNZ_EINVAL   # no status
  widec = lambda N, M, K: lib.lnz_lanczos_ritz_kstep_wide_edges(   # noqa: E731
      one, 10, one, one, 2, N, M, K, 64, 1, one, big, one, one, null, null, null, null, null, 0, 0, null, one, null)
  assert widec(16388, 8, 8) == _lib.LNZ_ENOTSUP and widec(4096, 257, 8) == _lib.LNZ_ENOTSUP
  assert widec(4096, 8, 9) == _lib.LNZ_ENOTSUP
  assert lib.lnz_laplacian_l4_edges_image(one, 10, one, one, 2, 301, one, big, null, null, one, 32, 0, one, one,
                                          null) == _lib.LNZ_EINVAL
  assert lib.lnz_laplacian_l4_edges_image(one, 10, one, one, 2, 20000, one, big, one, null, one, 32, 0, one, one,
                                          null) == _lib.LNZ_ENOTSUP
  assert lib.lnz_laplacian_l4_edges_image(one, -1, one, one, 2, 301, one, big, one, null, one, 32, 0, one, one,
                                          null) == _lib.LNZ_EINVAL


def test_collate_graph_edges_validates_its_arguments():
  from lanczosnet_amd.dataset import collate_graph_edges
  good = eg.items(eg.case('n301')[0])
  with pytest.raises(ValueError, match='non-empty'):
    collate_graph_edges([], 20)
  with pytest.raises(ValueError, match="no 'edges'"):
    collate_graph_edges([dict(node_feat=good[0]['node_feat'], label=good[0]['label'])], 20)
  with pytest.raises(ValueError, match=r'\[m, 2\]'):
    collate_graph_edges([dict(good[0], edges=np.zeros((5, 3), np.int32))], 20)
  with pytest.raises(ValueError, match='integer'):
    collate_graph_edges([dict(good[0], edges=good[0]['edges'].astype(np.float32))], 20)
  with pytest.raises(ValueError, match='lanczos_steps'):
    collate_graph_edges(good, 20, lanczos_steps=10)
  with pytest.raises(ValueError, match='num_eigs'):
    collate_graph_edges(good, -1)
  big = dict(node_feat=np.zeros((16385, 2), np.float32), label=np.zeros((1, 2)), edges=np.zeros((0, 2), np.int32))
  with pytest.raises(ValueError, match='16384'):
    collate_graph_edges([big], 8)
  with pytest.raises(ValueError, match='self loop'):   # (small batches are densified on the host)
    collate_graph_edges([dict(node_feat=np.zeros((5, 2), np.float32), label=np.zeros((1, 2)),
                              edges=np.array([[1, 1]]))], 2)


def test_sparse_laplacian_answers_like_the_dense_tensor():
  import torch
  from lanczosnet_amd import ops
  z = torch.zeros((3,), dtype=torch.int32)
  img = ops.LargeSparseImage(torch.zeros((3, 301, 32), dtype=torch.int32), torch.zeros((3, 301), dtype=torch.int32),
                             torch.zeros((1,), dtype=torch.int32), 32, torch.zeros((3, 301, 32)))
  sl = ops.SparseLaplacian(3, 301, z, img, torch.zeros((0, 2), dtype=torch.int32), torch.zeros((4,), dtype=torch.int64))
  assert tuple(sl.shape) == (3, 301, 301, 2) and sl.dtype == torch.float32 and sl.device == z.device
  assert sl.dim() == 4 and sl.to('cpu') is sl and sl.image.values is not None
  with pytest.raises(RuntimeError, match='AMD GPU'):   # no CPU path
    ops.lanczos_ritz_edges(sl.edges, sl.edge_off, sl.n_nodes, 301, 20)
  assert [bit for bit, _ in ops.EDGE_STATUS_REASONS] == [1, 2, 4, 8, 16]
  # the dense route's entry orders: the pair in place when it is aligned, else a contiguous copy / the 4-byte walk
  assert ops.dense_entry_orders(2048) == (ops.EDGE_ORDER_PAIR, ops.EDGE_ORDER_PAIR)
  assert ops.dense_entry_orders(302) == (ops.EDGE_ORDER_QUAD, ops.EDGE_ORDER_PAIR)
  assert ops.dense_entry_orders(301) == (ops.EDGE_ORDER_QUAD, ops.EDGE_ORDER_ASCENDING)
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  for name in ('ASCENDING', 'PAIR', 'QUAD'):
    assert re.search(r'#define LNZ_EDGE_ORDER_%s %d\b' % (name, getattr(ops, 'EDGE_ORDER_' + name)), hdr)


@pytest.mark.parametrize('name', sorted(eg.CASES))
def test_no_overflow_cases_stay_inside_both_capacities(name):
  from lanczosnet_amd import ops
  graphs, N = eg.case(name)
  Np = (N + 3) // 4 * 4
  assert eg.conv_cap(N) == ops.large_sparse_row_cap(N)
  longest = eg.max_row_entries(graphs)
  assert longest <= min(ops.kstep_row_cap(Np), ops.large_sparse_row_cap(N)), (name, longest)
  assert max(g['n'] for g in graphs) == N and graphs[-1]['n'] < N        # ragged
  for g in graphs:
    e = g['edges']
    assert e.dtype == np.int32 and (e.size == 0 or (0 <= e.min() and e.max() < g['n']))
    assert not (e[:, 0] == e[:, 1]).any()
    code = np.minimum(e[:, 0], e[:, 1]).astype(np.int64) * N + np.maximum(e[:, 0], e[:, 1])
    assert np.unique(code).shape[0] == e.shape[0]                        # a simple graph
    if g['n'] > 0:
      rows = eg.row_entries(g)
      assert list(rows[-4:]) == [ops.large_sparse_row_cap(N), 8, 9, 1]   # at the capacity, 8, 9, isolated
  if name != 'n4096':
    assert graphs[-1]['n'] == 0 and graphs[-1]['edges'].shape[0] == 0    # one empty graph
  assert sorted(np.concatenate([g['edges'] for g in eg.shuffled(graphs, 3)]).tolist()) != \
      sorted(np.concatenate([g['edges'] for g in graphs]).tolist())      # (the shuffle does swap endpoints)


def test_overflow_case_exceeds_both_capacities_and_small_case_is_small():
  from lanczosnet_amd import ops
  graphs, N = eg.star_case()
  assert int(eg.row_entries(graphs[0]).max()) == 301 > max(ops.kstep_row_cap(304), ops.large_sparse_row_cap(301))
  assert eg.max_row_entries(graphs[1:]) <= min(ops.kstep_row_cap(304), ops.large_sparse_row_cap(301))
  small, Ns = eg.small_case()
  assert Ns == max(g['n'] for g in small) <= ops.RITZ_FULL_MAX_N and min(g['n'] for g in small) == 20
