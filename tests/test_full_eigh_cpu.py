"""Host-side contract of the full eigendecomposition entry (lnz_sym_eigh_topk): the header, the
library and the dispatcher expose it, the workspace query answers without a device, and every
refusal happens before anything is launched.  Runs without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from lanczosnet_amd import _lib, _torch_ext, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ('lnz_sym_eigh_topk_workspace_bytes', 'lnz_sym_eigh_topk')


def _call(A, B, N, K, ws=None, ws_bytes=0, D=None, V=None):
  lib = _lib.load()
  return lib.lnz_sym_eigh_topk(A, N, 1, 1, None, B, N, K, ws, ws_bytes, D, V, None, None)


def test_header_library_and_dispatcher_expose_the_entry():
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  for s in SYMS:
    assert re.search(r'\b%s\s*\(' % s, hdr), s
    assert s in _lib.SIGNATURES
    assert hasattr(_lib.load(), s)
  assert 'lnz_sym_eigh_topk' in hdr.split('#define LNZ_ABI_VERSION')[0]   # in the "7:" change log
  assert _lib.load().lnz_abi_version() == 7
  _torch_ext.load()
  assert hasattr(torch.ops.lanczosnet, 'raw_sym_eigh_topk')
  assert hasattr(torch.ops.lanczosnet, 'raw_sym_eigh_topk_workspace_bytes')


def test_workspace_query_answers_on_the_host_and_grows_with_B_and_N():
  q = _lib.load().lnz_sym_eigh_topk_workspace_bytes
  one = q(1, 2048, 64)
  assert one >= 2048 * 2048 * 8            # the fp64 copy of the matrix at least
  assert q(4, 2048, 64) == 4 * one
  assert q(1, 1024, 64) < one and q(1, 2048, 256) > one
  assert q(1, 2049, 64) == 0 and q(1, 2048, 257) == 0 and q(0, 2048, 64) == 0
  assert ops._abi().sym_eigh_topk_workspace_bytes(3, 300, 40) == q(3, 300, 40)


def test_refusals_before_any_launch():
  lib = _lib.load()
  buf = C.create_string_buffer(64)
  dummy = C.cast(buf, C.c_void_p)
  rc = _call(dummy, 1, 2049, 64, dummy, 1 << 40, dummy, dummy)
  assert rc == _lib.LNZ_ENOTSUP
  assert b'2048' in lib.lnz_last_error()
  rc = _call(dummy, 1, 64, 257, dummy, 1 << 40, dummy, dummy)
  assert rc == _lib.LNZ_ENOTSUP and b'256' in lib.lnz_last_error()
  rc = _call(dummy, 1, 64, 0, dummy, 1 << 40, dummy, dummy)
  assert rc in (_lib.LNZ_EINVAL, _lib.LNZ_ENOTSUP)
  rc = _call(None, 1, 64, 8, dummy, 1 << 40, dummy, dummy)
  assert rc == _lib.LNZ_EINVAL
  rc = _call(dummy, 1, 64, 8, dummy, 16, dummy, dummy)            # workspace too small
  assert rc == _lib.LNZ_EINVAL and b'workspace' in lib.lnz_last_error()


def test_batch_limit_per_call_is_refused_and_the_front_end_codes_match_the_entry():
  lib = _lib.load()
  buf = C.create_string_buffer(64)
  dummy = C.cast(buf, C.c_void_p)
  rc = _call(dummy, 65536, 8, 4, dummy, 1 << 60, dummy, dummy)
  assert rc == _lib.LNZ_EINVAL and b'65535' in lib.lnz_last_error()
  assert ops.SYM_EIGH_MAX_B == 65535   # the front end's chunk limit


def test_ops_front_end_has_no_cpu_fallback():
  A = torch.zeros((2, 8, 8))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    ops.sym_eigh_topk(A, torch.tensor([8, 8], dtype=torch.int32), 4)
  L = torch.zeros((2, 8, 8, 2))
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    ops.lanczos_ritz_collated(L, torch.tensor([8, 8], dtype=torch.int32), 4, method='full')


def test_full_method_refuses_the_krylov_switch():
  from lanczosnet_amd.utils.data_helper import get_graph_laplacian_eigs_batched
  A = torch.zeros((1, 8, 8))
  with pytest.raises(ValueError):
    get_graph_laplacian_eigs_batched(A, None, 4, use_eigen_decomp=False, method='full')
  with pytest.raises(ValueError):
    get_graph_laplacian_eigs_batched(A, None, 4, method='nope')
  with pytest.raises(ValueError):
    ops.lanczos_ritz_collated(torch.zeros((1, 8, 8, 2)), None, 4, method='nope')
