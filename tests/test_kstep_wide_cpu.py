"""The wide K-step entry (lnz_lanczos_ritz_kstep_wide: N <= 16384, K <= M <= 256) without a GPU: the
declaration and binding, the workspace query, the argument checks (nothing is launched), and the
Python surface's refusals."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_wide_entries_and_the_binding_has_them():
  from lanczosnet_amd import _lib
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  for name in ('lnz_lanczos_ritz_kstep_wide', 'lnz_lanczos_ritz_kstep_wide_workspace_bytes'):
    assert re.search(r'\b%s\s*\(' % name, hdr), name
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.load(), name)
  assert 'utils/data_helper.py:205-208' in hdr[hdr.index('for what one workgroup cannot hold') - 400:
                                               hdr.index('lnz_lanczos_ritz_kstep_wide_workspace_bytes(int')]
  assert '#define LNZ_ABI_VERSION 7' in hdr and _lib.ABI_VERSION == 7       # additive: the version stays


def test_wide_workspace_query_grows_with_the_steps():
  from lanczosnet_amd import _lib
  q = _lib.load().lnz_lanczos_ritz_kstep_wide_workspace_bytes
  B, N, cap = 2, 4096, 64
  sizes = [q(B, N, M, cap) for M in (64, 128, 256)]
  assert sizes[0] < sizes[1] < sizes[2]
  # the fp64 basis [B][M][N] is the bulk of the growth
  assert sizes[2] - sizes[0] >= B * (256 - 64) * N * 8
  assert q(B, N, 64, 256) > q(B, N, 64, 64)                       # the image's row capacity
  assert q(2 * B, N, 64, cap) > q(B, N, 64, cap)
  for bad in ((0, N, 64, cap), (B, 0, 64, cap), (B, N, 0, cap), (B, N, 64, 0), (-1, N, 64, cap), (B, -4, 64, cap)):
    assert q(*bad) == 0


def test_wide_entry_refuses_before_it_launches():
  from lanczosnet_amd import _lib
  lib = _lib.load()
  null = C.c_void_p(None)
  one = C.c_void_p(256)   # (a non-NULL, aligned "pointer": every call below fails before anything is touched)
  big = 1 << 50

  def call(N=4096, M=128, K=64, sc=1, A=one, ws=one, wsb=big, D=one, V=one, fb=one, cap=64):
    return lib.lnz_lanczos_ritz_kstep_wide(A, N * N * sc, N * sc, sc, null, 1, N, M, K, cap, ws, wsb, D, V, null,
                                           fb, null)
  assert call(N=16388) == _lib.LNZ_ENOTSUP
  assert b'16384' in lib.lnz_last_error()
  assert call(M=257, K=64) == _lib.LNZ_ENOTSUP
  assert b'256' in lib.lnz_last_error()
  assert call(M=64, K=65) == _lib.LNZ_ENOTSUP                      # K > M: the existing entry's code
  assert call(N=64, M=128, K=64) == _lib.LNZ_EINVAL                # M > N
  assert b'M=128 > N=64' in lib.lnz_last_error()
  for kw in (dict(A=null), dict(ws=null), dict(D=null), dict(V=null)):
    assert call(**kw) == _lib.LNZ_EINVAL
  need = lib.lnz_lanczos_ritz_kstep_wide_workspace_bytes(1, 4096, 128, 64)
  assert call(wsb=need - 1) == _lib.LNZ_EINVAL
  assert b'workspace' in lib.lnz_last_error()
  assert call(cap=12) == _lib.LNZ_EINVAL and b'row_cap' in lib.lnz_last_error()
  assert call(sc=3) == _lib.LNZ_ENOTSUP
  assert b'stride_c' in lib.lnz_last_error()
  assert call(sc=2, fb=null) == _lib.LNZ_ENOTSUP                   # the pair view needs the fallback flags
  assert call(N=4098) == _lib.LNZ_ENOTSUP                          # N % 4


def test_python_surface_refusals_without_gpu():
  import torch
  from lanczosnet_amd import _lib, ops
  from lanczosnet_amd.utils.data_helper import get_graph_laplacian_eigs_batched
  A = torch.zeros((1, 2304, 2304))
  with pytest.raises(Exception, match='no CPU fallback'):
    ops.lanczos_ritz_kstep(A, None, 96, 96)
  with pytest.raises(Exception, match='no CPU fallback'):
    ops.lanczos_ritz_kstep(A[:, :256, :256], None, 32, 32)
  k = 48
  with pytest.raises(ValueError, match='lanczos_steps'):
    get_graph_laplacian_eigs_batched(A, None, k, use_eigen_decomp=False, lanczos_steps=k - 1)
  with pytest.raises(ValueError, match='lanczos_steps'):
    get_graph_laplacian_eigs_batched(A, None, k, lanczos_steps=k - 1)
  with pytest.raises(ValueError, match='lanczos_steps'):
    get_graph_laplacian_eigs_batched(A, None, k, use_eigen_decomp=True, lanczos_steps=2 * k)
  with pytest.raises(ValueError, match='lanczos_steps'):
    ops.lanczos_ritz_collated(A[..., None], None, k, lanczos_steps=k - 1)
  assert (ops.KSTEP_WIDE_MAX_N, ops.KSTEP_WIDE_MAX_M) == (16384, 256)
  assert issubclass(_lib.NotSupported, NotImplementedError)
