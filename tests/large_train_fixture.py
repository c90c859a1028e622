"""Planted inputs of the kernel-level checks in tests/test_gpu_large_train.py (and the CPU check of
their preconditions in tests/test_large_train_cpu.py): numpy only.

EXACT cases in the manner of tests/large_edges_fixture.py (whose helpers these are): every operand of
lnz_large_grad_project / _spectral / _input is a small integer, every product and every partial sum an
integer below 2^24, so the fp32 result must EQUAL the float64 one whatever the summation order.  Each
builder asserts that precondition on its own inputs (`_check_below` on the sums of ABSOLUTE products)."""
import functools

import numpy as np

from large_edges_fixture import EXACT_LIMIT, _check_below, _ints, _sparse_signs

# (B, N, K, S, d)
GRAD_SHAPES = [
    (3, 193, 1, 1, 1),        # every extent at its minimum; one row in the seventh 32-row step
    (3, 257, 17, 16, 127),    # the scale limit, an odd width, the second 256-row chunk holds ONE row
    (10, 300, 64, 2, 128),    # the K limit, the full width, B not a multiple of 8
    (3, 256, 20, 8, 10),      # the reference's configuration; N exactly one chunk
]


def ragged_nodes(B, N):
  """Graph 0 fills the padding, the others lose 7, 14, ... nodes; the LAST graph has one node less than
  a multiple of 32 where that fits (a step whose last row is padding)."""
  n = np.array([N - 7 * b for b in range(B)], np.int32)
  n[-1] = max(1, (N - 1) // 32 * 32 - 1)
  assert n.min() >= 1 and n.max() == N
  return n


@functools.lru_cache(maxsize=None)
def project_case(B, N, K, S, d):
  """dX (integers in -8..8; NaN and huge values planted in the rows at or beyond n_nodes), Xout (integers
  in -2..2: about 2 in 5 positive), V (signs, zero at or beyond n_nodes) -> dP, db [B,128], A [B,K,128]."""
  rs = np.random.RandomState(3 * N + K + B)
  n = ragged_nodes(B, N)
  live = (np.arange(N)[None, :] < n[:, None])[:, :, None]
  g = _ints(rs, (B, N, 128), -8, 8)
  x = _ints(rs, (B, N, 128), -2, 2)
  V = _sparse_signs(rs, B, N, K, 40) * live
  dP = g * (x > 0) * live
  A = np.einsum('bnk,bno->bko', V, dP)
  db = dP.sum(axis=1)
  what = 'project_case(%d, %d, %d)' % (B, N, K)
  worst = _check_below(what + ' A', np.einsum('bnk,bno->bko', np.abs(V), np.abs(dP)))
  worst = max(worst, _check_below(what + ' db', np.abs(dP).sum(axis=1)))
  assert np.abs(A).max() > 0 and np.abs(db).max() > 0
  assert B < 2 or not np.array_equal(V[0], V[1])
  dirty = g.copy()
  junk = np.where(rs.rand(B, N, 128) < 0.5, np.nan, 3.0e38)
  dirty = np.where(live, dirty, junk)
  f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
  return dict(dX=f32(dirty), dX_clean=f32(g * live), Xout=f32(x), V=f32(V), n=n, dP=dP, A=A, db=db, worst=worst)


@functools.lru_cache(maxsize=None)
def spectral_case(B, N, K, S, d):
  """A [B,K,128] in -4..4, Y [B,K,ldy] in -2..2 (ldy = d rounded up to 32, NaN beyond d), G [B,S,K] in
  {-1,0,1}, W [128,(S+2) d]: long blocks in {-1,0,1}, NaN in the two edge-type blocks (never read)."""
  rs = np.random.RandomState(5 * K + S + d + B)
  ldy = (d + 31) // 32 * 32
  A = _ints(rs, (B, K, 128), -4, 4)
  Y = _ints(rs, (B, K, d), -2, 2)
  G = _ints(rs, (B, S, K), -1, 1)
  Wl = _ints(rs, (128, S, d), -1, 1, density=0.5)
  U = np.einsum('bko,osi->bksi', A, Wl)                        # [B,K,S,d]
  dG = np.einsum('bksi,bki->bks', U, Y)
  dY = np.einsum('bsk,bksi->bki', G, U)
  Q = G.transpose(0, 2, 1)[:, :, :, None] * Y[:, :, None, :]   # [B,K,S,d]
  what = 'spectral_case(%d, %d, %d, %d)' % (B, K, S, d)
  Ua = np.einsum('bko,osi->bksi', np.abs(A), np.abs(Wl))
  worst = _check_below(what + ' U', Ua)
  worst = max(worst, _check_below(what + ' dG', np.einsum('bksi,bki->bks', Ua, np.abs(Y))))
  worst = max(worst, _check_below(what + ' dY', np.einsum('bsk,bksi->bki', np.abs(G), Ua)))
  assert np.abs(dG).max() > 0 and np.abs(dY).max() > 0
  Yp = np.full((B, K, ldy), np.nan, np.float32)
  Yp[..., :d] = Y
  W = np.full((128, S + 2, d), np.nan, np.float32)
  W[:, :S] = Wl
  f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
  dYp = np.zeros((B, K, 128))
  dYp[..., :d] = dY
  return dict(A=f32(A), Y=Yp, G=f32(G), W=W.reshape(128, -1), dG=dG, Q=Q, dY=dYp, worst=worst)


@functools.lru_cache(maxsize=None)
def input_case(B, N, K, S, d):
  """dZ [B,N,128] in -4..4, Wn [128,128] in -2..2 (columns >= d zero), V signs [B,N,K], dY [B,K,128] in
  -8..8 with junk integers in its columns >= d (the launch masks them) -> dX [B,N,128], columns >= d zero."""
  rs = np.random.RandomState(7 * N + K + d + B)
  dZ = _ints(rs, (B, N, 128), -4, 4)
  Wn = _ints(rs, (128, 128), -2, 2, density=0.6)
  Wn[:, d:] = 0
  V = _sparse_signs(rs, B, N, K, 40)
  dY = _ints(rs, (B, K, 128), -8, 8)
  ref = np.zeros((B, N, 128))
  ref[..., :d] = (dZ @ Wn + V @ dY)[..., :d]
  what = 'input_case(%d, %d, %d, %d)' % (B, N, K, d)
  worst = _check_below(what, np.abs(dZ) @ np.abs(Wn) + np.abs(V) @ np.abs(dY))
  assert np.abs(ref).max() > 0 and (d == 128 or np.abs(dY[..., d:]).max() > 0)
  assert B < 9 or not np.array_equal(dZ[0], dZ[8])
  f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
  return dict(dZ=f32(dZ), Wn=f32(Wn), V=f32(V), dY=f32(dY), dX=ref, worst=worst)


def all_exact_cases():
  """Build every case (each asserts its own precondition) -> the worst bound met."""
  worst = 0.0
  for shape in GRAD_SHAPES:
    for case in (project_case, spectral_case, input_case):
      worst = max(worst, case(*shape)['worst'])
  assert worst < EXACT_LIMIT
  return worst
