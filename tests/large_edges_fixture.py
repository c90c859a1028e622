"""Planted inputs of tests/test_gpu_large_edges.py (and its worker, and the CPU check of their
preconditions in tests/test_large_edges_cpu.py): numpy only.

EXACT cases: every operand is a small integer that survives every rounding on its way through the
large-graph kernels (bf16 / fp16 pieces, the 2^10 A-operand scale of the two-plane mode), so every
product and every partial sum is an integer below 2^24 and an fp32 result must EQUAL the float64
one whatever the summation order — a dropped, repeated or misplaced block changes an integer.  Each
builder asserts that precondition on its own inputs in float64 (`_check_below`): the bound is the
sum of the ABSOLUTE products of a dot product, which covers every partial sum in every order."""
import functools

import numpy as np

EXACT_LIMIT = 2.0 ** 24
F16_A_SCALE = 1024.0   # csrc/conv_large.hip ElemTraits<2>::kAScale: the two-plane mode's A operands

# ---- the streamed layer: (C, N, B, also run real-valued); total = C * ceil(N / 64) + 1 blocks ----
CONV_SHAPES = [
    (0, 130, 10, False),   # total  1: the lift alone (the sparse layers' launch)
    (2, 64, 10, False),    # total  3: shorter than the prologue, tail of 3, nkb = 1 wrap
    (2, 160, 10, True),    # total  7: = 3 mod 4
    (2, 300, 10, True),    # total 11: = 3 mod 4, two row tiles, waves past the last row group
    (3, 129, 10, False),   # total 10: = 2 mod 4, first N beyond the mid route
    (1, 257, 10, True),    # total  6: the second tile holds ONE row
    (4, 256, 10, False),   # total 17: = 1 mod 4, N exactly one tile, Nk == N
    (8, 130, 10, False),   # total 25: the channel limit
    (1, 192, 10, False),   # total  4: = 0 mod 4, Nk == N
]
CONV_DIN, CONV_S, CONV_K = 10, 2, 40


def conv_total(C, N):
  return C * ((N + 63) // 64) + 1


def is_bf16(x):
  """every entry is a bf16 number (the low 16 bits of its fp32 form are zero)"""
  x32 = np.ascontiguousarray(x, np.float32)
  return bool((x32.astype(np.float64) == np.asarray(x, np.float64)).all()
              and ((x32.view(np.uint32) & np.uint32(0xffff)) == 0).all())


def bf16_round(x):
  """round to nearest even to bf16, as float64 (numpy only; finite inputs)"""
  u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
  u = (u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xffff0000)
  return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _check_below(what, abs_sum, limit=EXACT_LIMIT):
  m = float(np.max(abs_sum)) if np.size(abs_sum) else 0.0
  assert m < limit, '%s: max |partial sum| bound %g is not below %g' % (what, m, limit)
  return m


def _ints(rs, shape, lo, hi, density=1.0):
  x = rs.randint(lo, hi + 1, size=shape).astype(np.float64)
  if density < 1.0:
    x *= rs.rand(*shape) < density
  return x


def _sparse_signs(rs, B, N, K, per_column):
  """[B,N,K] entries in {-1, 0, 1}, about `per_column` nonzeros per column"""
  return (rs.rand(B, N, K) < per_column / float(N)) * (rs.randint(0, 2, size=(B, N, K)) * 2.0 - 1.0)


def spectral_reference(X, V, G, Wlong):
  """T [B,K,128] = sum_s diag(g_s) (V^T X) W_s^T in float64; Wlong [128,S,din]"""
  Y = np.einsum('bnk,bni->bki', V, X)
  return np.einsum('bsk,bki,osi->bko', G, Y, Wlong, optimize=True), Y


def _check_spectral_exact(what, X, V, G, Wlong):
  _check_below(what + ' Y = V^T X', np.einsum('bnk,bni->bki', np.abs(V), np.abs(X)))
  Ya = np.abs(np.einsum('bnk,bni->bki', V, X))
  _check_below(what + ' T', np.einsum('bsk,bki,osi->bko', np.abs(G), Ya, np.abs(Wlong), optimize=True))


@functools.lru_cache(maxsize=None)
def conv_exact_case(C, N, B, K=CONV_K, din=CONV_DIN, S=CONV_S):
  """Integer inputs of one streamed layer and its float64 stages.  L entries, X and the node-space
  weight blocks in {-2..2}; V, G and the long-scale blocks in {-1, 0, 1}; |Z| <= 64 and T a bf16
  integer (they are rounded to one bf16 / fp16 piece between the launches); bias in {-8..8}."""
  rs = np.random.RandomState(1000 * C + N)
  L = _ints(rs, (B, N, N, max(C, 1)), -2, 2, density=12.0 / N)[..., :C]
  X = _ints(rs, (B, N, din), -2, 2)
  Wn = _ints(rs, (128, C, din), -2, 2, density=0.6)
  Wl = _ints(rs, (128, S, din), -1, 1, density=0.5)
  V = _sparse_signs(rs, B, N, K, 40)
  G = _ints(rs, (B, S, K), -1, 1)
  bias = _ints(rs, (128,), -8, 8)
  Z = np.einsum('bni,oci->bcon', X, Wn)                                # [B,C,128,N]
  T, Y = spectral_reference(X, V, G, Wl)                               # [B,K,128]
  pre = np.einsum('bnk,bko->bno', V, T) + bias
  for c in range(C):
    pre += np.matmul(L[..., c], Z[:, c].transpose(0, 2, 1))
  # ---- the precondition: nothing on the way rounds, no partial sum reaches 2^24
  what = 'conv_exact_case(C=%d, N=%d)' % (C, N)
  assert B > 8 and B % 8 != 0
  for b0, b1 in ((0, 8), (1, 9)):   # a `b % 8` graph map must not pass
    assert not np.array_equal(X[b0], X[b1]) and not np.array_equal(V[b0], V[b1])
    assert C == 0 or not np.array_equal(L[b0], L[b1])
  assert np.abs(Z).max(initial=0.0) <= 64 and is_bf16(Z) and is_bf16(T) and np.abs(T).max() > 0
  # (fp16 holds the integers up to 2048: T as it is, Z, and 1024 x the A operands L, V, W)
  assert np.abs(T).max() <= 2048 and F16_A_SCALE * 2 <= 2048
  worst = _check_below(what + ' gemm1', F16_A_SCALE * np.einsum('bni,oci->bcon', np.abs(X), np.abs(Wn)))
  _check_spectral_exact(what, X, V, G, Wl)
  absum = np.einsum('bnk,bko->bno', np.abs(V), np.abs(T)) + np.abs(bias)
  for c in range(C):
    absum += np.matmul(np.abs(L[..., c]), np.abs(Z[:, c]).transpose(0, 2, 1))
  worst = max(worst, _check_below(what + ' conv', F16_A_SCALE * absum))
  f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
  return dict(L=f32(L), X=f32(X), Wn=f32(Wn), Wl=f32(Wl), V=f32(V), G=f32(G), bias=f32(bias), Z=Z, T=T,
              pre=pre, worst=worst, K=K, din=din, S=S)


# ---- the projection / gemm1 entries: (B, N, din, ldx, K, S) --------------------------------------
SPECTRAL_SHAPES = [
    (3, 129, 1, 1, 1, 1),
    (3, 256, 16, 16, 7, 16),
    (3, 257, 17, 17, 16, 1),
    (3, 129, 127, 127, 17, 16),
    (3, 256, 128, 128, 63, 1),
    (3, 257, 128, 128, 64, 16),
    (3, 257, 10, 32, 20, 2),       # ldx > din: the fp32 sparse layer's padded input
]
# projection chunking by batch size: rows = max(128, roundup64(ceil(N / ceil(256 / B))))
CHUNK_SHAPES = [
    (256, 140, 10, 10, 20, 2),     # one chunk of 192 rows covers the graph
    (128, 300, 10, 10, 20, 2),     # two chunks of 192 rows, the last one ragged (108 rows)
]
WGS_SHAPE = (3, 300, 10, 10, 20, 2)   # LNZ_LARGE_PROJECT_WGS = 1: one chunk of 320; 4096: three of 128


def project_rows(B, N, target_wgs=256):
  """(rows per chunk, chunks) of lnz_large_spectral's projection launch (csrc/conv_large.hip)"""
  chunks = (target_wgs + B - 1) // B
  rows = max(128, ((N + chunks - 1) // chunks + 63) // 64 * 64)
  return rows, (N + rows - 1) // rows


@functools.lru_cache(maxsize=None)
def spectral_exact_case(B, N, din, ldx, K, S):
  """Integer X [B,N,ldx] (NaN in the columns >= din: the entries promise "first din columns used"),
  one node-space block Wn [128,din] in {-2..2}, V / G / long blocks in {-1, 0, 1}."""
  rs = np.random.RandomState(7 * N + din + K + S + B)
  X = _ints(rs, (B, N, din), -2, 2)
  Wn = _ints(rs, (128, din), -2, 2, density=0.6)
  Wl = _ints(rs, (128, S, din), -1, 1, density=0.5)
  V = _sparse_signs(rs, B, N, K, 40)
  G = _ints(rs, (B, S, K), -1, 1)
  Z = np.einsum('bni,oi->bno', X, Wn)                                   # [B,N,128]
  T, Y = spectral_reference(X, V, G, Wl)
  what = 'spectral_exact_case(B=%d, N=%d, din=%d, K=%d, S=%d)' % (B, N, din, K, S)
  worst = _check_below(what + ' gemm1', F16_A_SCALE * np.einsum('bni,oi->bno', np.abs(X), np.abs(Wn)))
  _check_spectral_exact(what, X, V, G, Wl)
  assert np.abs(T).max() > 0 and np.abs(T).max() < EXACT_LIMIT and np.abs(Y).max() > 0
  Xp = np.full((B, N, ldx), np.nan, np.float32)
  Xp[..., :din] = X
  f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
  return dict(X=Xp, Wn=f32(Wn), Wl=f32(Wl), V=f32(V), G=f32(G), Z=Z, T=T, worst=worst)


@functools.lru_cache(maxsize=None)
def spectral_real_case(B, N, din, ldx, K, S):
  rs = np.random.RandomState(11 * N + din + K + S)
  X = np.full((B, N, ldx), np.nan, np.float32)
  X[..., :din] = rs.randn(B, N, din)
  Wn = (rs.randn(128, din) / np.sqrt(din)).astype(np.float32)
  Wl = (rs.randn(128, S, din) / np.sqrt(S * din)).astype(np.float32)
  V = (rs.randn(B, N, K) / np.sqrt(N)).astype(np.float32)
  G = rs.randn(B, S, K).astype(np.float32)
  return dict(X=X, Wn=Wn, Wl=Wl, V=V, G=G)


# ---- the gathers: prescribed row lengths -----------------------------------------------------------
GATHER_B, GATHER_N, GATHER_CAP = 10, 133, 128
ROW_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 40, 48, 56, 57, 63, 64, 65, 72, 73, 96,
               127, 128]
# a wave's 8 rows: a 65+ row, an empty row, a 65+ row ... — the entries requested one row ahead
# cross "long -> empty" and "empty -> long"
_LONG_WAVE = [65, 0, 128, 0, 73, 0, 127, 96]
_SHORT_WAVE = [32, 0, 31, 0, 25, 0, 17, 24]
_TAIL = {128: [72, 0, 65, 33, 1], 32: [32, 0, 9, 25, 1]}   # the last tile: one wave, five rows


def gather_row_plan(cap=GATHER_CAP, B=GATHER_B, N=GATHER_N):
  """[B,N] prescribed entries per row (<= cap), another assignment of lengths to rows per graph:
  the 16 full waves of the base order are rotated by the graph index, every other graph walks its
  waves backwards; the five-row tail wave stays."""
  lengths = [n for n in ROW_LENGTHS if n <= cap]
  base = list(_LONG_WAVE if cap >= 128 else _SHORT_WAVE)
  i = 0
  while len(base) < N - N % 8:
    base.append(lengths[i % len(lengths)])
    i += 1
  waves = [base[8 * w:8 * w + 8] for w in range(N // 8)]
  plan = np.zeros((B, N), np.int64)
  for b in range(B):
    ws = waves[b % len(waves):] + waves[:b % len(waves)]
    rows = [n for w in ws for n in (w[::-1] if b & 1 else w)] + _TAIL[cap]
    plan[b] = rows
  for b in range(B):
    assert set(plan[b]) == set(lengths), 'every listed row length in every graph'
    assert b == 0 or not np.array_equal(plan[b], plan[0])
  # long -> empty -> long inside ONE wave's rows
  w0 = plan[0, :8]
  assert cap < 128 or (w0[0] > 64 and w0[1] == 0 and w0[2] > 64)
  return plan


@functools.lru_cache(maxsize=None)
def gather_case(cap=GATHER_CAP, exact=True):
  """L [B,N,N] with exactly plan[b, r] nonzeros in row r (random columns), Z [B,N,128], X0 [B,N,128]
  (the gathers accumulate in place).  exact: L in +-{1, 2}, Z and X0 integers of magnitude <= 64;
  otherwise real values (Z rounded to bf16: both gathers are handed the same numbers)."""
  B, N = GATHER_B, GATHER_N
  plan = gather_row_plan(cap)
  rs = np.random.RandomState(cap + (0 if exact else 1))
  # the `n` smallest of N random keys: n distinct random columns per row
  rank = np.argsort(np.argsort(rs.rand(B, N, N), axis=2), axis=2)
  mask = rank < plan[:, :, None]
  if exact:
    vals = rs.randint(1, 3, size=(B, N, N)) * (rs.randint(0, 2, size=(B, N, N)) * 2.0 - 1.0)
    Z = _ints(rs, (B, N, 128), -64, 64)
    X0 = _ints(rs, (B, N, 128), -64, 64)
  else:
    vals = rs.randn(B, N, N)
    vals = np.where(vals == 0.0, 1.0, vals).astype(np.float32).astype(np.float64)
    Z = bf16_round(rs.randn(B, N, 128))
    X0 = rs.randn(B, N, 128).astype(np.float32).astype(np.float64)
  L = mask * vals
  assert np.array_equal((L != 0).sum(axis=2), plan)
  absum = np.abs(X0) + np.matmul(np.abs(L), np.abs(Z))
  if exact:
    assert is_bf16(L) and is_bf16(Z)
    _check_below('gather_case(cap=%d)' % cap, absum)
  return dict(L=L.astype(np.float32), Z=Z.astype(np.float32), X0=X0.astype(np.float32), plan=plan)


@functools.lru_cache(maxsize=None)
def gather_channels_case(cap, R):
  """R operators from gather_case(cap, exact=False): channel c of L [B,N,N,R] is the case's L with the
  graphs rotated by c, L[(b + c) % B] — every graph walks its waves in another order, so the R rows of a
  (row, channel) group have other lengths —; Z [R,B,N,128]: R different blocks (the case's Z, its nodes
  rotated by 3 c, the sign flipped for odd c: still bf16 numbers); plan [R,B,N]; X0 as the case's."""
  case = gather_case(cap, False)
  B = GATHER_B
  assert 2 <= R <= 8 and R < B
  rot = [[(b + c) % B for b in range(B)] for c in range(R)]
  L = np.stack([case['L'][rot[c]] for c in range(R)], axis=3)
  plan = np.stack([case['plan'][rot[c]] for c in range(R)], axis=0)
  Z = np.stack([np.roll(case['Z'], 3 * c, axis=1) * (-1.0 if c & 1 else 1.0) for c in range(R)], axis=0)
  # the preconditions: no row beyond cap (the images raise no flag), the plan is the rotated plan, no two
  # channels of a graph share their lengths or their features
  assert plan.max() == cap and np.array_equal((L != 0).sum(axis=2).transpose(2, 0, 1), plan)
  for c in range(1, R):
    for d in range(c):
      assert not np.array_equal(Z[c], Z[d])
      assert all(not np.array_equal(plan[c, b], plan[d, b]) for b in range(B))
  assert is_bf16(Z)
  return dict(L=np.ascontiguousarray(L, np.float32), Z=np.ascontiguousarray(Z, np.float32), X0=case['X0'], plan=plan)


def gather_reference(L64, Z64, X064, relu):
  """(float64 result, per-element bound 2 (n + 1) 2^-24 (|x0| + sum |v z|)): a chain of n fp32 FMAs,
  the standard running-error bound, doubled"""
  ref = X064 + np.matmul(L64, Z64)
  n = (L64 != 0).sum(axis=2)[:, :, None]
  bound = 2.0 * (n + 1) * 2.0 ** -24 * (np.abs(X064) + np.matmul(np.abs(L64), np.abs(Z64)))
  return (np.maximum(ref, 0.0) if relu else ref), bound


def all_exact_cases():
  """build every exact case (each asserts its own precondition) -> the worst bound met"""
  worst = 0.0
  for C, N, B, _ in CONV_SHAPES:
    worst = max(worst, conv_exact_case(C, N, B)['worst'])
  for shape in SPECTRAL_SHAPES + CHUNK_SHAPES + [WGS_SHAPE]:
    worst = max(worst, spectral_exact_case(*shape)['worst'])
  for cap in (128, 32):
    gather_case(cap, True)
  return worst


# ---- lnz_large_conv on given operand images (the wave-count switch): real values ------------------
WAVES_SHAPES = [(2, 300, 10), (1, 257, 10)]   # (C, N, B), planes = 1


@functools.lru_cache(maxsize=None)
def conv_real_case(C, N, B, K=CONV_K):
  """L [B,N,N,C], V [B,N,K] fp32 and the B images the launch is HANDED: Zt [B,C,128,N], Tt [B,128,K]
  bf16 numbers — no projection atomics in front of it, so two runs give the same bits.  `ref`: the
  float64 result on the bf16-rounded operators (what planes = 1 packs)."""
  rs = np.random.RandomState(31 * C + N)
  L = (rs.randn(B, N, N, C) * (rs.rand(B, N, N, C) < 0.1)).astype(np.float32)
  V = (rs.randn(B, N, K) / np.sqrt(N)).astype(np.float32)
  Zt = bf16_round(rs.randn(B, C, 128, N))
  Tt = bf16_round(rs.randn(B, 128, K))
  bias = rs.randn(128).astype(np.float32)
  ref = np.matmul(bf16_round(V), Tt.transpose(0, 2, 1)) + bias
  for c in range(C):
    ref += np.matmul(bf16_round(L[..., c]), Zt[:, c].transpose(0, 2, 1))
  return dict(L=L, V=V, Zt=Zt.astype(np.float32), Tt=Tt.astype(np.float32), bias=bias,
              ref=np.maximum(ref, 0.0))
