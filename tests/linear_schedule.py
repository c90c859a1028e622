"""The host rules of the two hand-written Linear kernels, restated in plain Python (a helper module
for tests/test_linear_schedule_cpu.py and tests/test_gpu_linear_edges.py, not a test).

`f32_plan` follows csrc/f32_linear.hip: `f32_linear_sk_per` (stream-K or one workgroup per tile),
the kernel's segment computation and the XCD-block search of `lnz_f32_linear`.  `f16x3_plan` follows
csrc/f16x3_linear.hip: `lnz_f16x3_linear_splits`, the kernel's K range per split and the launcher's
choice of the slice-pipelined kernel.  The shape tables below name the seam each shape was chosen
for; the CPU test asserts that the plans have those properties and agree with the library's host
entry points, so that a change of a launch rule that moves a shape off its seam fails there."""
import collections

import numpy as np

BM = BN = 128
F32_BK = 32          # floats per k-slice of f32_linear
F16_BK = 64          # halves per k-slice of f16x3_linear
F16_PIPE_MIN_SLICES = 16
CUS = 256

F32Plan = collections.namedtuple('F32Plan', 'tiles_m tiles_n tiles Tall per grid bh segments')
F16Plan = collections.namedtuple('F16Plan', 'tiles Tall nsplit slices pipe')


def _cdiv(a, b):
  return (a + b - 1) // b


def f32_sk_per(M, N, K):
  """(per, grid) of f32_linear_sk_per: per = 0 for one workgroup per tile."""
  tiles = _cdiv(M, BM) * _cdiv(N, BN)
  Tall = K // F32_BK
  if tiles >= 128 or Tall < 16:
    return 0, tiles
  U = tiles * Tall
  per = max(_cdiv(U, 256), 8)
  if per >= Tall:
    return 0, tiles
  return per, _cdiv(U, per)


def _xcd_block_height(tiles_m, tiles_n):
  """the `bh` search of lnz_f32_linear / lnz_f16x3_linear (0: plain row-major order)"""
  grid = tiles_m * tiles_n
  bh = 0
  if grid % 8 == 0:
    per = grid // 8
    h = 1
    while h <= tiles_m and h * h <= per:
      if tiles_m % h == 0 and per % h == 0 and tiles_n % (per // h) == 0 and \
          (tiles_m // h) * (tiles_n // (per // h)) == 8:
        bh = h
      h += 1
  return bh


def f32_plan(M, N, K, workspace=True):
  """The launch of lnz_f32_linear(M, N, K) with a stream-K workspace (ops.f32_linear always gives
  one): `segments[wg]` = the (tile, first slice, slice count) runs of workgroup wg in the order the
  kernel executes them."""
  assert M > 0 and N > 0 and K >= F32_BK and K % F32_BK == 0
  tiles_m, tiles_n = _cdiv(M, BM), _cdiv(N, BN)
  tiles, Tall = tiles_m * tiles_n, K // F32_BK
  per, grid = f32_sk_per(M, N, K) if workspace else (0, tiles)
  segments, bh = [], 0
  if per > 0:
    U = tiles * Tall
    for wg in range(grid):
      u0 = wg * per
      u1 = min(u0 + per, U)
      t0, t1 = u0 // Tall, (u1 - 1) // Tall
      if t0 == t1:
        segments.append([(t0, u0 - t0 * Tall, u1 - u0)])
      else:   # the head of the later tile first, then the tail this workgroup owns
        segments.append([(t1, 0, u1 - t1 * Tall), (t0, u0 - t0 * Tall, t1 * Tall - u0)])
  else:
    bh = _xcd_block_height(tiles_m, tiles_n)
    for wg in range(grid):
      xcd, slot = wg & 7, wg >> 3
      if bh > 0:
        bw = (grid >> 3) // bh
        bpr = tiles_n // bw
        tm, tn = (xcd // bpr) * bh + slot % bh, (xcd % bpr) * bw + slot // bh
      else:
        tm, tn = wg // tiles_n, wg % tiles_n
      segments.append([(tm * tiles_n + tn, 0, Tall)])
  return F32Plan(tiles_m, tiles_n, tiles, Tall, per, grid, bh, segments)


def f32_splits(plan):
  """lnz_f32_linear_splits: the number of stream-K workgroups, 1 without stream-K"""
  return plan.grid if plan.per > 0 else 1


def f32_workspace_floats(plan):
  """lnz_f32_linear_workspace_floats: one partial tile per workgroup + one counter per tile"""
  return plan.grid * BM * BN + plan.tiles if plan.per > 0 else 0


def f32_two_segment_workgroups(plan):
  return sum(len(s) == 2 for s in plan.segments)


def f32_shortest_segment(plan):
  return min(T for s in plan.segments for _, _, T in s)


def f32_odd_segments(plan):
  return sum(T % 2 for s in plan.segments for _, _, T in s)


def f32_owner(plan, tile):
  """the workgroup holding the tile's last slice"""
  return next(wg for wg, s in enumerate(plan.segments) for t, k0, T in s if t == tile and k0 + T == plan.Tall)


def f32_contributors(plan, tile):
  """the workgroups that hand a partial of `tile` to its owner, ascending"""
  return [wg for wg, s in enumerate(plan.segments) for t, k0, T in s if t == tile and k0 + T < plan.Tall]


def f32_max_contributors(plan):
  return max(len(f32_contributors(plan, t)) for t in range(plan.tiles))


def f32_short_last_run(plan):
  return plan.per > 0 and (plan.tiles * plan.Tall) % plan.per != 0


def f16x3_plan(M, N, K, workspace=True):
  """The launch of lnz_f16x3_linear(M, N, K): with `partials` (ops.f16x3_linear gives them whenever
  lnz_f16x3_linear_splits > 1) or without (the raw entry point with partials = NULL: no split)."""
  assert M > 0 and N > 0 and K >= F16_BK and K % F16_BK == 0
  tiles, Tall = _cdiv(M, BM) * _cdiv(N, BN), K // F16_BK
  ns = 1
  if workspace:
    if tiles < 128:
      ns = 256 // tiles
    ns = max(min(ns, Tall // 8, 8), 1)
  slices = [(s + 1) * Tall // ns - s * Tall // ns for s in range(ns)]
  return F16Plan(tiles, Tall, ns, slices, Tall // ns >= F16_PIPE_MIN_SLICES)


# ---------------------------------------------------------------------------- the shapes (M, N, K)
# what the suite ran before (tests/test_gpu_ada.py)
F32_EXISTING = [(128, 128, 64), (1024, 256, 832), (300, 1056, 4096), (77, 200, 192), (1024, 4096, 4096),
                (1, 5, 32)]
F16_EXISTING = [(128, 128, 64), (1024, 256, 832), (300, 1056, 4096), (77, 200, 192), (1024, 4096, 4096)]

# the seams of f32_linear: the properties are asserted by test_linear_schedule_cpu.py
F32_CASES = [
    (100, 100, 512),    # smallest stream-K launch: 1 tile, 2 workgroups, one contributor
    (100, 100, 544),    # 3 workgroups: a one-slice owner, a middle workgroup neither head nor tail
    (130, 100, 640),    # 2 tiles, 5 workgroups, one two-segment workgroup (tail 4 + head 4)
    (129, 129, 544),    # 4 tiles, one real row / column in the ragged ones, odd N, short last run
    (140, 1, 4064),     # N = 1, 16 contributors to a tile, a one-slice segment
    (128, 128, 8192),   # 1 tile, 32 workgroups: 31 partials added by one owner
    (300, 1056, 4064),  # per = 14, odd Tall: 27 odd segments, 25 two-segment workgroups
    (1024, 1920, 544),  # 120 tiles, 255 workgroups, 105 two-segment workgroups
    (256, 512, 64),     # one workgroup per tile, XCD blocks of height 1
    (512, 1024, 64),    # one workgroup per tile, XCD blocks of height 2
]
F32_STREAMK_CASES = F32_CASES[:8]
F32_GUARD_CASES = [(129, 129, 544), (130, 100, 640), (256, 512, 64)]
F32_SHARED_WORKSPACE = [(130, 100, 640), (130, 100, 576)]   # two layouts of one workspace size

# the seams of f16x3_linear: (M, N, K, raw); raw = the C entry point with partials = NULL
F16_CASES = [
    (5, 5, 1088, True),        # pipelined kernel, T = 17 (odd), one tile
    (5, 5, 1088, False),       # plain kernel, 2 splits of 8 and 9 slices
    (5, 5, 1600, False),       # plain kernel, 3 splits of 8, 8, 9
    (130, 5, 1216, False),     # 2 tiles, 2 splits of 9 and 10, ragged M across a tile boundary
    (1000, 1400, 2112, False),  # 88 tiles, 2 splits of 16 and 17: pipelined under split-K
    (640, 1500, 4160, False),  # 60 tiles, 4 splits of 16, 16, 16, 17, pipelined
]


# ------------------------------------------------------------------------------- exact operands
def _integers(rs, shape):
  return rs.randint(-8, 9, size=shape).astype(np.float64)


def _scaled_slices(x):
  """32-column slice s times 1 + s % 3, clipped to [-8, 8]: a swapped or repeated slice cannot cancel"""
  s = np.arange(x.shape[1]) // 32
  return np.clip(x * (1 + s % 3), -8, 8)


def f32_exact_operands(M, N, K):
  """float64 x [M, K], w [N, K], bias [N] of integers in [-8, 8]: every partial sum of x w^T + bias
  is an integer below 64 K + 8 <= 2^19 + 8 at K <= 8192 — exact in fp32 in every summation order."""
  assert K <= 8192
  rs = np.random.RandomState(M + 3 * N + 7 * K)
  return _scaled_slices(_integers(rs, (M, K))), _integers(rs, (N, K)), _integers(rs, (N,))


def f16x3_exact_operands(M, N, K):
  """float64 x, bias of integers in [-8, 8] and W = q / 64, q integer in [-8, 8]: x and 1024 W = 16 q
  are exact in fp16 with zero low planes, the accumulated sums integers below 8 * 128 * K < 2^23
  at K <= 4160, and 2^-10 sum + bias a multiple of 1 / 64 below 2^13: exact in fp32."""
  assert K <= 4160
  rs = np.random.RandomState(5 * M + 3 * N + K)
  return _scaled_slices(_integers(rs, (M, K))), _integers(rs, (N, K)) / 64.0, _integers(rs, (N,))
