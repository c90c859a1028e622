"""CPU-only: tests/linear_schedule.py restates the launch rules of lnz_f32_linear and
lnz_f16x3_linear.  Here the restatement is held to the library's own host entry points, every shape
of tests/test_gpu_linear_edges.py is shown to sit on the seam it was chosen for (so that a later
change of a launch rule cannot quietly make the GPU test vacuous), the stream-K plans are checked
for the properties the kernel's forward-progress argument rests on, and the "exact data" claim of
the GPU test — fp32 arithmetic on these operands has no rounding — is checked against float64."""
import numpy as np
import pytest
import torch

import linear_schedule as S


@pytest.fixture(scope='module')
def lib():
  from lanczosnet_amd import _lib
  return _lib.load()


F32_ALL = S.F32_CASES + S.F32_EXISTING + S.F32_SHARED_WORKSPACE[1:]
F16_ALL = sorted(set(c[:3] for c in S.F16_CASES)) + S.F16_EXISTING


def test_restatement_agrees_with_the_library_host_rules(lib):
  for M, N, K in F32_ALL:
    p = S.f32_plan(M, N, K)
    assert lib.lnz_f32_linear_splits(M, N, K) == S.f32_splits(p), (M, N, K)
    assert lib.lnz_f32_linear_workspace_floats(M, N, K) == S.f32_workspace_floats(p), (M, N, K)
  for M, N, K in F16_ALL:
    assert lib.lnz_f16x3_linear_splits(M, N, K) == S.f16x3_plan(M, N, K).nsplit, (M, N, K)
  # ... and on a sweep around the thresholds of both rules (tiles 128, 16 slices, the floor of 8)
  for M in (1, 128, 129, 1000, 1024, 2000):
    for N in (1, 128, 129, 1056, 1920, 2048, 4096):
      for K in (64, 448, 512, 576, 1024, 1088, 4032, 4096, 8192):
        p = S.f32_plan(M, N, K)
        assert lib.lnz_f32_linear_splits(M, N, K) == S.f32_splits(p), (M, N, K)
        assert lib.lnz_f32_linear_workspace_floats(M, N, K) == S.f32_workspace_floats(p), (M, N, K)
        assert lib.lnz_f16x3_linear_splits(M, N, K) == S.f16x3_plan(M, N, K).nsplit, (M, N, K)


def _props(M, N, K):
  p = S.f32_plan(M, N, K)
  return dict(tiles=p.tiles, Tall=p.Tall, per=p.per, grid=p.grid, bh=p.bh,
              two=S.f32_two_segment_workgroups(p), shortest=S.f32_shortest_segment(p),
              odd=S.f32_odd_segments(p), contributors=S.f32_max_contributors(p),
              short_last=S.f32_short_last_run(p))


def test_the_existing_f32_shapes_reach_what_the_table_says():
  """the shapes of test_f32_linear_kernel_matches_float64: no odd segment, nothing below two slices"""
  for c in [(128, 128, 64), (77, 200, 192), (1, 5, 32)]:
    assert _props(*c)['per'] == 0 and _props(*c)['bh'] == 0
  assert _props(1024, 4096, 4096)['per'] == 0 and _props(1024, 4096, 4096)['bh'] == 4
  a, b = _props(1024, 256, 832), _props(300, 1056, 4096)
  assert (a['per'], a['grid'], a['shortest'], a['odd']) == (8, 52, 2, 0)
  assert (b['per'], b['grid'], b['shortest'], b['odd']) == (14, 247, 2, 0)
  assert max(a['contributors'], b['contributors']) == 9


def test_the_f32_shapes_sit_on_their_seams():
  """DESIGN.md §4, "The Linear kernels at their schedule seams": the table, asserted"""
  assert S.F32_CASES == [(100, 100, 512), (100, 100, 544), (130, 100, 640), (129, 129, 544), (140, 1, 4064),
                         (128, 128, 8192), (300, 1056, 4064), (1024, 1920, 544), (256, 512, 64),
                         (512, 1024, 64)]
  assert S.F32_STREAMK_CASES == S.F32_CASES[:8]
  for c in S.F32_STREAMK_CASES:
    assert _props(*c)['per'] > 0, c
  # the smallest stream-K launch: two workgroups on one tile, one contributor, no second segment
  p = _props(100, 100, 512)
  assert (p['tiles'], p['Tall'], p['per'], p['grid'], p['two'], p['contributors']) == (1, 16, 8, 2, 0, 1)
  # an owner of ONE slice, and a middle workgroup that holds neither the head nor the tail
  assert S.f32_plan(100, 100, 544).segments == [[(0, 0, 8)], [(0, 8, 8)], [(0, 16, 1)]]
  # one two-segment workgroup: head 4 of tile 1 first, then the tail 4 of tile 0; 3 workgroups a tile
  pl = S.f32_plan(130, 100, 640)
  assert (pl.tiles, pl.Tall, pl.grid) == (2, 20, 5) and pl.segments[2] == [(1, 0, 4), (0, 16, 4)]
  assert [len(S.f32_contributors(pl, t)) + 1 for t in range(2)] == [3, 3]
  # ragged tiles of one real row / column, odd N (scalar stores), one-slice segments, short last run
  p = _props(129, 129, 544)
  assert (p['tiles'], p['two'], p['shortest'], p['odd'], p['short_last']) == (4, 3, 1, 4, True)
  assert S.f32_plan(129, 129, 544).segments[-1] == [(3, 13, 4)] and 129 % 128 == 1 and 129 % 4 != 0
  # N = 1, two tiles along M, odd Tall, 16 partials for one owner, a one-slice segment
  p = _props(140, 1, 4064)
  assert (p['tiles'], p['Tall'], p['contributors'], p['shortest']) == (2, 127, 16, 1)
  # 31 partials added by one owner
  p = _props(128, 128, 8192)
  assert (p['tiles'], p['grid'], p['contributors']) == (1, 32, 31)
  # per above its floor with an odd slice count
  p = _props(300, 1056, 4064)
  assert (p['per'], p['Tall'], p['odd'], p['two'], p['shortest'], p['short_last']) == (14, 127, 27, 25, 1, True)
  # the whole chip: every tile boundary crossed inside a workgroup or between two
  p = _props(1024, 1920, 544)
  assert (p['tiles'], p['grid'], p['two']) == (120, 255, 105)
  # one workgroup per tile in XCD-block order, block heights 1 and 2
  assert (_props(256, 512, 64)['per'], _props(256, 512, 64)['bh'], _props(256, 512, 64)['grid']) == (0, 1, 8)
  assert (_props(512, 1024, 64)['per'], _props(512, 1024, 64)['bh'], _props(512, 1024, 64)['grid']) == (0, 2, 32)
  # the guard-band cases are cases, and cover stream-K with odd N, stream-K with N % 4 == 0, one per tile
  assert set(S.F32_GUARD_CASES) <= set(S.F32_CASES)
  assert [_props(*c)['per'] > 0 for c in S.F32_GUARD_CASES] == [True, True, False]
  # two layouts of one workspace size: what ops._f32_linear_workspace hands from one to the other
  a, b = (S.f32_plan(*c) for c in S.F32_SHARED_WORKSPACE)
  assert S.f32_workspace_floats(a) == S.f32_workspace_floats(b) == 81922
  assert a.segments != b.segments and (a.tiles, a.grid) == (b.tiles, b.grid)


def test_the_f16x3_shapes_sit_on_their_seams():
  want = {(5, 5, 1088, True): (1, [17], True), (5, 5, 1088, False): (1, [8, 9], False),
          (5, 5, 1600, False): (1, [8, 8, 9], False), (130, 5, 1216, False): (2, [9, 10], False),
          (1000, 1400, 2112, False): (88, [16, 17], True),
          (640, 1500, 4160, False): (60, [16, 16, 16, 17], True)}
  assert set(want) == set(S.F16_CASES)
  for (M, N, K, raw), (tiles, slices, pipe) in want.items():
    p = S.f16x3_plan(M, N, K, workspace=not raw)
    assert (p.tiles, p.slices, p.pipe) == (tiles, slices, pipe), (M, N, K, raw)
    assert sum(p.slices) == p.Tall and len(p.slices) == p.nsplit
  # what the existing shapes reach: the plain kernel unsplit or evenly split, the pipelined one at even T
  got = [S.f16x3_plan(*c) for c in S.F16_EXISTING]
  assert [(p.slices, p.pipe) for p in got] == [([1], False), ([13], False), ([8] * 8, False), ([3], False),
                                               ([64], True)]


@pytest.mark.parametrize('M,N,K', F32_ALL)
def test_every_f32_plan_is_a_partition_with_forward_progress(M, N, K):
  p = S.f32_plan(M, N, K)
  assert p.grid == len(p.segments) <= S.CUS
  cover = np.zeros((p.tiles, p.Tall), np.int64)
  for segs in p.segments:
    assert 1 <= len(segs) <= 2
    for tile, k0, T in segs:
      assert T >= 1 and k0 >= 0 and k0 + T <= p.Tall
      cover[tile, k0:k0 + T] += 1
    if len(segs) == 2:   # the head of the later tile runs first, the tail it owns last
      (t1, k1, T1), (t0, k0, T0) = segs
      assert t1 == t0 + 1 and k1 == 0 and T1 < p.Tall and k0 + T0 == p.Tall
  assert (cover == 1).all()
  for tile in range(p.tiles):
    own, con = S.f32_owner(p, tile), S.f32_contributors(p, tile)
    # a contributor sits in a lower-numbered workgroup and hands its partial over in its FIRST
    # segment: no owner waits for work queued behind another wait
    assert all(wg < own for wg in con) and con == list(range(own - len(con), own))
    for wg in con:
      assert p.segments[wg][0][0] == tile
    if p.per > 0:   # the kernel's gA, gB
      assert own == ((tile + 1) * p.Tall - 1) // p.per and own - len(con) == tile * p.Tall // p.per
    else:
      assert not con


def _exact_cases():
  for c in S.F32_CASES + S.F32_SHARED_WORKSPACE[1:]:
    yield ('f32',) + c
  for c in sorted(set(c[:3] for c in S.F16_CASES)):
    yield ('f16x3',) + c


@pytest.mark.parametrize('kind,M,N,K', list(_exact_cases()))
def test_fp32_arithmetic_is_exact_on_the_integer_operands(kind, M, N, K):
  """torch.nn.functional.linear in fp32 equals the float64 product on the operands of every exact
  case: the GPU test may then demand torch.equal."""
  x, w, b = (S.f32_exact_operands if kind == 'f32' else S.f16x3_exact_operands)(M, N, K)
  x, w, b = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)
  for t in (x, w, b):
    assert torch.equal(t.float().double(), t)
  ref = torch.nn.functional.linear(x, w, b)
  assert torch.equal(torch.nn.functional.linear(x.float(), w.float(), b.float()).double(), ref)
  assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) < 2.0 ** 19 + 9
  # the 32-column slices of x carry different scales
  s = x.abs().reshape(M, K // 32, 32).amax(dim=(0, 2))
  assert float(s.max()) == 8.0 and float(x.abs().max()) <= 8.0
  if kind == 'f16x3':   # both operands of the split product are single fp16 planes
    for t in (x, 1024.0 * w):
      assert torch.equal(t.half().double(), t)
    assert float((1024.0 * w).abs().max()) <= 128.0
    v = ref.float()
    hi = v.half()
    assert torch.isfinite(hi).all() and torch.isfinite((v - hi.float()).half()).all()
