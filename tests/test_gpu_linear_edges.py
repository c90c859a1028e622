"""lnz_f32_linear and lnz_f16x3_linear at the seams of their host-side schedules (DESIGN.md §4,
"The Linear kernels at their schedule seams"): a stream-K segment of one slice, odd segments in a
loop unrolled by two, a run that ends inside a tile, a shorter last run, 31 partials for one owner,
the scalar-store epilogue, XCD-block order at small grids; the slice-pipelined f16x3 kernel at an odd
slice count and under an uneven split-K.  tests/linear_schedule.py restates the launch rules and
tests/test_linear_schedule_cpu.py asserts that every shape below has the property it is here for.

Every case runs on integer operands for which fp32 arithmetic is EXACT (checked on the CPU in
test_linear_schedule_cpu.py), so the comparison with float64 is torch.equal: a dropped, repeated or
swapped k-slice cannot hide inside a tolerance.  Each case also runs once on the random operands of
tests/test_gpu_ada.py against the bars used there, which keeps the low fp16 planes under test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import linear_schedule as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = -12345.5   # no result of the integer data ends in .5


def _t(x, dtype=torch.float32):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)


def _ref(x, w, b, relu):
  """the float64 reference: torch.nn.functional.linear on doubles"""
  r = torch.nn.functional.linear(x.double(), w.double(), None if b is None else b.double())
  return torch.relu(r) if relu else r


@functools.lru_cache(maxsize=None)
def _f32_exact(M, N, K):
  return tuple(_t(a) for a in S.f32_exact_operands(M, N, K))


@functools.lru_cache(maxsize=None)
def _f16x3_exact(M, N, K):
  return tuple(_t(a) for a in S.f16x3_exact_operands(M, N, K))


def _random(M, N, K):
  rs = np.random.RandomState(M + N + K)
  return (_t(rs.randn(M, K).astype(np.float32)), _t((rs.randn(N, K) / np.sqrt(K)).astype(np.float32)),
          _t(rs.randn(N).astype(np.float32)))


def _workspace(M, N, K):
  """the stream-K workspace ops.f32_linear used for this shape on the current stream"""
  from lanczosnet_amd import ops
  need = S.f32_workspace_floats(S.f32_plan(M, N, K))
  return ops._F32_LINEAR_WS[(torch.device(DEV).index, torch.cuda.current_stream(DEV).cuda_stream, need)]


def _assert_counters_zero(M, N, K):
  plan = S.f32_plan(M, N, K)
  if plan.per == 0:
    return
  ws = _workspace(M, N, K)
  assert ws.numel() == plan.grid * 128 * 128 + plan.tiles
  assert not ws.view(torch.int32)[-plan.tiles:].any(), 'tile counters are not zero on return'


# ------------------------------------------------------------------------------------ f32_linear
@pytest.mark.parametrize('M,N,K', S.F32_CASES)
def test_f32_linear_is_exact_on_integer_operands(M, N, K):
  """[relu](x w^T + bias) bit for bit against float64; stream-K shapes three times (bit-reproducible,
  tile counters zero on every return); then x and w with row stride K + 32 at once, no bias."""
  from lanczosnet_amd import ops
  x, w, b = _f32_exact(M, N, K)
  repeats = 3 if S.f32_plan(M, N, K).per > 0 else 1
  for relu in (False, True):
    ref = _ref(x, w, b, relu)
    first = None
    for _ in range(repeats):
      out = ops.f32_linear(x, w, b, relu=relu)
      _assert_counters_zero(M, N, K)
      if first is None:
        first = out
        bad = int((out.double() != ref).sum())
        assert bad == 0, '%d of %d elements differ from float64 (relu=%s)' % (bad, M * N, relu)
      assert torch.equal(out, first)
  # row strides > K on both operands; the columns beyond K hold what must not be read
  xs = torch.full((M, K + 32), 7.0, device=DEV)
  ws = torch.full((N, K + 32), 7.0, device=DEV)
  xs[:, :K], ws[:, :K] = x, w
  for relu in (False, True):
    out = ops.f32_linear(xs[:, :K], ws[:, :K], None, relu=relu)
    _assert_counters_zero(M, N, K)
    assert torch.equal(out.double(), _ref(x, w, None, relu)), relu


@pytest.mark.parametrize('M,N,K', S.F32_CASES)
def test_f32_linear_random_operands_meet_the_library_bar(M, N, K):
  """the bar of test_f32_linear_kernel_matches_float64: max(2 e_lib, 1e-6) of the scale"""
  from lanczosnet_amd import ops
  x, w, b = _random(M, N, K)
  ref = _ref(x, w, b, False)
  lib = torch.nn.functional.linear(x, w, b)
  scale = float(ref.abs().max())
  out = ops.f32_linear(x, w, b)
  e = float((out.double() - ref).abs().max()) / scale
  e_lib = float((lib.double() - ref).abs().max()) / scale
  print('f32_linear %s vs fp64: %.2e of the scale, library %.2e' % ((M, N, K), e, e_lib))
  assert e < max(2.0 * e_lib, 1e-6), (e, e_lib)
  _assert_counters_zero(M, N, K)


@pytest.mark.parametrize('M,N,K,pad', [c + (2,) for c in S.F32_GUARD_CASES] + [(130, 100, 640, 4)])
def test_f32_linear_writes_nothing_outside_its_output(M, N, K, pad):
  """`out` is a view inside a buffer of sentinels: `pad` columns on each side, two rows below.
  pad = 2: ldo = N + 4 and a base 8 bytes off 16-byte alignment — the scalar-store epilogue even at
  N % 4 == 0; pad = 4: aligned base, ldo % 4 == 0 — the 16-byte stores with ldo > N."""
  from lanczosnet_amd import ops
  x, w, b = _f32_exact(M, N, K)
  for relu in (False, True):
    buf = torch.full((M + 2, N + 2 * pad), SENTINEL, device=DEV)
    out = buf[:M, pad:pad + N]
    assert out.stride(0) == N + 2 * pad and out.data_ptr() % 16 == (8 if pad == 2 else 0)
    assert pad == 2 or (out.stride(0) % 4 == 0 and N % 4 == 0)
    ops.f32_linear(x, w, b, relu=relu, out=out)
    _assert_counters_zero(M, N, K)
    assert torch.equal(out.double(), _ref(x, w, b, relu))
    guard = buf.clone()
    guard[:M, pad:pad + N] = SENTINEL
    assert int((guard != SENTINEL).sum()) == 0, 'a sentinel around out[:M, :N] was overwritten'


def test_f32_linear_workspace_serves_two_layouts_of_one_size():
  """ops._f32_linear_workspace keys its buffers on their size: (130, 100, 640) and (130, 100, 576)
  share one, each finds the other's partial tiles in it and the counters zero.  A, B, A, B on one
  stream: every result exact and equal to the first of its shape."""
  from lanczosnet_amd import ops
  A, B = S.F32_SHARED_WORKSPACE
  first = {}
  for shape in (A, B, A, B):
    x, w, b = _f32_exact(*shape)
    out = ops.f32_linear(x, w, b)
    _assert_counters_zero(*shape)
    assert torch.equal(out.double(), _ref(x, w, b, False)), shape
    assert torch.equal(out, first.setdefault(shape, out)), shape
  assert _workspace(*A) is _workspace(*B)


# ---------------------------------------------------------------------------------- f16x3_linear
def _f16x3_launch(raw, xp, wp, bias, M, N, relu, out_planes=None, out_f32=None):
  """ops.f16x3_linear, or (raw) the C entry point with partials = NULL: no split-K, which at >= 16
  slices selects the slice-pipelined kernel however few the tiles"""
  from lanczosnet_amd import ops, _lib
  if not raw:
    return ops.f16x3_linear(xp, wp, bias, M, N, relu=relu, out_planes=out_planes, out_f32=out_f32)
  p_ = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
  K = xp.shape[2]
  assert xp.shape[1] % 128 == 0 and xp.shape[1] >= M and wp.shape[1] % 128 == 0 and wp.shape[1] >= N
  oh, ol = (out_planes[0], out_planes[1]) if out_planes is not None else (None, None)
  ldo = out_f32.stride(0) if out_f32 is not None else out_planes.stride(1)
  st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
  _lib.check(_lib.load().lnz_f16x3_linear(p_(xp[0]), p_(xp[1]), xp.stride(1), p_(wp[0]), p_(wp[1]),
                                          wp.stride(1), p_(bias), 1.0 / ops.F16X3_WEIGHT_SCALE, int(relu),
                                          M, N, K, p_(oh), p_(ol), p_(out_f32), ldo, None, st))
  return out_f32 if out_f32 is not None else out_planes


def _bits(h):
  return h.contiguous().view(torch.int16)


@pytest.mark.parametrize('M,N,K,raw', S.F16_CASES)
def test_f16x3_linear_is_exact_on_integer_operands(M, N, K, raw):
  """x, bias integers, W = q / 64: both operands are single fp16 planes and every sum is exact.  The
  fp32 output equals float64; the plane output is bit for bit the (hi, lo) split of the exact value,
  its padding rows and columns still zero; a second launch gives the same bits."""
  from lanczosnet_amd import ops
  X, W, b = _f16x3_exact(M, N, K)
  xp, wp = ops.f16x3_split(X), ops.f16x3_pack_weight(W)
  assert xp.shape == (2, (M + 127) // 128 * 128, K) and wp.shape == (2, (N + 127) // 128 * 128, K)
  assert torch.equal(xp[0, :M].float(), X) and torch.equal(wp[0, :N].float(), 1024.0 * W)
  assert not xp[1].any() and not wp[1].any() and not xp[:, M:].any() and not wp[:, N:].any()
  for bias, relu in ((None, False), (b, True)):
    ref = _ref(X, W, bias, relu)
    v = ref.float()
    assert torch.equal(v.double(), ref)
    outs = []
    for _ in range(2):
      out = torch.full((M, N), SENTINEL, device=DEV)
      outs.append(_f16x3_launch(raw, xp, wp, bias, M, N, relu, out_f32=out))
    bad = int((outs[0].double() != ref).sum())
    assert bad == 0, '%d of %d fp32 outputs differ from float64 (relu=%s)' % (bad, M * N, relu)
    assert torch.equal(outs[0], outs[1])
    hi = v.half()
    lo = (v - hi.float()).half()
    planes = []
    for _ in range(2):
      hp = torch.zeros((2, xp.shape[1], (N + 63) // 64 * 64), dtype=torch.float16, device=DEV)
      planes.append(_f16x3_launch(raw, xp, wp, bias, M, N, relu, out_planes=hp))
    hp = planes[0]
    assert torch.equal(_bits(hp[0, :M, :N]), _bits(hi)), 'hi plane != half(v)'
    assert torch.equal(_bits(hp[1, :M, :N]), _bits(lo)), 'lo plane != half(v - hi)'
    assert not hp[:, M:].any() and not hp[:, :, N:].any()
    assert torch.equal(_bits(planes[0]), _bits(planes[1]))


@pytest.mark.parametrize('M,N,K,raw', S.F16_CASES)
def test_f16x3_linear_random_operands_meet_the_split_precision_bar(M, N, K, raw):
  """the bar of test_f16x3_linear_kernel_matches_float64: 2e-6 of the scale, fp32 and plane output"""
  from lanczosnet_amd import ops
  X, W, b = _random(M, N, K)
  xp, wp = ops.f16x3_split(X), ops.f16x3_pack_weight(W)
  ref = _ref(X, W, b, False)
  scale = float(ref.abs().max())
  out = _f16x3_launch(raw, xp, wp, b, M, N, False, out_f32=torch.empty((M, N), device=DEV))
  e = float((out.double() - ref).abs().max()) / scale
  e_lib = float((torch.nn.functional.linear(X, W, b).double() - ref).abs().max()) / scale
  hp = torch.zeros((2, xp.shape[1], (N + 63) // 64 * 64), dtype=torch.float16, device=DEV)
  _f16x3_launch(raw, xp, wp, b, M, N, True, out_planes=hp)
  h = torch.relu(ref)
  e_planes = float((hp[0, :M, :N].double() + hp[1, :M, :N].double() - h).abs().max()) / float(h.abs().max())
  print('f16x3_linear %s%s vs fp64: fp32 output %.2e, planes %.2e of the scale, library fp32 %.2e'
        % ((M, N, K), ' raw' if raw else '', e, e_planes, e_lib))
  assert e < 2e-6 and e_planes < 2e-6, (e, e_planes)
  assert not hp[:, M:].any() and not hp[:, :, N:].any()
