"""The large-graph layer kernels (csrc/conv_large.hip, csrc/conv_sparse.hip; graphs beyond 128
nodes) against float64 at every kernel seam: the k pipeline's tails and short totals, the second
dealing round and the k rotation, row tiles of one row, eight channels, the 4-wave instantiation,
both row-chunk regimes of the projection, every input / eigen-space width, and in the two gathers
every turn size, rows of more than 64 entries and the entries requested one row ahead.

Two kinds of reference (tests/large_edges_fixture.py):
  EXACT — small-integer operands that survive every rounding on the way, every partial sum below
  2^24 (asserted in float64 by the fixture, on a CPU too: tests/test_large_edges_cpu.py): the fp32
  result EQUALS the float64 one in any summation order, for one, two and three planes;
  REAL — the bars of test_gpu_large.py::test_large_conv_stages_match_numpy for the streamed stages;
  for the gathers, a chain of n fp32 FMAs: |out - ref| <= 2 (n + 1) 2^-24 (|x0| + sum |v z|) per
  element (the running-error bound, doubled).  The worst achieved / allowed ratio is printed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import large_edges_fixture as fx
from lanczosnet_amd import ops
from large_edges_worker import (conv_waves_outputs, pack_weights, run_layer,
                                run_projection, to_dev)
from test_gpu_large import _bf16_round, _pieces_sum, _untile

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
  return to_dev(a, DEV)


def _act(x, relu):
  return np.maximum(x, 0.0) if relu else x


# ------------------------------------------------------------------ 1. lnz_large_conv, the layer
@pytest.mark.parametrize('C,N,B', [s[:3] for s in fx.CONV_SHAPES])
def test_streamed_layer_is_exact_on_integer_operands(C, N, B):
  """gemm1 + projection + conv (C = 0: the lift-only launch) at every `total mod 4`, totals 1 / 3,
  B = 10 (second dealing round, dead workgroups, every k rotation), N = 256 / 257, C = 8: the
  images Zt / Tt and the output EQUAL float64, for every plane count, with and without ReLU, into a
  fresh tensor and into a caller's buffer."""
  case = fx.conv_exact_case(C, N, B)
  K = case['K']
  for planes in (1, 2, 3):
    for relu in (0, 1):
      buf = torch.full((B, N, 128), float('nan'), device=DEV) if relu else None
      out, Zt, Tt, Ybuf = run_layer(case, planes, relu, DEV, out=buf)
      assert buf is None or out.data_ptr() == buf.data_ptr()
      assert (Ybuf == 0).all()
      if C:
        Zg = _pieces_sum(Zt)
        assert (Zg[..., N:] == 0).all()
        np.testing.assert_array_equal(Zg[..., :N], case['Z'])
      Tg = _pieces_sum(Tt).transpose(0, 2, 1)
      assert (Tg[:, K:] == 0).all()
      np.testing.assert_array_equal(Tg[:, :K], case['T'])
      np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), _act(case['pre'], relu))


def test_lnz_large_conv_alone_is_exact_with_planted_images():
  """ops.large_conv on HANDED integer images (|Z| <= 64 drawn directly, not a product): C = 2,
  N = 300, B = 10 — graphs 8 and 9 are other graphs than 0 and 1."""
  C, N, B, K = 2, 300, 10, fx.CONV_K
  case = fx.conv_exact_case(C, N, B)
  rs = np.random.RandomState(5)
  Z = rs.randint(-64, 65, size=(B, C, 128, N)).astype(np.float64)
  T = rs.randint(-16, 17, size=(B, 128, K)).astype(np.float64)
  L64, V64 = case['L'].astype(np.float64), case['V'].astype(np.float64)
  ref = np.matmul(V64, T.transpose(0, 2, 1)) + case['bias']
  absum = np.matmul(np.abs(V64), np.abs(T).transpose(0, 2, 1)) + np.abs(case['bias'])
  for c in range(C):
    ref += np.matmul(L64[..., c], Z[:, c].transpose(0, 2, 1))
    absum += np.matmul(np.abs(L64[..., c]), np.abs(Z[:, c]).transpose(0, 2, 1))
  assert fx.F16_A_SCALE * absum.max() < fx.EXACT_LIMIT and not np.array_equal(Z[8], Z[0])
  for planes in (1, 2, 3):
    Lb, Vb = ops_pack(case, planes)
    Zt, Tt, _ = ops.large_work_buffers(Lb)
    Zt[0, :, :, :, :N] = _dev(Z.astype(np.float32)).to(Zt.dtype)
    Tt[0, :, :, :K] = _dev(T.astype(np.float32)).to(Tt.dtype)
    for relu in (0, 1):
      out = ops.large_conv(Lb, Vb, Zt, Tt, _dev(case['bias']), relu=relu)
      np.testing.assert_array_equal(out.cpu().numpy().astype(np.float64), _act(ref, relu))


def ops_pack(case, planes):
  return ops.large_pack_operators(_dev(case['L']), _dev(case['V']), planes)


@pytest.mark.parametrize('planes', [1, 2, 3])
@pytest.mark.parametrize('C,N,B', [s[:3] for s in fx.CONV_SHAPES if s[3]])
def test_streamed_layer_real_values_within_the_stage_bars(planes, C, N, B):
  """The stage bars of test_gpu_large.py::test_large_conv_stages_match_numpy, unchanged, at B = 10
  and the totals = 3 (mod 4) / the one-row tile: Zt, Tt and the conv on the images it was handed."""
  K, din, S = 40, 10, 3
  rs = np.random.RandomState(N + planes)
  L = (rs.randn(B, N, N, C) * (rs.rand(B, N, N, C) < 0.1)).astype(np.float32)
  V = (rs.randn(B, N, K) / np.sqrt(N)).astype(np.float32)
  X = rs.randn(B, N, din).astype(np.float32)
  Wn = (rs.randn(128, C, din) / np.sqrt(C * din)).astype(np.float32)
  Wl = (rs.randn(128, S, din) / np.sqrt(C * din)).astype(np.float32)
  G = rs.randn(B, S, K).astype(np.float32)
  bias = rs.randn(128).astype(np.float32)
  case = dict(L=L, X=X, V=V, G=G, bias=bias, Wn=Wn, Wl=Wl, din=din)
  Lb, Vb = ops_pack(case, planes)
  ascale = ops.LARGE_F16_A_SCALE if planes == 2 else 1.0
  Lsum = _untile(_pieces_sum(Lb))[:, :, :N, :N] / ascale
  Vsum = _untile(_pieces_sum(Vb)[:, :, None])[:, :N] / ascale
  out, Zt, Tt, Ybuf = run_layer(case, planes, True, DEV)
  assert (Ybuf == 0).all()
  out = out.cpu().numpy().astype(np.float64)
  rnd = _bf16_round if planes == 1 else (lambda a: np.asarray(a, np.float64))
  Z = np.einsum('bni,oci->bcon', rnd(X), rnd(Wn))
  Zg = _pieces_sum(Zt)
  tol = 2e-6 if planes == 3 else 4e-6 if planes == 2 else 1e-5
  assert (Zg[..., N:] == 0).all()
  zbar = (8e-3 if planes == 1 else tol) * np.abs(Z).max()
  rz = np.abs(Zg[..., :N] - (rnd(Z) if planes == 1 else Z)).max() / zbar
  T = np.einsum('bsk,bki,osi->bko', G.astype(np.float64),
                np.einsum('bnk,bni->bki', V.astype(np.float64), X.astype(np.float64)),
                Wl.astype(np.float64), optimize=True)
  Tg = _pieces_sum(Tt).transpose(0, 2, 1)[:, :K]
  rt = np.abs(Tg - T).max() / ((8e-3 if planes == 1 else 1e-5) * np.abs(T).max())
  ref = np.matmul(Vsum, _pieces_sum(Tt).transpose(0, 2, 1)) + bias
  for c in range(C):
    ref += np.matmul(Lsum[:, c], Zg[:, c, :, :N].transpose(0, 2, 1))
  ref = np.maximum(ref, 0)
  ro = np.abs(out - ref).max() / ((2e-5 if planes == 1 else 5e-6) * np.abs(ref).max())
  print('C=%d N=%d planes=%d: achieved / bar  Zt %.3f  Tt %.3f  conv %.3f' % (C, N, planes, rz, rt, ro))
  assert rz <= 1.0 and rt <= 1.0 and ro <= 1.0


def _child(tmp_path, mode, name, env):
  """one fresh child, under its own timeout; an assertion here ends the test before the next child"""
  path = str(tmp_path / (name + '.npz'))
  base = {k: v for k, v in os.environ.items() if k not in ('LNZ_LARGE_CONV_WAVES', 'LNZ_LARGE_PROJECT_WGS')}
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'large_edges_worker.py'), mode, path],
                       cwd=ROOT, env=dict(base, **env), capture_output=True, text=True, timeout=300)
  assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
  assert 'LARGE_EDGES_OK %s' % mode in out.stdout
  return dict(np.load(path))


def test_four_wave_conv_kernel_is_exact_and_gives_the_eight_wave_bits(tmp_path):
  """LNZ_LARGE_CONV_WAVES=4 (large_conv_kernel<1,4>: 128-row tiles) in a child of its own, planes =
  1, at (C = 2, N = 300) and (C = 1, N = 257): the exact layer EQUALS float64; the real-valued conv
  on handed images is within the planes = 1 conv bar of float64 and bit for bit the default
  child's — a row's k order does not depend on the wave count."""
  default = _child(tmp_path, 'conv', 'waves8', {})
  four = _child(tmp_path, 'conv', 'waves4', {'LNZ_LARGE_CONV_WAVES': '4'})
  here = conv_waves_outputs(torch.device(DEV))
  for C, N, B in fx.WAVES_SHAPES:
    case = fx.conv_exact_case(C, N, B)
    for relu in (0, 1):
      key = 'exact_%d_%d_relu%d' % (C, N, relu)
      for got in (default[key], four[key], here[key]):
        np.testing.assert_array_equal(got.astype(np.float64), _act(case['pre'], relu))
    key = 'real_%d_%d' % (C, N)
    ref = fx.conv_real_case(C, N, B)['ref']
    ratio = np.abs(four[key].astype(np.float64) - ref).max() / (2e-5 * np.abs(ref).max())
    print('C=%d N=%d four waves: achieved / bar %.3f' % (C, N, ratio))
    assert ratio <= 1.0
    assert four[key].tobytes() == default[key].tobytes() == here[key].tobytes()


# ------------------------------------------------------------- 2. gemm1 / gemm1_rows / spectral
def _exact_T(T, planes):
  return fx.bf16_round(T) if planes == 1 else T   # (one bf16 piece rounds the exact integer once)


def _check_projection_exact(shape):
  B, N, din, ldx, K, S = shape
  case = fx.spectral_exact_case(*shape)
  for planes in (1, 2, 3):
    Tg, Ybuf, _ = run_projection(case, shape, planes, DEV, False)
    assert (Ybuf == 0).all() and (Tg[:, K:] == 0).all()
    np.testing.assert_array_equal(Tg[:, :K], _exact_T(case['T'], planes))
  Tg, Ybuf, Z = run_projection(case, shape, 1, DEV, True)
  assert (Ybuf == 0).all() and (Tg[:, K:] == 0).all()
  np.testing.assert_array_equal(Tg[:, :K], fx.bf16_round(case['T']))
  np.testing.assert_array_equal(Z.float().cpu().numpy().astype(np.float64), fx.bf16_round(case['Z']))
  return case, Z


@pytest.mark.parametrize('shape', fx.SPECTRAL_SHAPES, ids=lambda s: 'B%d-N%d-din%d-ldx%d-K%d-S%d' % s)
def test_projection_and_gemm1_entries_are_exact_at_every_width(shape):
  """din 1 / 16 / 17 / 127 / 128 and ldx = 32 > din = 10 (NaN planted in the ignored columns), N 129
  / 256 / 257, K 1 / 7 / 16 / 17 / 63 / 64, S 1 / 16: T of lnz_large_spectral (1, 2, 3 pieces) and of
  the fused launch, Z of lnz_large_gemm1_rows, of the fused launch (the same bits) and the
  transposed image of lnz_large_gemm1 EQUAL float64 (one bf16 piece: its rounding); Ybuf is left
  zero, the k padding of Zt and the slots beyond K of Tt stay zero."""
  B, N, din, ldx, K, S = shape
  case, Zfused = _check_projection_exact(shape)
  X = _dev(case['X'])
  abi = ops._abi()
  Wf1, _ = pack_weights(case['Wn'][:, None, :], case['Wl'], 1, DEV)
  Zrows = torch.empty((B, N, 128), dtype=torch.bfloat16, device=DEV)
  abi.large_gemm1_rows(X, ldx, din, Wf1, B, N, Zrows)
  assert torch.equal(Zrows.view(torch.int16), Zfused.view(torch.int16))
  Nk = int(abi.large_nk(N))
  for planes in (1, 2, 3):
    Wf, _ = pack_weights(case['Wn'][:, None, :], case['Wl'], planes, DEV)
    Zt = torch.zeros((planes, B, 1, 128, Nk), dtype=ops.large_plane_dtype(planes), device=DEV)
    abi.large_gemm1(X, ldx, din, Wf, B, N, 1, planes, Zt)
    Zg = _pieces_sum(Zt)[:, 0]
    assert (Zg[..., N:] == 0).all()
    want = case['Z'].transpose(0, 2, 1)
    np.testing.assert_array_equal(Zg[..., :N], fx.bf16_round(want) if planes == 1 else want)


@pytest.mark.parametrize('shape', fx.CHUNK_SHAPES, ids=lambda s: 'B%d-N%d' % s[:2])
def test_projection_row_chunks_beyond_128_rows_are_exact(shape):
  """rows = max(128, roundup64(ceil(N / ceil(256 / B)))): B = 256, N = 140 — ONE chunk of 192 rows
  covers the graph; B = 128, N = 300 — two chunks of 192, the last one ragged.  Y = V^T X is an
  integer sum: the order of the chunks' atomics cannot matter."""
  assert fx.project_rows(*shape[:2])[0] == 192
  _check_projection_exact(shape)


@pytest.mark.parametrize('shape', fx.SPECTRAL_SHAPES, ids=lambda s: 'B%d-N%d-din%d-ldx%d-K%d-S%d' % s)
def test_projection_and_gemm1_entries_real_values_within_the_stage_bars(shape):
  """The T and Z bars of test_large_conv_stages_match_numpy at the same widths; the fused launch's
  Z is lnz_large_gemm1_rows's bit for bit."""
  B, N, din, ldx, K, S = shape
  case = fx.spectral_real_case(*shape)
  X64 = case['X'][..., :din].astype(np.float64)
  T = fx.spectral_reference(X64, case['V'].astype(np.float64), case['G'].astype(np.float64),
                            case['Wl'].astype(np.float64))[0]
  worst = 0.0
  for planes in (1, 2, 3):
    Tg, Ybuf, _ = run_projection(case, shape, planes, DEV, False)
    assert (Ybuf == 0).all()
    worst = max(worst, np.abs(Tg[:, :K] - T).max() / ((8e-3 if planes == 1 else 1e-5) * np.abs(T).max()))
  Tg, Ybuf, Zfused = run_projection(case, shape, 1, DEV, True)
  worst = max(worst, np.abs(Tg[:, :K] - T).max() / (8e-3 * np.abs(T).max()))
  abi = ops._abi()
  Wf1, _ = pack_weights(case['Wn'][:, None, :], case['Wl'], 1, DEV)
  Zrows = torch.empty((B, N, 128), dtype=torch.bfloat16, device=DEV)
  abi.large_gemm1_rows(_dev(case['X']), ldx, din, Wf1, B, N, Zrows)
  assert torch.equal(Zrows.view(torch.int16), Zfused.view(torch.int16))
  Zb = np.einsum('bni,oi->bno', _bf16_round(case['X'][..., :din]), _bf16_round(case['Wn']))
  wz = np.abs(Zrows.float().cpu().numpy() - _bf16_round(Zb)).max() / (8e-3 * np.abs(Zb).max())
  Nk = int(abi.large_nk(N))
  for planes in (2, 3):
    Wf, _ = pack_weights(case['Wn'][:, None, :], case['Wl'], planes, DEV)
    Zt = torch.zeros((planes, B, 1, 128, Nk), dtype=ops.large_plane_dtype(planes), device=DEV)
    abi.large_gemm1(_dev(case['X']), ldx, din, Wf, B, N, 1, planes, Zt)
    Z = np.einsum('bni,oi->bon', X64, case['Wn'].astype(np.float64))
    tol = 2e-6 if planes == 3 else 4e-6
    wz = max(wz, np.abs(_pieces_sum(Zt)[:, 0, :, :N] - Z).max() / (tol * np.abs(Z).max()))
  print('%s: achieved / bar  T %.3f  Z %.3f' % (shape, worst, wz))
  assert worst <= 1.0 and wz <= 1.0


def test_projection_chunk_switch_is_exact_in_both_directions(tmp_path):
  """LNZ_LARGE_PROJECT_WGS = 1 (one chunk of 320 rows) and 4096 (three chunks of 128) at B = 3,
  N = 300, each in a child of its own: T (one piece, fused; three pieces) and Z EQUAL float64."""
  case = fx.spectral_exact_case(*fx.WGS_SHAPE)
  K = fx.WGS_SHAPE[4]
  for wgs in ('1', '4096'):
    got = _child(tmp_path, 'project', 'wgs' + wgs, {'LNZ_LARGE_PROJECT_WGS': wgs})
    assert (got['ybuf'] == 0).all()
    assert (got['T1'][:, K:] == 0).all() and (got['T3'][:, K:] == 0).all()
    np.testing.assert_array_equal(got['T1'][:, :K], fx.bf16_round(case['T']))
    np.testing.assert_array_equal(got['T3'][:, :K], case['T'])
    np.testing.assert_array_equal(got['Z'].astype(np.float64), fx.bf16_round(case['Z']))


# ------------------------------------------------------------------------------ 3. the gathers
def _image(case, cap, channels=2):
  L = _dev(case['L'])
  B, N = L.shape[:2]
  Lx = L.unsqueeze(3).expand(B, N, N, channels) if channels > 1 else L.unsqueeze(3)
  img = ops.large_sparse_image(Lx, cap, values=True)
  assert int(img.flags.item()) == 0
  assert np.array_equal(img.counts.cpu().numpy(), case['plan'])
  return img


def _gather_into(out, img, Z, relu, f32):
  B, N = img.B, img.N
  abi = ops._abi()
  if f32:
    abi.large_sparse_conv_f32(img.entries, img.values, img.counts, img.cap, Z, B, N, int(relu), out)
  else:
    abi.large_sparse_conv(img.entries, img.counts, img.cap, Z, B, N, int(relu), out)
  return out


def _gather(img, Z, X0, relu, f32):
  """the ABI entry on given Z (bf16) / Zf (fp32) and a non-zero X (accumulated in place)"""
  return _gather_into(_dev(X0).clone(), img, Z, relu, f32)


def _z_operand(Z, f32):
  return _dev(Z) if f32 else _dev(Z).to(torch.bfloat16)


@pytest.mark.parametrize('f32', [False, True], ids=['sparse_conv', 'sparse_conv_f32'])
@pytest.mark.parametrize('cap', [128, None], ids=['cap128', 'default_cap32'])
def test_gathers_alone_hold_every_row_length(cap, f32):
  """B = 10, N = 133 (last tile: one wave, five rows), prescribed row lengths 0 .. 128 in another
  order per graph, long -> empty -> long inside one wave: the image's counts equal the plan; on
  integers both gathers EQUAL float64; on real values they stay within the FMA-chain bound; ReLU
  on and off; one channel and its expanded view give the same image."""
  rcap = ops.large_sparse_row_cap(fx.GATHER_N) if cap is None else cap
  assert rcap == (32 if cap is None else 128)
  for exact in (True, False):
    case = fx.gather_case(rcap, exact)
    img = _image(case, cap)
    one = _image(case, cap, channels=1)
    keep = torch.arange(rcap, device=DEV)[None, None, :] < ((img.counts + 7) // 8 * 8)[:, :, None]
    assert torch.equal(img.entries[keep], one.entries[keep]) and torch.equal(img.values[keep], one.values[keep])
    L64 = case['L'].astype(np.float64) if (f32 or exact) else _bf16_round(case['L'])
    Z = _z_operand(case['Z'], f32)
    for relu in (0, 1):
      got = _gather(img, Z, case['X0'], relu, f32).cpu().numpy().astype(np.float64)
      ref, bound = fx.gather_reference(L64, case['Z'].astype(np.float64), case['X0'].astype(np.float64), relu)
      if exact:
        np.testing.assert_array_equal(got, ref)
      else:
        err = np.abs(got - ref)
        assert (err[bound == 0] == 0).all()
        ratio = (err[bound > 0] / bound[bound > 0]).max()
        print('cap %d %s relu %d: achieved / bound %.3f' % (rcap, 'f32' if f32 else 'bf16', relu, ratio))
        assert ratio <= 1.0


def test_image_row_of_exactly_cap_entries_is_kept_and_cap_plus_one_is_flagged():
  case = fx.gather_case(128, True)
  assert case['plan'].max() == 128
  _image(case, 128)                                   # (asserts flags == 0)
  L = case['L'].copy()
  r = int(np.argmax(case['plan'][3]))
  free = np.nonzero(L[3, r] == 0)[0]
  L[3, r, free[0]] = 1.0                              # cap + 1 entries in ONE row
  img = ops.large_sparse_image(_dev(L).unsqueeze(3), 128, values=True)
  assert int(img.flags.item()) == 2


@pytest.mark.parametrize('f32', [False, True], ids=['sparse_conv', 'sparse_conv_f32'])
def test_gathers_keep_graphs_apart(f32):
  """One graph's Z rows non-finite: every other graph's output is bit for bit what it is without
  (the per-graph buffer bounds and the graph map of the second dealing round) — one operator, then
  R = 3 with ONE channel's block of that graph non-finite."""
  case = fx.gather_case(128, False)
  img = _image(case, 128)
  base = _gather(img, _z_operand(case['Z'], f32), case['X0'], 0, f32)   # (no ReLU: it would clear a NaN)
  Zp = case['Z'].copy()
  Zp[1] = np.nan
  Zp[1, ::2] = np.inf
  got = _gather(img, _z_operand(Zp, f32), case['X0'], 0, f32)
  others = [b for b in range(fx.GATHER_B) if b != 1]
  assert torch.equal(got[others], base[others]) and torch.isfinite(got[others]).all()
  empty = torch.from_numpy(case['plan'][1] == 0).to(DEV)
  assert torch.equal(got[1][empty], base[1][empty]) and not torch.isfinite(got[1][~empty]).any()
  # R = 3 operators: the Z block of ONE graph in ONE channel (the per-pair buffer and its bounds)
  R, g, ch = 3, 1, 2
  case = fx.gather_channels_case(128, R)
  imgs = _images(case, 128)
  base = _gather_channels(imgs, _z_operand(case['Z'], f32), case['X0'], 0, f32)
  Zp = case['Z'].copy()
  Zp[ch, g] = np.nan
  Zp[ch, g, ::2] = np.inf
  got = _gather_channels(imgs, _z_operand(Zp, f32), case['X0'], 0, f32)
  assert torch.equal(got[others], base[others]) and torch.isfinite(got[others]).all()
  empty = torch.from_numpy(case['plan'][ch, g] == 0).to(DEV)
  assert torch.equal(got[g][empty], base[g][empty]) and not torch.isfinite(got[g][~empty]).any()


def _images(case, cap):
  imgs = ops.large_sparse_image_channels(_dev(case['L']), cap, values=True)
  assert int(imgs.flags.item()) == 0   # (the inputs: no row of the plan beyond the capacity, test_large_edges_cpu.py)
  assert np.array_equal(imgs.counts.cpu().numpy(), case['plan'])
  return imgs


def _gather_channels(imgs, Z, X0, relu, f32):
  """the channel ABI entry on class-major Z [R,B,N,128] and a non-zero X (accumulated in place)"""
  R, B, N = imgs.R, imgs.B, imgs.N
  out = _dev(X0).clone()
  abi = ops._abi()
  if f32:
    abi.large_sparse_conv_channels_f32(imgs.entries, imgs.values, imgs.counts, imgs.cap, Z, B, N, R, int(relu), out)
  else:
    abi.large_sparse_conv_channels(imgs.entries, imgs.counts, imgs.cap, Z, B, N, R, int(relu), out)
  return out


@pytest.mark.parametrize('f32', [False, True], ids=['sparse_conv_channels', 'sparse_conv_channels_f32'])
@pytest.mark.parametrize('R', [2, 3, 8])
@pytest.mark.parametrize('cap', [128, None], ids=['cap128', 'default_cap32'])
def test_channel_gathers_equal_chained_one_operator_gathers(cap, R, f32):
  """The gather over R operators is R one-operator gathers chained through X: the same fp32 FMA
  sequence (channels ascending, entries in entry order, one accumulator per row) with a store and a
  reload between channels, the activation on the last one — EQUAL bits, no tolerance.  The gather
  case's B = 10, N = 133 with channel c = the graphs rotated by c (other row lengths in every channel
  of a row), R different Z blocks; R = 3: lane % R with no power of two, R = 8: 64 (row, channel)
  pairs.  The channel images: no flag, the rotated plan's counts, and on the live entries the bits of
  the one-operator image of each channel alone."""
  rcap = ops.large_sparse_row_cap(fx.GATHER_N) if cap is None else cap
  case = fx.gather_channels_case(rcap, R)
  imgs = _images(case, cap)
  L = _dev(case['L'])
  for c in range(R):
    one = ops.large_sparse_image(L[..., c:c + 1], cap, values=True)
    assert int(one.flags.item()) == 0 and torch.equal(one.counts, imgs.counts[c])
    keep = torch.arange(rcap, device=DEV)[None, None, :] < ((one.counts + 7) // 8 * 8)[:, :, None]
    assert torch.equal(imgs.entries[c][keep], one.entries[keep])
    assert torch.equal(imgs.values[c][keep], one.values[keep])
  Z = _z_operand(case['Z'], f32)
  for relu in (0, 1):
    got = _gather_channels(imgs, Z, case['X0'], relu, f32)
    assert ops.last_kernel() == ('sparse_conv_channels_f32_kernel' if f32 else 'sparse_conv_channels_kernel')
    chained = _dev(case['X0']).clone()
    for c in range(R):
      _gather_into(chained, imgs.channel(c), Z[c], relu if c == R - 1 else 0, f32)
    assert torch.equal(got, chained) and not torch.equal(got, _dev(case['X0']))


@pytest.mark.parametrize('f32', [False, True], ids=['sparse_conv', 'sparse_conv_f32'])
def test_node_0_non_finite_features_reach_every_padded_row_of_its_graph(f32):
  """the image pads a row to a multiple of 8 entries with `column 0, value
  0.0` and the gathers run fmaf(0.0, Z[node 0], acc) for the padding.  With ONLY node 0's Z row NaN
  in one graph, the NaN rows of that graph are exactly node 0's neighbours AND every row whose count
  is not a multiple of 8; every other row (empty rows, counts 8, 16, ...) and every other graph is
  bit for bit what it is with a finite node 0.  (Any other node's non-finite features reach its
  neighbours only: test_gathers_keep_graphs_apart's empty rows, and the rows checked here.)"""
  g = 2
  case = fx.gather_case(128, False)
  plan, L = case['plan'][g], case['L'][g]
  neighbour = L[:, 0] != 0
  padded = plan % 8 != 0
  assert (padded & ~neighbour).any()                       # a padded row that is NOT a neighbour of node 0
  assert (~padded & ~neighbour & (plan > 0)).any()         # a full row that is not: stays finite
  img = _image(case, 128)
  base = _gather(img, _z_operand(case['Z'], f32), case['X0'], 0, f32)
  Zp = case['Z'].copy()
  Zp[g, 0] = np.nan
  got = _gather(img, _z_operand(Zp, f32), case['X0'], 0, f32)
  hit = torch.from_numpy(neighbour | padded).to(DEV)
  assert torch.isnan(got[g][hit]).all()
  assert torch.equal(got[g][~hit], base[g][~hit])
  others = [b for b in range(fx.GATHER_B) if b != g]
  assert torch.equal(got[others], base[others])
  # another node (not node 0): its neighbours only
  n = 5
  Zq = case['Z'].copy()
  Zq[g, n] = np.nan
  got = _gather(img, _z_operand(Zq, f32), case['X0'], 0, f32)
  hit = torch.from_numpy(L[:, n] != 0).to(DEV)
  assert hit.any() and torch.isnan(got[g][hit]).all() and torch.equal(got[g][~hit], base[g][~hit])


# ------------------------------------------------------------------ 4. one product-surface case
@pytest.mark.parametrize('mode,kernel,bar', [('fp32', 'sparse_conv_f32_kernel', 1e-5),
                                             ('bf16', 'sparse_conv_kernel', 2e-3)])
def test_module_gathers_rows_of_more_than_64_entries(mode, kernel, bar):
  """LanczosNetGeneral, 3 layers, B = 2 at N = 2304, where the default row capacity (72) exceeds
  the 64 entries one wave load holds: a handful of rows of 65..72 entries among sparse ones, the
  image unflagged, the sparse gather named by last_kernel(); the scores equal the streamed kernels'
  at the module tests' bars.  (Orthonormal V and arbitrary D drawn directly: the layer does not need true eigenpairs.)"""
  import oracle
  from large_fixture import general_cfg
  from lanczosnet_amd.model import LanczosNetGeneral
  from lanczosnet_amd.utils.arg_helper import make_model_config
  B, N, K = 2, 2304, 32
  assert ops.large_sparse_row_cap(N) == 72
  cfg = general_cfg(K, 3)
  P = oracle.make_lanczosnet_params(cfg, 17, general=True)
  net = LanczosNetGeneral(make_model_config(cfg, general=True)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
  net = net.to(DEV)
  net.gemm_mode = mode
  g = torch.Generator(device=DEV).manual_seed(23)
  L0 = (torch.rand((B, N, N), device=DEV, generator=g) < 8.0 / N).float() * \
      (torch.rand((B, N, N), device=DEV, generator=g) - 0.5) * 0.5
  planted = {5: 65, 700: 68, 1500: 71, 2303: 72}
  for b in range(B):
    for r, n in planted.items():
      L0[b, r] = 0.0
      cols = torch.randperm(N, device=DEV, generator=g)[:n]
      L0[b, r, cols] = 0.05 * (1 + b)
  L = L0.unsqueeze(3).expand(B, N, N, 2)                     # one operator class: an expanded view
  counts = ops.large_sparse_image(L).counts
  assert int(counts.max()) == 72 and int((counts > 64).sum()) == B * len(planted)
  X = torch.randn((B, N, 10), device=DEV, generator=g)
  hg = torch.Generator().manual_seed(24)
  V = torch.linalg.qr(torch.randn((B, N, K), generator=hg)).Q.contiguous().to(DEV)
  D = torch.rand((B, K), device=DEV, generator=g) * 2.0 - 1.0
  mask = torch.ones((B, N), dtype=torch.uint8, device=DEV)
  mask[1, N - N // 5:] = 0
  with torch.no_grad():
    s = net(X, L, D, V, mask=mask)
    assert ops.last_kernel() == kernel
    assert net._large_sparse_state[torch.device(DEV).index]['last_flags'] == 0
    net.large_sparse = False
    ref = net(X, L, D, V, mask=mask)
  assert torch.isfinite(s).all()
  ratio = (s - ref).abs().max().item() / (bar * ref.abs().max().item())
  print('N=2304 %s mode: sparse vs streamed, achieved / bar %.3f' % (mode, ratio))
  assert ratio <= 1.0
