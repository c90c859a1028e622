"""Worker of tests/test_gpu_large_edges.py for the two switches the library reads once per process:
LNZ_LARGE_CONV_WAVES (4 selects large_conv_kernel<1,4>) and LNZ_LARGE_PROJECT_WGS (the row chunking
of the eigen-space projection).  The test starts this file as a fresh child per setting, one at a
time, and holds the arrays each child writes to the float64 references of large_edges_fixture.
The launch helpers here are the test's own as well."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import large_edges_fixture as fx  # noqa: E402
from lanczosnet_amd import ops  # noqa: E402
from test_gpu_large import _pieces_sum as pieces_sum  # noqa: E402


def to_dev(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def pack_weights(Wn, Wl, planes, dev):
  """Wn [128,C,din] node-space blocks -> Wf (lnz_large_gemm1's fragments, `planes` pieces; None for
  C = 0); Wl [128,S,din] long-scale blocks -> Wt (lnz_pack_rows_k8 image); as the model packs them."""
  C, din = Wn.shape[1], Wn.shape[2]
  S = Wl.shape[1]
  dinp = (din + 15) // 16 * 16
  Wf = None
  if C:
    Wnp = np.zeros((128, C, dinp), np.float32)
    Wnp[..., :din] = Wn
    Wf = ops.large_weight_fragments(ops.split_bf16_planes(
        to_dev(Wnp.transpose(1, 0, 2).reshape(C * 128, dinp), dev), planes))
  Wlp = np.zeros((128, S, dinp), np.float32)
  Wlp[..., :din] = Wl
  Wt = ops.pack_rows_k8(to_dev(Wlp.reshape(128, S * dinp), dev))
  return Wf, Wt


def run_layer(case, planes, relu, dev, out=None):
  """One streamed layer (C >= 1: ops.large_conv_layer; C = 0: the projection and the lift-only
  lnz_large_conv launch of the sparse layers) -> (X' [B,N,128], Zt or None, Tt, Ybuf)."""
  L, X, V, G = (to_dev(case[k], dev) for k in ('L', 'X', 'V', 'G'))
  bias = to_dev(case['bias'], dev)
  B, N, _, C = L.shape
  din = case['din']
  Wf, Wt = pack_weights(case['Wn'], case['Wl'], planes, dev)
  if C:
    Lb, Vb = ops.large_pack_operators(L, V, planes)
    Zt, Tt, Ybuf = work = ops.large_work_buffers(Lb)
    res = ops.large_conv_layer(X, din, Lb, Vb, V, Wf, Wt, G, bias, work, relu=relu, out=out)
    return res, Zt, Tt, Ybuf
  Vb = ops.large_pack_vectors(V, planes)
  Tt = torch.zeros((planes, B, 128, 64), dtype=ops.large_plane_dtype(planes), device=dev)
  Ybuf = torch.zeros((B, 64, 128), dtype=torch.float32, device=dev)
  if out is None:
    out = torch.empty((B, N, 128), dtype=torch.float32, device=dev)
  with torch.cuda.device(dev):
    ops._abi().large_spectral(X, X.shape[2], din, V, G, Wt, B, N, V.shape[2], G.shape[1], planes, Ybuf, Tt)
    ops._abi().large_conv(None, Vb, None, Tt, bias, B, N, 0, planes, int(bool(relu)), out)
  return out, None, Tt, Ybuf


def run_conv_on_images(case, relu, dev):
  """lnz_large_conv (planes = 1) on the HANDED B images of fx.conv_real_case -> X' [B,N,128]"""
  L, V = to_dev(case['L'], dev), to_dev(case['V'], dev)
  B, N, _, C = L.shape
  K = V.shape[2]
  Lb, Vb = ops.large_pack_operators(L, V, 1)
  Zt, Tt, _ = ops.large_work_buffers(Lb)
  Zt[0, :, :, :, :N] = to_dev(case['Zt'], dev).to(torch.bfloat16)
  Tt[0, :, :, :K] = to_dev(case['Tt'], dev).to(torch.bfloat16)
  return ops.large_conv(Lb, Vb, Zt, Tt, to_dev(case['bias'], dev), relu=relu)


def run_projection(case, shape, planes, dev, fused):
  """lnz_large_spectral (or, planes = 1 and `fused`, lnz_large_spectral_gemm1_rows) -> (T [B,64,128]
  float64 sum of the pieces, Ybuf, Z bf16 [B,N,128] or None)"""
  B, N, din, ldx, K, S = shape
  X, V, G = (to_dev(case[k], dev) for k in ('X', 'V', 'G'))
  Wf, Wt = pack_weights(case['Wn'][:, None, :], case['Wl'], 1, dev)
  Tt = torch.zeros((planes, B, 128, 64), dtype=ops.large_plane_dtype(planes), device=dev)
  Ybuf = torch.zeros((B, 64, 128), dtype=torch.float32, device=dev)
  Z = None
  with torch.cuda.device(dev):
    if fused:
      assert planes == 1
      Z = torch.empty((B, N, 128), dtype=torch.bfloat16, device=dev)
      ops._abi().large_spectral_gemm1_rows(X, ldx, din, V, G, Wt, Wf, B, N, K, S, Ybuf, Tt, Z)
    else:
      ops._abi().large_spectral(X, ldx, din, V, G, Wt, B, N, K, S, planes, Ybuf, Tt)
  return pieces_sum(Tt).transpose(0, 2, 1), Ybuf, Z


def conv_waves_outputs(dev):
  """planes = 1 at fx.WAVES_SHAPES: the exact layer with and without ReLU, the real-valued conv"""
  out = {}
  for C, N, B in fx.WAVES_SHAPES:
    case = fx.conv_exact_case(C, N, B)
    for relu in (0, 1):
      out['exact_%d_%d_relu%d' % (C, N, relu)] = run_layer(case, 1, relu, dev)[0].cpu().numpy()
    out['real_%d_%d' % (C, N)] = run_conv_on_images(fx.conv_real_case(C, N, B), True, dev).cpu().numpy()
  return out


def project_outputs(dev):
  """fx.WGS_SHAPE, exact inputs: T of the fused launch (and its Z) and of lnz_large_spectral with
  three pieces; Ybuf's largest magnitude afterwards"""
  case = fx.spectral_exact_case(*fx.WGS_SHAPE)
  T1, Y1, Z = run_projection(case, fx.WGS_SHAPE, 1, dev, True)
  T3, Y3, _ = run_projection(case, fx.WGS_SHAPE, 3, dev, False)
  return dict(T1=T1, T3=T3, Z=Z.float().cpu().numpy(),
              ybuf=np.array([float(Y1.abs().max()), float(Y3.abs().max())]))


def main():
  mode, path = sys.argv[1], sys.argv[2]
  dev = torch.device('cuda', 0)
  if mode == 'conv':
    assert os.environ.get('LNZ_LARGE_CONV_WAVES') in (None, '4')
    out = conv_waves_outputs(dev)
  else:
    assert mode == 'project' and os.environ.get('LNZ_LARGE_PROJECT_WGS') in ('1', '4096')
    out = project_outputs(dev)
  torch.cuda.synchronize()
  np.savez(path, **out)
  print('LARGE_EDGES_OK %s waves=%s wgs=%s' % (mode, os.environ.get('LNZ_LARGE_CONV_WAVES'),
                                               os.environ.get('LNZ_LARGE_PROJECT_WGS')))


if __name__ == '__main__':
  main()
