"""The compact first and last Linear of the spectral-gains MLP (csrc/gains_body.hpp, COMPACT)
against the padded form it replaces as the default (LNZ_GAINS_COMPACT=0) and against the float64
oracle.

The compact form issues fewer matrix instructions for the same sums in the same order: S <= 8
features ride on both k-halves of the first Linear's 32x32x2 MFMAs, and the last Linear runs on
4x4x1 MFMAs, four output features at a time.  An fp32 MFMA is a k-ordered fmaf chain, so the two
forms are expected to agree bit for bit; the oracle bar (`rel_err` < 1e-5, the project's parity bar,
as in test_gpu_gains.py) holds for each form on its own.

The two forms are fixed per process, so one fresh child per form computes every case once
(gains_compact_worker.py); the tests below share what the children wrote."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err
from gains_compact_worker import OFF_W0C, PACK_SIZE, SCALES, SHAPES, case_inputs, cases, compact_images
from gains_tiles_worker import DIST16, gains_cfg, mlp_layers
from lanczosnet_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(x):
  return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope='module')
def forms(tmp_path_factory):
  """{'padded' | 'compact': {(S, B, K, L): (G, G_rows)}}, each form from its own child process"""
  tmp = tmp_path_factory.mktemp('gains_compact')
  env = {k: v for k, v in os.environ.items() if k not in ('LNZ_GAINS_COMPACT', 'LNZ_GAINS_TILES')}
  got = {}
  for name, extra in (('padded', {'LNZ_GAINS_COMPACT': '0'}), ('compact', {})):
    path = str(tmp / (name + '.f32'))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gains_compact_worker.py'), path],
                         cwd=ROOT, env=dict(env, **extra), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert 'GAINS_COMPACT_OK form=%s' % extra.get('LNZ_GAINS_COMPACT') in out.stdout
    flat = np.fromfile(path, dtype=np.float32)
    got[name], at = {}, 0
    for (S, B, K, L) in cases():
      n = L * B * S * K
      got[name][(S, B, K, L)] = (flat[at:at + n].reshape(L, B, S, K), flat[at + n:at + 2 * n].reshape(L, B, S, K))
      at += 2 * n
    assert at == flat.size
  return got


def test_the_shapes_reach_both_kernels():
  """the launch rule of lnz_spectral_gains_rows_split_to, restated"""
  two = [(B * K + 31) // 32 * L >= 2048 for B, K, L in SHAPES]
  assert two == [False, False, True, True]
  assert all(0 < (B * K) % 64 for B, K, L in SHAPES[2:])   # ragged second tile
  assert set(SCALES) >= {1, 3, 5, 7, 8, 9, 16}


@pytest.mark.parametrize('B,K,L', SHAPES)
@pytest.mark.parametrize('S', SCALES)
def test_compact_equals_padded_bit_for_bit(forms, S, B, K, L):
  """G as bytes, without and with the live-row list; the list leaves every other slot zero and
  changes no live slot."""
  pad, pad_rows = forms['padded'][(S, B, K, L)]
  com, com_rows = forms['compact'][(S, B, K, L)]
  differ = int((pad.view(np.uint32) != com.view(np.uint32)).sum())
  print('compact vs padded: S=%d B=%d K=%d L=%d: %d of %d floats differ, max |diff| %.3e'
        % (S, B, K, L, differ, pad.size, float(np.abs(pad.astype(np.float64) - com).max())))
  assert pad.tobytes() == com.tobytes()
  assert pad_rows.tobytes() == com_rows.tobytes()
  _, _, n = case_inputs(S, B, K, L)
  sel = np.broadcast_to((np.arange(K)[None, :] < np.minimum(n, K)[:, None])[None, :, None, :], com.shape)
  assert np.array_equal(com_rows[sel].view(np.uint32), com[sel].view(np.uint32))
  assert (com_rows[~sel] == 0).all()


@pytest.mark.parametrize('B,K,L', SHAPES)
@pytest.mark.parametrize('S', SCALES)
def test_both_forms_match_the_float64_oracle(forms, S, B, K, L):
  cfg = gains_cfg(S, L)
  P, D, _ = case_inputs(S, B, K, L)
  refs = [oracle.spectral_gains(P, cfg, D, l, dtype=np.float64) for l in range(L)]   # B x K x S
  for name in ('padded', 'compact'):
    G = forms[name][(S, B, K, L)][0]
    assert np.isfinite(G).all()
    worst = max(rel_err(G[l].transpose(0, 2, 1), refs[l]) for l in range(L))
    print('%s vs fp64: S=%d B=%d K=%d L=%d: rel_err %.3e' % (name, S, B, K, L, worst))
    assert worst < 1e-5, name


@pytest.mark.parametrize('S', [1, 8, 9, 16])
def test_the_two_packers_write_the_same_compact_images(S):
  """lnz_pack_spectral_mlp per layer and lnz_pack_spectral_mlp_layers: the same bytes behind the
  prefetch slack, and the bytes the index maps of gains_body.hpp say (numpy restatement)."""
  L = 3
  P = oracle.make_lanczosnet_params(gains_cfg(S, L), 600 + S)
  layers = mlp_layers(P, L, DEV)
  one = torch.stack([ops.pack_spectral_mlp(lins, S) for lins in layers]).cpu().numpy()
  all_ = ops.pack_spectral_mlp_layers(layers, S).cpu().numpy()
  assert one.shape == all_.shape == (L, PACK_SIZE)
  assert one[:, OFF_W0C:].tobytes() == all_[:, OFF_W0C:].tobytes()
  for l in range(L):
    W0 = P['spectral_filter.%d.0.weight' % l]
    W6 = P['spectral_filter.%d.6.weight' % l]
    assert all_[l, OFF_W0C:].tobytes() == compact_images(W0, W6, S).tobytes()


@pytest.mark.parametrize('S', [7, 8])
def test_fused_preparation_launch_computes_the_compact_gains(S):
  """lnz_prepare_batch_prev_gains on a small ragged batch, S <= 8 (both compact paths live): the
  previous batch's gains equal the standalone launch bit for bit on the live slots."""
  from lanczosnet_amd.model import LanczosNet
  from lanczosnet_amd.synthetic import draw_batch
  from lanczosnet_amd.utils.arg_helper import make_model_config
  assert os.environ.get('LNZ_GAINS_COMPACT') in (None, '1')
  cfg = dict(oracle.DEFAULT_QM8_CFG, long_diffusion_dist=DIST16[:S], num_layer=3, hidden_dim=[128] * 3)
  net = LanczosNet(make_model_config(cfg)).eval()
  net.load_state_dict({k: torch.from_numpy(v) for k, v in oracle.make_lanczosnet_params(cfg, 6).items()})
  net = net.to(DEV)
  plan = net._plan()
  gains = (DIST16[:S], 3, plan['mlp_pack'])
  ba, bb = draw_batch(45, seed=3, n_min=1, n_max=26), draw_batch(70, seed=4)
  prep = {}
  for key, b in (('a', ba), ('b', bb)):
    n = _t(b['n_nodes'])
    L = ops.laplacian_l4(_t(b['adjs']), n)
    mask = _t(b['node_mask']).contiguous()
    prep[key] = (L, mask, n) + tuple(ops.prepare_batch(plan, L, mask, n, 20))
  La, ma, na, Lpa, tla, rowsa, Da, Va = prep['a']
  Lb, mb, nb, Lpb, tlb, rowsb, Db, Vb = prep['b']
  Ga = ops.spectral_gains(Da, *gains, rows=rowsa)
  Lp2, tl2, rows2, D2, V2, G2 = ops.prepare_batch_prev_gains(plan, Lb, mb, nb, 20, prev=(Da, rowsa), gains=gains)
  assert torch.equal(Lp2, Lpb) and torch.equal(D2, Db) and torch.equal(V2, Vb)
  live = torch.clamp(na, max=20).long()
  sel = (torch.arange(20, device=DEV)[None, :] < live[:, None])[None, :, None, :].expand_as(Ga)
  assert tuple(G2.shape) == (3, 45, S, 20) and bool(sel.any())
  assert torch.equal(Ga[sel], G2[sel])
  # and the standalone launch it is compared with is itself right
  Gref = oracle.spectral_gains({k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}, cfg,
                               Da.cpu().numpy(), 1, dtype=np.float64)
  G_full = ops.spectral_gains(Da, *gains).cpu().numpy()
  assert rel_err(G_full[1].transpose(0, 2, 1), Gref) < 1e-5
