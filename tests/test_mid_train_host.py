"""Host-side checks of the training path for graphs of 33..128 nodes (csrc/conv_mid_grad.hip,
`_MidGraphFusedFunction`): the workspace-size queries, the envelope `_mid_backward_supported`
answers for, and the default of its opt-in switch.  No GPU."""
import pytest

from graph_fixture import GRAPH_CFG


def _lib():
  from lanczosnet_amd import _lib
  return _lib.load()


def test_workspace_queries_answer_on_the_host():
  lib = _lib()
  B, N, K, C, S, nl, dout = 10, 100, 20, 2, 8, 7, 2
  NR = 112
  assert lib.lnz_midgraph_head_grad_workspace_floats(B, dout) == B * (dout + 1) * 129
  want = nl * B * (K * 128 + K * S * 128 + NR * C * 128 + K * S + 128)
  assert lib.lnz_midgraph_project_workspace_floats(B, N, K, C, S, nl) == want
  # without long scales only the node-row operand and the bias partials remain
  assert lib.lnz_midgraph_project_workspace_floats(B, N, K, C, 0, nl) == nl * B * (K * 128 + NR * C * 128 + 128)
  assert lib.lnz_midgraph_project_workspace_floats(0, N, K, C, S, nl) == 0
  assert lib.lnz_midgraph_head_grad_workspace_floats(B, 0) == 0
  # the backward's stored activations are the forward's exchange buffer
  assert lib.lnz_midgraph_workspace_floats(B, N, nl) == nl * B * NR * 128


def _module(name='LanczosNetGeneral', **over):
  import oracle
  from lanczosnet_amd import model
  from lanczosnet_amd.utils.arg_helper import make_model_config
  general = name == 'LanczosNetGeneral'
  cfg = dict(GRAPH_CFG if general else dict(oracle.DEFAULT_QM8_CFG, num_bond_type=1), **over)
  return getattr(model, name)(make_model_config(cfg, general=general))


def test_the_switch_defaults_to_the_torch_route():
  from lanczosnet_amd.model import LanczosNet, LanczosNetGeneral
  import os
  if 'LANCZOSNET_MID_BACKWARD' not in os.environ:
    assert LanczosNet.mid_backward_impl == 'torch' and LanczosNetGeneral.mid_backward_impl == 'torch'
  net = _module()
  assert net.mid_backward_impl == LanczosNetGeneral.mid_backward_impl
  net.mid_backward_impl = 'torch'
  assert not net._mid_backward_supported(100, 20, 2)


@pytest.mark.parametrize('name,over,N,K,C,want', [
    ('LanczosNetGeneral', {}, 100, 20, 2, True),                       # the reference's graph configuration
    ('LanczosNetGeneral', {}, 33, 20, 2, True),
    ('LanczosNetGeneral', {}, 128, 32, 1, True),
    ('LanczosNet', dict(hidden_dim=[128] * 3, num_layer=3), 60, 20, 2, True),   # the embedding model
    ('LanczosNetGeneral', dict(long_diffusion_dist=list(range(1, 17))), 100, 20, 2, True),
    ('LanczosNetGeneral', dict(long_diffusion_dist=[]), 100, 20, 2, True),
    ('LanczosNetGeneral', dict(input_dim=128), 100, 20, 2, True),
    ('LanczosNetGeneral', {}, 32, 20, 2, False),                       # the 32-row tile has its own backward
    ('LanczosNetGeneral', {}, 129, 20, 2, False),
    ('LanczosNetGeneral', {}, 100, 33, 2, False),
    ('LanczosNetGeneral', {}, 100, 20, 3, False),
    ('LanczosNetGeneral', dict(short_diffusion_dist=[1]), 100, 20, 2, False),
    ('LanczosNetGeneral', dict(long_diffusion_dist=list(range(1, 18))), 100, 20, 2, False),
    ('LanczosNetGeneral', dict(hidden_dim=[64] * 7), 100, 20, 2, False),
    ('LanczosNetGeneral', dict(input_dim=130), 100, 20, 2, False),
])
def test_mid_backward_envelope(name, over, N, K, C, want):
  net = _module(name, **over)
  net.mid_backward_impl = 'hip'
  assert net._mid_backward_supported(N, K, C) is want
  net.backward_impl = 'torch'
  assert net._mid_backward_supported(N, K, C) is False
  net.backward_impl, net.gemm_mode = 'hip', 'f16x3'
  assert net._mid_backward_supported(N, K, C) is False
