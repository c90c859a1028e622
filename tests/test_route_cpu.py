"""`_LanczosNetBase._route`: which path `forward` takes for (architecture, N, K, operator channels,
gradients, dropout, capture), asked on the host.  The expected names are read off the `if` chain
`forward` had before the route function existed:

  fused = _fused_supported() and _fused_channels_ok()
  N > 32 or not fused or drop:
    not drop, gradients, _mid_backward_supported(N, K, C), not capturing -> 'mid_train_hip'
    gradients or drop                                                   -> 'torch'
    _mid_hip_supported(N, K, C)                                         -> 'mid'
    N > 32 and _large_hip_supported(K, C)                               -> 'large_hip'
    else                                                                -> 'library'
  gradients: _fused_backward_supported() -> 'fused_train_hip', else 'fused_train_torch'
  else 'fused'

No GPU."""
import pytest

from graph_fixture import GRAPH_CFG

ROUTES = {'fused', 'fused_train_hip', 'fused_train_torch', 'mid', 'mid_train_hip', 'large_hip',
          'library', 'torch'}
# every class-level switch a route depends on, pinned (the environment may set the class defaults)
SWITCHES = dict(gemm_mode='fp32', backward_impl='hip', mid_backward_impl='torch', mid_graph_kernel=True)


def _module(name, over, switches):
  import oracle
  from lanczosnet_amd import model
  from lanczosnet_amd.utils.arg_helper import make_model_config
  general = name == 'LanczosNetGeneral'
  cfg = dict(GRAPH_CFG if general else oracle.DEFAULT_QM8_CFG, **over)
  net = getattr(model, name)(make_model_config(cfg, general=general))
  for k, v in dict(SWITCHES, **switches).items():
    setattr(net, k, v)
  return net


G, Q = 'LanczosNetGeneral', 'LanczosNet'   # graph config: 7 x 128, 8 long scales, input 10; QM8: + embedding
LONG = lambda n: dict(long_diffusion_dist=list(range(1, n + 1)))    # noqa: E731
SHORT = lambda n: dict(short_diffusion_dist=list(range(1, n + 1)))  # noqa: E731
MIDHIP = dict(mid_backward_impl='hip')
INFER, TRAIN = (False, False, False), (True, False, False)          # (needs_grad, drop, capturing)

CASES = [
    # ---- node count: 32 | 33 .. 128 | 129
    (G, {}, {}, 32, 20, 2, INFER, 'fused'),
    (G, {}, {}, 33, 20, 2, INFER, 'mid'),
    (G, {}, {}, 128, 20, 2, INFER, 'mid'),
    (G, {}, {}, 129, 20, 2, INFER, 'large_hip'),
    (Q, {}, {}, 32, 20, 7, INFER, 'fused'),
    (Q, {}, {}, 9, 20, 7, TRAIN, 'fused_train_hip'),
    # ---- Ritz pairs: 32 | 33 (one launch), 64 | 65 (streamed kernels)
    (G, {}, {}, 100, 32, 2, INFER, 'mid'),
    (G, {}, {}, 100, 33, 2, INFER, 'large_hip'),
    (G, {}, {}, 100, 64, 2, INFER, 'large_hip'),
    (G, {}, {}, 100, 65, 2, INFER, 'library'),
    (G, {}, {}, 2048, 64, 2, INFER, 'large_hip'),
    (G, {}, {}, 2048, 65, 2, INFER, 'library'),
    (G, {}, {}, 32, 65, 2, INFER, 'fused'),
    # ---- operator channels of L: 2 | 3 (one launch), 8 | 9 (streamed kernels)
    (G, {}, {}, 100, 20, 2, INFER, 'mid'),
    (G, {}, {}, 100, 20, 3, INFER, 'large_hip'),
    (G, {}, {}, 100, 20, 8, INFER, 'large_hip'),
    (G, {}, {}, 100, 20, 9, INFER, 'library'),
    (G, {}, {}, 2048, 20, 8, INFER, 'large_hip'),
    (G, {}, {}, 2048, 20, 9, INFER, 'library'),
    # ---- long scales: 12 | 13 (fused kernels), 16 | 17 (gains kernels: one launch, streamed)
    (G, LONG(12), {}, 32, 20, 2, INFER, 'fused'),
    (G, LONG(12), {}, 32, 20, 2, TRAIN, 'fused_train_hip'),
    (G, LONG(13), {}, 32, 20, 2, INFER, 'library'),
    (G, LONG(13), {}, 32, 20, 2, TRAIN, 'torch'),
    (G, LONG(13), {}, 100, 20, 2, INFER, 'mid'),
    (G, LONG(16), {}, 100, 20, 2, INFER, 'mid'),
    (G, LONG(17), {}, 100, 20, 2, INFER, 'library'),
    (G, LONG(16), {}, 2048, 64, 2, INFER, 'large_hip'),
    (G, LONG(17), {}, 2048, 64, 2, INFER, 'library'),
    (G, LONG(0), {}, 100, 20, 2, INFER, 'mid'),
    # ---- short scales: 8 | 9 (fused kernels); none beyond 32 nodes
    (G, SHORT(8), {}, 32, 20, 2, INFER, 'fused'),
    (G, SHORT(8), {}, 32, 20, 2, TRAIN, 'fused_train_hip'),
    (G, SHORT(9), {}, 32, 20, 2, INFER, 'library'),
    (G, SHORT(9), {}, 32, 20, 2, TRAIN, 'torch'),
    (G, SHORT(1), {}, 100, 20, 2, INFER, 'library'),
    (G, SHORT(1), {}, 2048, 64, 2, INFER, 'library'),
    # ---- message channels in all: 8 short + 12 long + 12 operators = 32 | 33
    (Q, dict(SHORT(8), **LONG(12), num_bond_type=11), {}, 32, 20, 12, INFER, 'fused'),
    (Q, dict(SHORT(8), **LONG(12), num_bond_type=12), {}, 32, 20, 13, INFER, 'library'),
    (Q, dict(LONG(12), num_bond_type=19), {}, 32, 20, 20, TRAIN, 'fused_train_hip'),
    (Q, dict(LONG(12), num_bond_type=20), {}, 32, 20, 21, TRAIN, 'torch'),
    # ---- widths
    (G, dict(hidden_dim=[64] * 7), {}, 32, 20, 2, INFER, 'fused'),
    (G, dict(hidden_dim=[64] * 7), {}, 32, 20, 2, TRAIN, 'fused_train_torch'),
    (G, dict(hidden_dim=[64] * 7), {}, 100, 20, 2, INFER, 'library'),
    (G, dict(hidden_dim=[64] * 7), {}, 2048, 64, 2, INFER, 'library'),
    (G, dict(hidden_dim=[96] * 7), {}, 32, 20, 2, INFER, 'library'),
    (G, dict(hidden_dim=[96] * 7), {}, 32, 20, 2, TRAIN, 'torch'),
    (G, dict(hidden_dim=[128] * 6 + [64]), {}, 32, 20, 2, INFER, 'library'),
    (G, dict(input_dim=128), {}, 32, 20, 2, INFER, 'fused'),
    (G, dict(input_dim=130), {}, 32, 20, 2, INFER, 'library'),
    (G, dict(input_dim=130), {}, 100, 20, 2, INFER, 'library'),
    (G, dict(output_dim=31), {}, 32, 20, 2, INFER, 'fused'),
    (G, dict(output_dim=32), {}, 32, 20, 2, INFER, 'library'),
    (G, dict(output_dim=32), {}, 100, 20, 2, INFER, 'large_hip'),
    # ---- training at <= 32 nodes: the `backward_impl` toggle, the split-precision mode
    (G, {}, {}, 32, 20, 2, TRAIN, 'fused_train_hip'),
    (G, {}, dict(backward_impl='torch'), 32, 20, 2, TRAIN, 'fused_train_torch'),
    (G, {}, dict(gemm_mode='f16x3'), 32, 20, 2, TRAIN, 'fused_train_torch'),
    (G, {}, dict(gemm_mode='f16x3'), 32, 20, 2, INFER, 'fused'),
    (G, {}, {}, 32, 20, 2, (True, False, True), 'fused_train_hip'),
    # ---- training at 33 .. 128 nodes: opt-in, both toggles, capture
    (G, {}, {}, 100, 20, 2, TRAIN, 'torch'),
    (G, {}, MIDHIP, 100, 20, 2, TRAIN, 'mid_train_hip'),
    (G, {}, MIDHIP, 33, 20, 2, TRAIN, 'mid_train_hip'),
    (G, {}, MIDHIP, 128, 32, 1, TRAIN, 'mid_train_hip'),
    (G, {}, MIDHIP, 32, 20, 2, TRAIN, 'fused_train_hip'),
    (G, {}, MIDHIP, 129, 20, 2, TRAIN, 'torch'),
    (G, {}, MIDHIP, 100, 33, 2, TRAIN, 'torch'),
    (G, {}, MIDHIP, 100, 20, 3, TRAIN, 'torch'),
    (G, {}, dict(MIDHIP, backward_impl='torch'), 100, 20, 2, TRAIN, 'torch'),
    (G, {}, MIDHIP, 100, 20, 2, (True, False, True), 'torch'),
    (G, {}, MIDHIP, 100, 20, 2, INFER, 'mid'),
    (Q, dict(num_bond_type=1), MIDHIP, 60, 20, 2, TRAIN, 'mid_train_hip'),
    (G, {}, {}, 2048, 64, 2, TRAIN, 'torch'),
    # ---- the other switches of the one-launch kernel
    (G, {}, dict(mid_graph_kernel=False), 100, 20, 2, INFER, 'large_hip'),
    (G, {}, dict(gemm_mode='bf16'), 100, 20, 2, INFER, 'large_hip'),
    (G, {}, dict(MIDHIP, gemm_mode='bf16'), 100, 20, 2, TRAIN, 'torch'),
    # ---- dropout in training: the torch restatement whatever else holds
    (G, dict(dropout=0.5), {}, 32, 20, 2, (True, True, False), 'torch'),
    (G, dict(dropout=0.5), {}, 32, 20, 2, (False, True, False), 'torch'),
    (G, dict(dropout=0.5), MIDHIP, 100, 20, 2, (True, True, False), 'torch'),
    (G, dict(dropout=0.5), {}, 2048, 64, 2, (False, True, False), 'torch'),
    (G, dict(dropout=0.5), {}, 32, 20, 2, INFER, 'fused'),           # (eval mode: no dropout)
    (G, dict(dropout=0.5), {}, 100, 20, 2, INFER, 'mid'),
]


@pytest.mark.parametrize('name,over,switches,N,K,C,flags,want', CASES)
def test_route(name, over, switches, N, K, C, flags, want):
  assert want in ROUTES
  net = _module(name, over, switches)
  assert net._route(N, K, C, *flags) == want


def test_routes_follow_the_predicates_the_tests_call():
  """The seven predicates stay the source of the answer: flipping one on the instance moves the route."""
  net = _module(G, {}, MIDHIP)
  assert net._route(100, 20, 2, *TRAIN) == 'mid_train_hip'
  net._mid_backward_supported = lambda N, K, C: False
  assert net._route(100, 20, 2, *TRAIN) == 'torch'
  assert net._route(100, 20, 2, *INFER) == 'mid'
  net._mid_hip_supported = lambda N, K, C: False
  assert net._route(100, 20, 2, *INFER) == 'large_hip'
  net._large_hip_supported = lambda K, C=1: False
  assert net._route(100, 20, 2, *INFER) == 'library'
  assert net._route(32, 20, 2, *TRAIN) == 'fused_train_hip'
  net._fused_backward_supported = lambda: False
  assert net._route(32, 20, 2, *TRAIN) == 'fused_train_torch'
  net._fused_channels_ok = lambda: False
  assert net._route(32, 20, 2, *INFER) == 'library'


def test_warning_text_names_the_limits_once():
  """The library-path warning is built from the envelope constants; its text is the one the module
  has always emitted."""
  import warnings
  net = _module(G, dict(hidden_dim=[96] * 7), {})
  with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter('always')
    net._warn_library_path(False)
    net._warn_library_path(False)   # once per module
  assert len(w) == 1
  assert str(w[0].message) == (
      'lanczosnet_amd: hidden_dim=[96, 96, 96, 96, 96, 96, 96] / input_dim=10 is outside the fused MFMA '
      'kernel (uniform width 64 or 128, <= 8 short and <= 12 long scales, <= 32 channels in all, no '
      'training dropout): using the device library-GEMM path (hipBLASLt conv + HIP spectral gains; '
      'differentiable torch ops when gradients or dropout are needed), which is slower')
