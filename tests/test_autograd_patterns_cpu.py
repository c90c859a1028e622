"""tests/autograd_patterns.py on the host: the driver itself, the `objective=` / `inputs=` arguments of the float64
restatement of test_gpu_small_train_edges.py, and — P5 — the module's own `forward` with differentiable inputs.

The adapter's "route" is the module's differentiable restatement `_torch_forward` on CPU tensors (plain torch: the
gradient oracle the HIP backward passes are tested against), at two cases of test_gpu_small_train_edges.py.  A
call in which an input requires grad goes through `net(...)` itself — `_guard_forward` and the capture query are
patched, nothing else — so that the routing of such a call ('torch', one warning per module, gradients for
node_feat, D and V with the parameters live or frozen) is what runs.

One hand-written Function runs here whole: `_LanczosNetFunction` (route 'fused_train_torch'), whose backward is
plain torch; its forward kernel launch `_hip_forward` is replaced by the restatement under `no_grad`, everything
else — `forward`'s routing, `Function.apply`, the saved tensors, `torch_param_grads`, `param_grad_tuple`,
`once_differentiable` — is the module's.  Every pattern, P7 included, is held on it.  No GPU.

Conditioning of the objectives the patterns add (fp32 against float64 `_truth`, worst deviation of |g| over the
tensors, one and eight threads): one-node molecules — two batches summed 8.8e-7, score.sum() 1.1e-6, weighted
8.6e-7; General, input width 1 — 1.3e-6, 1.2e-6, 1.0e-6: ten times inside the 1e-5 bar (the seed of the weights:
`autograd_patterns.weighted`)."""
import pytest
import torch

import autograd_patterns as AP
import test_gpu_small_train_edges as SM

CASES = ['one-node molecules, K > n, one output', 'General, input width 1, eight long']


class Host(AP.Route):
  bitwise, hip_route = True, 'restatement'

  def __init__(self, case):
    self.case, self.name, self.general = case, case, SM.CASES[case][-1]

  def make(self):
    c = SM._case(self.case)
    b1 = SM._host_inputs(c)
    return SM._host_net(c).train(), b1, tuple(t[1:] for t in b1)

  def forward(self, net, b):
    X, L, D, V, mask, _ = b
    if any(t.requires_grad for t in (X, D, V)):
      return net(X, L, D, V, mask=mask)
    net.last_route = 'restatement' if torch.is_grad_enabled() else 'restatement, no grad'
    return net._torch_forward(X, L, D, V, mask)

  def label(self, b):
    return b[5]

  def truth(self, net, b, objective, inputs=False):
    r = SM._truth(net, *(t.detach() for t in b), objective=objective, inputs=inputs)
    return (r[1], dict(r[4], node_feat=r[3])) if inputs else r[1]

  def assert_bar(self, grads, truth, tag):
    from test_gpu_mid_train import _deviation
    assert set(grads) == set(truth) and all(float(v.norm()) > 0 for v in truth.values()), tag
    e = _deviation(grads, truth)
    assert e[0] < 1e-5, (tag, e)

  def groups(self, net):
    kind = lambda k: ('embedding' if k.startswith('embedding.') else                       # noqa: E731
                      'spectral_filter' if k.startswith('spectral_filter.') else
                      'head' if k.startswith('att_func.') or k.startswith('filter.%d.' % net.num_layer) else 'conv')
    out = {}
    for k, _ in net.named_parameters():
      out.setdefault(kind(k), []).append(k)
    return out

  def inputs(self, b):
    return dict(node_feat=b[0], D=b[2], V=b[3])

  def with_inputs(self, b, **t):
    X, L, D, V, mask, label = b
    return (t.get('node_feat', X), L, t.get('D', D), t.get('V', V), mask, label)


@pytest.mark.parametrize('pattern', [AP.two_forwards_one_backward, AP.retained_graph, AP.cotangents,
                                     AP.frozen_groups, AP.inference_between], ids=lambda f: f.__name__)
@pytest.mark.parametrize('case', CASES)
def test_pattern_on_the_restatement(case, pattern):
  pattern(Host(case))


class FusedTorch(Host):
  """Route 'fused_train_torch' through `forward` and `_LanczosNetFunction` (fixture `host_forward`)."""
  hip_route = 'fused_train_torch'

  def make(self):
    net, b1, b2 = super().make()
    net.backward_impl = 'torch'
    return net, b1, b2

  def forward(self, net, b):
    X, L, D, V, mask, _ = b
    score = net(X, L, D, V, mask=mask)
    if net.last_route == self.hip_route:
      assert type(score.grad_fn).__name__ == '_LanczosNetFunctionBackward'
    return score


PATTERNS = [AP.two_forwards_one_backward, AP.retained_graph, AP.cotangents, AP.frozen_groups, AP.inference_between,
            AP.double_backward_raises]


@pytest.mark.parametrize('pattern', PATTERNS, ids=lambda f: f.__name__)
@pytest.mark.parametrize('case', CASES)
def test_pattern_on_the_function_of_route_fused_train_torch(case, pattern, host_forward):
  pattern(FusedTorch(case))


def test_p5_on_route_fused_train_torch(host_forward):
  AP.differentiable_inputs(FusedTorch('General, input width 1, eight long'))


def test_every_hand_written_backward_is_once_differentiable():
  """`once_differentiable` wraps the backward it decorates (`__wrapped__`); what it does is held by P7 above."""
  from lanczosnet_amd.model import _ada, _large, _mid, _small, gat, ggnn, mpnn
  functions = [_small._LanczosNetFusedFunction, _small._LanczosNetFunction, _ada._AdaLanczosNetFusedFunction,
               _ada._AdaLanczosNetFunction, _mid._MidGraphFusedFunction, _large._LargeSparseFusedFunction,
               gat._GatTrainFunction, ggnn._GgnnTrainFunction, mpnn._MpnnTrainFunction]
  for fn in functions:
    assert hasattr(fn.backward, '__wrapped__'), fn.__name__


@pytest.fixture
def host_forward(monkeypatch):
  """`forward` on a host module: the device guard answers 'cpu', no stream is capturing."""
  from lanczosnet_amd.model.lanczos_net import _LanczosNetBase
  monkeypatch.setattr(_LanczosNetBase, '_guard_forward', lambda self, L, mask: torch.device('cpu'))
  monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
  monkeypatch.setattr(_LanczosNetBase, '_hip_forward',
                      lambda self, X, L, D, V, mask: self._torch_forward(X, L, D, V, mask).detach())


def test_p5_a_call_with_differentiable_inputs_is_routed_to_the_restatement(host_forward):
  """node_feat / D, V / all three require grad, the parameters live or frozen: route 'torch', the score carries a
  graph, the input gradients within rel_err < 1e-5 of float64, the parameter gradients at their bar, one warning
  per module.  (Before the routing looked at the inputs this call went to `_LanczosNetFusedFunction`, which
  returns None for them; with every parameter frozen it went to the inference kernels.)"""
  AP.differentiable_inputs(Host('General, input width 1, eight long'))


def test_p5_integer_node_ids_with_differentiable_d_and_v(host_forward):
  """The embedding model: node ids cannot require grad, D and V can."""
  import warnings
  from conftest import rel_err
  route = Host(CASES[0])
  net, b1, _ = route.make()
  _, truth_in = route.truth(net, b1, AP.loss_of(net, route.label(b1)), inputs=True)
  leaves = {k: route.inputs(b1)[k].clone().requires_grad_(True) for k in ('D', 'V')}
  with warnings.catch_warnings(record=True) as rec:
    warnings.simplefilter('always')
    score = route.forward(net, route.with_inputs(b1, **leaves))
  assert net.last_route == 'torch' and score.grad_fn is not None
  assert len(rec) == 1 and 'D, V require grad' in str(rec[0].message)
  AP.loss_of(net, route.label(b1))(score).backward()
  for k, t in leaves.items():
    assert rel_err(t.grad.numpy(), truth_in[k].numpy()) < 1e-5, k
