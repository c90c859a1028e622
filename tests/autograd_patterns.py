"""The ways autograd may drive a hand-written training route beyond `zero_grad`, one forward, the module's
loss, one `backward()` — as plain functions over a small route adapter (`Route`).  No GPU code of its own: a
GPU file supplies one adapter per HIP training route (the net and its batches from that route's suite, its
`_hip` / `last_kernel()` / `last_route` check, its float64 restatement given the pattern's `objective=`, its bar)
and calls every pattern.  tests/test_autograd_patterns_cpu.py drives them on the host, through the module's
differentiable restatement and, for P5, through `forward` itself.

Let g(batch) be the gradients of one plain step on the HIP route; the suites of the routes hold it to float64.

  P1 two_forwards_one_backward   s1 = net(b1), s2 = net(b2), (obj(s1) + obj(s2)).backward(): the route's bar
                                 against the float64 truth of the summed objective; on a route whose suite
                                 asserts step-to-step bitwise reproducibility also the bits of two separate
                                 steps accumulated without zero_grad (fp32 a + b commutes)
  P2 retained_graph              backward(retain_graph=True), backward(): bitwise 2 g (g + g is exact)
  P3 cotangents                  (a) score.sum(): an expanded, zero-stride cotangent; (b) a non-contiguous one;
                                 both at the route's bar against float64 with that objective; (c) the objective
                                 of (b) times 2^10 and 2^-10: bitwise 2^+-10 times (b) — a power of two commutes
                                 with every fp32 rounding in range — and no gradient entry subnormal
  P4 frozen_groups               each parameter group frozen alone: the same route, `grad is None` on the frozen
                                 tensors, every other gradient bitwise g
  P5 differentiable_inputs       node_feat / D, V require grad: the input gradients within rel_err < 1e-5 of
                                 float64, the parameter gradients at their bar, the same with every parameter
                                 frozen; the route is the differentiable one, and the module says so once
  P6 inference_between           training forward of b1, `no_grad` forward of b2, backward: bitwise g(b1)
  P7 double_backward_raises      differentiating the gradients raises RuntimeError (`once_differentiable`)
"""
import contextlib
import warnings

import pytest
import torch

from conftest import rel_err

SUBNORMAL = 2.0 ** -126   # the smallest normal fp32


class Route:
  """What a pattern needs of a HIP training route.  A batch is whatever the adapter's own methods take."""
  name = None
  bitwise = False      # the route's suite asserts step-to-step bitwise reproducibility (P1's second half)
  general = False      # a LanczosNetGeneral route: float node features (P5)
  hip_route = None     # `net.last_route` of a step on this route

  def make(self):
    """-> (net on the HIP route, b1, b2); b2 is b1 without one graph: other shapes"""
    raise NotImplementedError

  def forward(self, net, b):
    """-> score"""
    raise NotImplementedError

  def label(self, b):
    raise NotImplementedError

  def check_forward(self, net):
    """after a forward with gradients on: the HIP route took it"""
    assert net.last_route == self.hip_route, (self.name, net.last_route)

  def check_backward(self, net):
    """after a backward: the route's own backward kernel ran"""

  def truth(self, net, b, objective, inputs=False):
    """float64 gradients of `objective(score)` by parameter name [, by input name]"""
    raise NotImplementedError

  def sum_truth(self, t1, t2):
    """the truth of a sum of two objectives"""
    return {k: t1[k] if t2[k] is None else t2[k] if t1[k] is None else t1[k] + t2[k] for k in t1}

  def assert_bar(self, grads, truth, tag):
    """the route's existing bar of a step's gradients against float64"""
    raise NotImplementedError

  def groups(self, net):
    """{group: [parameter names]}: what P4 freezes, one group at a time"""
    raise NotImplementedError

  def inputs(self, b):
    """{'node_feat' | 'D' | 'V': tensor}: the floating inputs of the batch (P5)"""
    raise NotImplementedError

  def with_inputs(self, b, **tensors):
    """the batch with those inputs replaced"""
    raise NotImplementedError


# ---- objectives: callables score -> scalar (rows: the molecules' permutation, for truths that permute the batch)
def loss_of(net, label):
  def objective(score, rows=None):
    lab = label.to(score)
    return net.loss_func(score, lab if rows is None else lab[torch.as_tensor(rows)])
  return objective


def total(score, rows=None):
  return score.sum()


def weighted(shape, scale=1.0, seed=20):
  """sum(score^T * w^T) * scale for a fixed seeded w.  The product is taken against a contiguous w^T, so that
  the cotangent of score^T is contiguous and that of score its transpose: NOT contiguous (B, P > 1).
  The seed is chosen for conditioning, from the float64 truth alone: under seed 11 the four graphs' shares of
  d/d att_func.0.bias on the one-node case cancel to |g| = 4e-4 (0.05 .. 0.3 under the other seeds of 11 .. 30),
  and fp32 torch itself lands 4e-6 or 2e-5 from float64 depending on the host; under seed 20 |g| is 0.15 and 0.23
  on the two host cases and fp32 `_truth` is 9e-7 and 1e-6 from float64."""
  w = torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed))

  def objective(score, rows=None):
    wt = (w if rows is None else w[torch.as_tensor(rows)]).to(score).t().contiguous()
    return (score.t() * wt).sum() * scale
  return objective


# ---- steps
def grads_of(net):
  return {k: None if p.grad is None else p.grad.detach().clone() for k, p in net.named_parameters()}


def step(route, net, b, objective=None, zero=True, hook=None):
  """One step on the HIP route -> gradients by name (None: no gradient)."""
  if zero:
    net.zero_grad(set_to_none=True)
  score = route.forward(net, b)
  route.check_forward(net)
  assert score.requires_grad and score.grad_fn is not None
  if hook is not None:
    score.register_hook(hook)
  (objective or loss_of(net, route.label(b)))(score).backward()
  route.check_backward(net)
  return grads_of(net)


def assert_bitwise(got, want, tag, scale=None):
  assert set(got) == set(want), tag
  for k, w in want.items():
    if w is None:
      assert got[k] is None, (tag, k)
    else:
      assert got[k] is not None and torch.equal(got[k], w if scale is None else w * scale), (tag, k)


@contextlib.contextmanager
def _frozen(net, names):
  params = dict(net.named_parameters())
  was = {k: params[k].requires_grad for k in names}
  for k in names:
    params[k].requires_grad_(False)
  try:
    yield
  finally:
    for k, v in was.items():
      params[k].requires_grad_(v)


# ---- P1
def two_forwards_one_backward(route):
  net, b1, b2 = route.make()
  o1, o2 = loss_of(net, route.label(b1)), loss_of(net, route.label(b2))
  net.zero_grad(set_to_none=True)
  s1 = route.forward(net, b1)
  route.check_forward(net)
  s2 = route.forward(net, b2)
  route.check_forward(net)
  assert s1.shape != s2.shape
  (o1(s1) + o2(s2)).backward()
  route.check_backward(net)
  g = grads_of(net)
  route.assert_bar(g, route.sum_truth(route.truth(net, b1, o1), route.truth(net, b2, o2)), 'P1 %s' % route.name)
  if route.bitwise:
    step(route, net, b1)
    assert_bitwise(g, step(route, net, b2, zero=False), 'P1 %s: two steps accumulated' % route.name)


# ---- P2
def retained_graph(route):
  net, b1, _ = route.make()
  g = step(route, net, b1)
  net.zero_grad(set_to_none=True)
  score = route.forward(net, b1)
  route.check_forward(net)
  loss = loss_of(net, route.label(b1))(score)
  loss.backward(retain_graph=True)
  route.check_backward(net)
  assert_bitwise(grads_of(net), g, 'P2 %s: the first backward' % route.name)
  loss.backward()
  route.check_backward(net)
  assert_bitwise(grads_of(net), g, 'P2 %s: g + g' % route.name, scale=2.0)


# ---- P3
def _no_subnormals(grads, tag):
  for k, g in grads.items():
    if g is not None:
      a = g.abs()
      assert not bool(((a > 0) & (a < SUBNORMAL)).any()), (tag, k)


def cotangents(route):
  net, b1, _ = route.make()
  with torch.no_grad():
    shape = tuple(route.forward(net, b1).shape)
  seen = []
  hook = lambda g: seen.append((tuple(g.stride()), g.is_contiguous())) and None   # noqa: E731
  # (a) an expanded cotangent
  g_a = step(route, net, b1, total, hook=hook)
  assert seen.pop() == ((0, 0), shape[0] * shape[1] == 1), route.name
  assert all(torch.isfinite(v).all() for v in g_a.values() if v is not None)
  route.assert_bar(g_a, route.truth(net, b1, total), 'P3a %s' % route.name)
  # (b) a non-contiguous one
  g_b = step(route, net, b1, weighted(shape), hook=hook)
  assert seen.pop()[1] == (min(shape) == 1), route.name
  route.assert_bar(g_b, route.truth(net, b1, weighted(shape)), 'P3b %s' % route.name)
  _no_subnormals(g_b, 'P3b %s' % route.name)
  # (c) powers of two
  for e in (10, -10):
    g_c = step(route, net, b1, weighted(shape, scale=2.0 ** e))
    _no_subnormals(g_c, 'P3c %s 2^%d' % (route.name, e))
    assert_bitwise(g_c, g_b, 'P3c %s 2^%d' % (route.name, e), scale=2.0 ** e)


# ---- P4
def frozen_groups(route, prepare=None, only=None):
  """prepare(net): a switch to set first (`mlp_grad_impl = 'torch'`); only: the groups to freeze (None: each)."""
  net, b1, _ = route.make()
  if prepare is not None:
    prepare(net)
  g = step(route, net, b1)
  groups = route.groups(net)
  assert set(sum(groups.values(), [])) == {k for k, v in g.items()}, 'every parameter is in a group'
  for name, frozen in groups.items():
    if only is not None and name not in only:
      continue
    assert frozen, name
    with _frozen(net, frozen):
      got = step(route, net, b1)
    for k in frozen:
      assert got[k] is None, ('P4 %s: %s frozen' % (route.name, name), k)
    assert_bitwise({k: v for k, v in got.items() if k not in frozen},
                   {k: v for k, v in g.items() if k not in frozen}, 'P4 %s: %s frozen' % (route.name, name))
  assert_bitwise(step(route, net, b1), g, 'P4 %s: thawed' % route.name)


# ---- P5
def differentiable_inputs(route, torch_route='torch'):
  assert route.general
  net, b1, _ = route.make()
  step(route, net, b1)                                   # (the batch is one the HIP route serves)
  truth, truth_in = route.truth(net, b1, loss_of(net, route.label(b1)), inputs=True)
  names = [k for k, _ in net.named_parameters()]
  said = []
  for wrt in (('node_feat',), ('D', 'V'), ('node_feat', 'D', 'V')):
    for frozen in (False, True):
      tag = 'P5 %s: %s require grad%s' % (route.name, ', '.join(wrt), ', every parameter frozen' if frozen else '')
      leaves = {k: route.inputs(b1)[k].detach().clone().requires_grad_(True) for k in wrt}
      b = route.with_inputs(b1, **leaves)
      with _frozen(net, names if frozen else []), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        net.zero_grad(set_to_none=True)
        score = route.forward(net, b)
        assert net.last_route == torch_route, (tag, net.last_route)
        assert score.requires_grad and score.grad_fn is not None, tag
        loss_of(net, route.label(b))(score).backward()
        g = grads_of(net)
      said += [w for w in rec if 'require grad' in str(w.message)]
      for k in wrt:
        assert truth_in[k] is not None and float(truth_in[k].abs().max()) > 0, (tag, k)
        e = rel_err(leaves[k].grad.cpu().numpy(), truth_in[k].cpu().numpy())
        print('%s: d loss / d %s vs float64 %.2e' % (tag, k, e))
        assert e < 1e-5, (tag, k, e)
      if frozen:
        assert all(v is None for v in g.values()), tag
      else:
        route.assert_bar(g, truth, tag)
  assert len(said) == 1 and all(k in str(said[0].message) for k in ('node_feat',)), [str(w.message) for w in said]
  step(route, net, b1)                                   # detached inputs: the HIP route again


# ---- P6
def inference_between(route):
  net, b1, b2 = route.make()
  g = step(route, net, b1)
  net.zero_grad(set_to_none=True)
  score = route.forward(net, b1)
  route.check_forward(net)
  loss = loss_of(net, route.label(b1))(score)
  with torch.no_grad():
    other = route.forward(net, b2)
  assert not other.requires_grad and net.last_route != route.hip_route
  loss.backward()
  route.check_backward(net)
  assert_bitwise(grads_of(net), g, 'P6 %s' % route.name)


# ---- P7
def double_backward_raises(route):
  net, b1, _ = route.make()
  net.zero_grad(set_to_none=True)
  score = route.forward(net, b1)
  route.check_forward(net)
  loss = loss_of(net, route.label(b1))(score)
  params = [p for p in net.parameters() if p.requires_grad]
  first = torch.autograd.grad(loss, params, create_graph=True, allow_unused=True)
  assert any(g is not None for g in first)
  with pytest.raises(RuntimeError, match='once_differentiable'):
    # (`backward()`, not `autograd.grad(.., params)`: the error node hangs on detached leaves, which a
    # differentiation towards the parameters alone would prune as unused without running it)
    sum(g.sum() for g in first if g is not None).backward()
