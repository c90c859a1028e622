"""Host side of the opt-in HIP backward for edge-list batches (`_LargeSparseFusedFunction`,
csrc/conv_sparse_grad.hip): the route `'large_train_hip'` and its envelope, asked of
`_LanczosNetBase._route` with no GPU; the new entries in the header, the bindings and the library; the
preconditions of the exact kernel cases (tests/large_train_fixture.py)."""
import itertools
import os
import re

import pytest

from test_route_cpu import CASES, G, Q, _module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = (True, False, False)          # (needs_grad, drop, capturing)
ON = dict(large_backward_impl='hip', large_split_planes=3, large_sparse=True)
ROUTE = 'large_train_hip'


def test_the_switch_defaults_to_the_torch_route():
  from lanczosnet_amd.model import _large
  src = open(_large.__file__).read()
  assert "large_backward_impl = os.environ.get('LANCZOSNET_LARGE_BACKWARD', 'torch')" in src
  if 'LANCZOSNET_LARGE_BACKWARD' not in os.environ:
    assert _large._LargeMixin.large_backward_impl == 'torch'


def test_route_is_taken_inside_the_envelope():
  for name in (G, Q):
    over = {} if name == G else dict(num_bond_type=1, hidden_dim=[128] * 7, num_layer=7)
    net = _module(name, over, ON)
    for N, K in ((193, 20), (2048, 64), (4104, 20), (16384, 1), (33, 20)):
      assert net._route(N, K, 2, *TRAIN, sparse_one_operator=True) == ROUTE, (name, N, K)
  # the route is one of the functions `forward` trains through
  from lanczosnet_amd.model import lanczos_net
  one_function_serves_the_large_routes()
  operand_description_of_an_untyped_edge_list_batch()
  assert ROUTE in lanczos_net._LanczosNetBase._route.__doc__


LARGE_TRAIN_ROUTES = ('large_train_hip', 'large_typed_train_hip', 'large_dense_train_hip',
                      'large_dense_channels_train_hip')


def one_function_serves_the_large_routes():
  """Each of the four large training routes maps to the ONE Function; the names it replaced are gone."""
  from lanczosnet_amd.model import _large, lanczos_net
  for route in LARGE_TRAIN_ROUTES:
    assert lanczos_net._TRAIN_FUNCTIONS[route] is _large._LargeSparseFusedFunction, route
  for gone in ('_LargeTypedSparseFusedFunction', '_DenseBatch'):
    assert not hasattr(_large, gone) and not hasattr(lanczos_net, gone), gone


def host_image(B, N, R=None, cap=32, values=True):
  """A LargeSparseImage (R None) or the LargeSparseImages of R channels, of host tensors: no GPU to describe it."""
  import torch
  from lanczosnet_amd import ops
  lead = (B, N) if R is None else (R, B, N)
  cls = ops.LargeSparseImage if R is None else ops.LargeSparseImages
  return cls(torch.zeros(lead + (cap,), dtype=torch.int32), torch.zeros(lead, dtype=torch.int32),
             torch.zeros((1,), dtype=torch.int32), cap, torch.zeros(lead + (cap,)) if values else None)


def operand_description_of_an_untyped_edge_list_batch():
  """One operator serving the two channels: R = 1, channels = 2, the batch's image and node counts."""
  import torch
  from lanczosnet_amd import ops
  from lanczosnet_amd.model._large import _SparseOperators
  n = torch.tensor([300, 7], dtype=torch.int32)
  sl = ops.SparseLaplacian(2, 300, n, host_image(2, 300), None, None)
  op = _SparseOperators(sl)
  assert (op.B, op.N, op.channels, op.R) == (2, 300, 2, 1)
  assert op.img is sl.image and op.n_nodes is n
  with pytest.raises(AssertionError):
    _SparseOperators(ops.SparseLaplacian(2, 300, n, host_image(2, 300, values=False), None, None))


@pytest.mark.parametrize('case,over,switches,call', [
    ('not a clean one-operator image', {}, {}, dict(sparse_one_operator=False)),
    ('the default keyword', {}, {}, dict(sparse_one_operator=None)),
    ('no gradients', {}, {}, dict(flags=(False, False, False))),
    ('dropout in training', dict(dropout=0.5), {}, dict(flags=(True, True, False))),
    ('capture in progress', {}, {}, dict(flags=(True, False, True))),
    ('large_backward_impl torch', {}, dict(large_backward_impl='torch'), {}),
    ('backward_impl torch', {}, dict(backward_impl='torch'), {}),
    ('bf16 mode', {}, dict(gemm_mode='bf16'), {}),
    ('one-plane mode', {}, dict(large_split_planes=1), {}),
    ('sparse layers off', {}, dict(large_sparse=False), {}),
    ('hidden width 64', dict(hidden_dim=[64] * 7), {}, {}),
    ('input width 129', dict(input_dim=129), {}, {}),
    ('short scales', dict(short_diffusion_dist=[1, 2]), {}, {}),
    ('seventeen long scales', dict(long_diffusion_dist=list(range(1, 18))), {}, {}),
    ('K = 65', {}, {}, dict(K=65)),
    ('a channel order', {}, dict(_channel_order=lambda: [1, 0]), {}),
    ('dense filters', {}, dict(filter_kind=1), {}),
])
def test_outside_the_envelope_the_answer_is_todays(case, over, switches, call):
  call = dict(dict(sparse_one_operator=True, flags=TRAIN, K=20), **call)
  net = _module(G, over, dict(ON, **switches))
  off = _module(G, over, dict(ON, **dict(switches, large_backward_impl='torch')))
  for N in (193, 2048, 4104):
    kw = {} if call['sparse_one_operator'] is None else dict(sparse_one_operator=call['sparse_one_operator'])
    got = net._route(N, call['K'], 2, *call['flags'], **kw)
    assert got != ROUTE, case
    assert got == off._route(N, call['K'], 2, *call['flags']), case
    if call['flags'][0] or call['flags'][1]:
      assert got == 'torch', case


def _todays_route(net, N, K, C, needs_grad, drop, capturing):
  """The chain `_route` had before the keyword existed (tests/test_route_cpu.py's header), from the predicates."""
  fused = net._fused_supported() and net._fused_channels_ok()
  if N <= 32 and fused and not drop:
    if not needs_grad:
      return 'fused'
    return 'fused_train_hip' if net._fused_backward_supported() else 'fused_train_torch'
  if not drop and needs_grad and net._mid_backward_supported(N, K, C) and not capturing:
    return 'mid_train_hip'
  if needs_grad or drop:
    return 'torch'
  if net._mid_hip_supported(N, K, C):
    return 'mid'
  if N > 32 and net._large_hip_supported(K, C):
    return 'large_hip'
  return 'library'


def test_the_default_keyword_reproduces_every_answer_over_a_grid():
  nets = [_module(G, {}, ON), _module(G, {}, dict(ON, mid_backward_impl='hip')),
          _module(G, dict(dropout=0.5), ON), _module(G, dict(hidden_dim=[96] * 7), ON),
          _module(Q, {}, ON), _module(G, dict(long_diffusion_dist=list(range(1, 18))), ON),
          _module(G, {}, dict(ON, backward_impl='torch'))]
  seen = set()
  for net in nets:
    for N, K, C in itertools.product((9, 32, 33, 128, 129, 192, 193, 2048, 4104), (1, 20, 32, 33, 64, 65),
                                     (1, 2, 3, 8, 9)):
      for needs_grad, training, capturing in itertools.product((False, True), repeat=3):
        drop = training and net.dropout > 0.0
        want = _todays_route(net, N, K, C, needs_grad, drop, capturing)
        assert net._route(N, K, C, needs_grad, drop, capturing) == want
        assert net._route(N, K, C, needs_grad, drop, capturing, sparse_one_operator=False) == want
        seen.add(want)
  assert seen == {'fused', 'fused_train_hip', 'fused_train_torch', 'mid', 'mid_train_hip', 'large_hip',
                  'library', 'torch'}


@pytest.mark.parametrize('name,over,switches,N,K,C,flags,want', CASES)
def test_the_route_table_is_unchanged_with_the_switch_on(name, over, switches, N, K, C, flags, want):
  assert _module(name, over, dict(ON, **switches))._route(N, K, C, *flags) == want


def test_forward_asks_the_image_only_where_it_can_matter():
  """`_sparse_one_operator` answers False for a dense L, a typed batch and every switch position outside
  the envelope WITHOUT touching the image (host objects stand in for it: a read would raise)."""
  import torch
  from lanczosnet_amd import ops

  class NoRead(object):
    values = object()

    @property
    def flags(self):
      raise AssertionError('the flag word was read')

  def batch(**kw):
    sl = ops.SparseLaplacian(2, 300, torch.zeros(2, dtype=torch.int32), NoRead(), None, None)
    for k, v in kw.items():
      setattr(sl, k, v)
    return sl
  net = _module(G, {}, ON).train()
  assert net._sparse_one_operator(torch.zeros(2, 300, 300, 2), False, False) is False
  assert net._sparse_one_operator(batch(images=object(), channels=3), False, False) is False
  assert net._sparse_one_operator(batch(), True, False) is False      # dropout
  assert net._sparse_one_operator(batch(), False, True) is False      # capture
  with torch.no_grad():
    assert net._sparse_one_operator(batch(), False, False) is False
  for sw in (dict(large_backward_impl='torch'), dict(gemm_mode='bf16'), dict(backward_impl='torch')):
    assert _module(G, {}, dict(ON, **sw)).train()._sparse_one_operator(batch(), False, False) is False
  with pytest.raises(AssertionError, match='flag word was read'):
    net._sparse_one_operator(batch(), False, False)


def test_header_bindings_and_library_carry_the_new_entries():
  from lanczosnet_amd import _lib
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  log = hdr.split('#define LNZ_ABI_VERSION')[0]
  lib = _lib.load()
  for name in ('lnz_large_grad_project', 'lnz_large_grad_spectral', 'lnz_large_grad_input'):
    assert name in log, 'not in the change log'
    assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SIGNATURES
    assert hasattr(lib, name)
  mk = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'Makefile')).read()
  assert 'conv_sparse_grad.hip' in mk
  src = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'conv_sparse_grad.hip')).read()
  assert '#include "wave.hpp"' in src and 'atomic' not in src.split('namespace {', 1)[1]
  # argument checks answer on the host, before any launch
  import ctypes as C
  null = C.c_void_p(0)
  assert lib.lnz_large_grad_project(null, null, null, null, 1, 8, 4, null, null, null, null) == _lib.LNZ_EINVAL
  one = C.c_void_p(16)
  assert lib.lnz_large_grad_project(one, one, one, null, 1, 8, 65, one, one, one, null) == _lib.LNZ_ENOTSUP
  assert lib.lnz_large_grad_spectral(one, one, 8, one, one, 8, 1, 4, 17, 8, null, one, one, null) == _lib.LNZ_ENOTSUP
  assert lib.lnz_large_grad_input(one, one, one, one, 1, 8, 4, 8, one, null) == _lib.LNZ_EINVAL   # dX aliases dZ
  assert lib.lnz_large_grad_input(one, one, one, one, 1, 8, 4, 129, C.c_void_p(32), null) == _lib.LNZ_ENOTSUP


def test_exact_kernel_cases_meet_their_preconditions():
  import large_train_fixture as F
  worst = F.all_exact_cases()
  print('worst |partial sum| bound over the exact cases: %g (limit %g)' % (worst, F.EXACT_LIMIT))
  assert 0 < worst < F.EXACT_LIMIT
  for B, N, K, S, d in F.GRAD_SHAPES:
    n = F.ragged_nodes(B, N)
    assert n[0] == N and (n[1:] < N).all() and (n[-1] + 1) % 32 == 0
