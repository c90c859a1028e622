"""Host side of the opt-in HIP backward for TYPED edge-list batches (`_LargeSparseFusedFunction` on R = channels
operators, lnz_large_sparse_conv_split_f32, lnz_large_grad_input_channels): the route
`'large_typed_train_hip'` and its envelope, asked of `_LanczosNetBase._route` with no GPU; the new entries in the
header, the bindings and the library; the preconditions of the exact kernel cases
(tests/large_typed_train_fixture.py)."""
import itertools
import os
import re

import pytest

from test_route_cpu import G, Q, _module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = (True, False, False)          # (needs_grad, drop, capturing)
ON = dict(large_typed_backward_impl='hip', large_backward_impl='torch', large_split_planes=3, large_sparse=True)
ROUTE = 'large_typed_train_hip'


def _typed(name, channels, over=None, switches=None):
  """The module for `channels` operator channels (channels - 1 edge / bond types)."""
  over = dict(over or {}, num_bond_type=channels - 1)
  if name == Q:
    over = dict(dict(hidden_dim=[128] * 7, num_layer=7), **over)
  return _module(name, over, dict(ON, **(switches or {})))


def test_the_switch_defaults_to_the_torch_route():
  from lanczosnet_amd.model import _large
  src = open(_large.__file__).read()
  assert "large_typed_backward_impl = os.environ.get('LANCZOSNET_LARGE_BACKWARD_TYPED', 'torch')" in src
  if 'LANCZOSNET_LARGE_BACKWARD_TYPED' not in os.environ:
    assert _large._LargeMixin.large_typed_backward_impl == 'torch'


def test_route_is_taken_inside_the_envelope():
  for name, channels in itertools.product((G, Q), (3, 8)):
    net = _typed(name, channels)
    assert net.num_edgetype + 1 == channels
    for N, K in itertools.product((193, 2048, 2740, 16384), (1, 20, 64)):
      assert net._route(N, K, channels, *TRAIN, sparse_typed_operators=True) == ROUTE, (name, channels, N, K)
  from lanczosnet_amd.model import lanczos_net
  from test_large_train_cpu import one_function_serves_the_large_routes
  one_function_serves_the_large_routes()
  operand_description_of_a_typed_edge_list_batch()
  assert ROUTE in lanczos_net._LanczosNetBase._route.__doc__


def operand_description_of_a_typed_edge_list_batch():
  """One operator per channel: R = channels = 3 .. 8, the batch's images and node counts."""
  import torch
  from lanczosnet_amd import ops
  from lanczosnet_amd.model._large import _SparseOperators
  from test_large_train_cpu import host_image
  n = torch.tensor([300, 7], dtype=torch.int32)
  for channels in (3, 8):
    imgs = host_image(2, 300, R=channels)
    sl = ops.SparseLaplacian(2, 300, n, imgs.channel(0), None, None, channels=channels,
                             edge_type=torch.zeros(0, dtype=torch.int32), images=imgs)
    op = _SparseOperators(sl)
    assert (op.B, op.N, op.channels, op.R) == (2, 300, channels, channels)
    assert op.img is imgs and op.n_nodes is n
  novals = host_image(2, 300, R=3, values=False)
  with pytest.raises(AssertionError):
    _SparseOperators(ops.SparseLaplacian(2, 300, n, novals.channel(0), None, None, channels=3, images=novals))


@pytest.mark.parametrize('case,over,switches,call', [
    ('not clean typed images', {}, {}, dict(typed=False)),
    ('the default keyword', {}, {}, dict(typed=None)),
    ('two channels', {}, {}, dict(channels=2)),
    ('nine channels', {}, {}, dict(channels=9)),
    ('K = 65', {}, {}, dict(K=65)),
    ('dropout in training', dict(dropout=0.5), {}, dict(flags=(True, True, False))),
    ('capture in progress', {}, {}, dict(flags=(True, False, True))),
    ('no gradients', {}, {}, dict(flags=(False, False, False))),
    ('large_typed_backward_impl torch', {}, dict(large_typed_backward_impl='torch'), {}),
    ('backward_impl torch', {}, dict(backward_impl='torch'), {}),
    ('bf16 mode', {}, dict(gemm_mode='bf16'), {}),
    ('one-plane mode', {}, dict(large_split_planes=1), {}),
    ('sparse layers off', {}, dict(large_sparse=False), {}),
    ('hidden width 64', dict(hidden_dim=[64] * 7), {}, {}),
    ('input width 129', dict(input_dim=129), {}, {}),
    ('short scales', dict(short_diffusion_dist=[1, 2]), {}, {}),
    ('seventeen long scales', dict(long_diffusion_dist=list(range(1, 18))), {}, {}),
    ('a channel order', {}, dict(_channel_order=lambda: [1, 0]), {}),
    ('dense filters', {}, dict(filter_kind=1), {}),
])
def test_outside_the_envelope_the_answer_is_todays(case, over, switches, call):
  call = dict(dict(typed=True, flags=TRAIN, K=20, channels=3), **call)
  C = call['channels']
  net = _typed(G, C, over, switches)
  off = _typed(G, C, over, dict(switches, large_typed_backward_impl='torch'))
  for N in (193, 2048, 2740):
    kw = {} if call['typed'] is None else dict(sparse_typed_operators=call['typed'])
    got = net._route(N, call['K'], C, *call['flags'], **kw)
    assert got != ROUTE, case
    assert got == off._route(N, call['K'], C, *call['flags']), case
    if call['flags'][0] or call['flags'][1]:
      assert got == 'torch', case


def test_the_default_keyword_reproduces_every_answer_over_a_grid():
  """The grid of tests/test_large_train_cpu.py with the typed switch on (and, in a second pass, both)."""
  from test_large_train_cpu import _todays_route
  seen = set()
  for both in (False, True):
    on = dict(ON, large_backward_impl='hip') if both else ON
    nets = [_module(G, {}, on), _module(G, {}, dict(on, mid_backward_impl='hip')),
            _module(G, dict(dropout=0.5), on), _module(G, dict(hidden_dim=[96] * 7), on),
            _module(Q, {}, on), _module(G, dict(long_diffusion_dist=list(range(1, 18))), on),
            _module(G, {}, dict(on, backward_impl='torch'))]
    for net in nets:
      for N, K, C in itertools.product((9, 32, 33, 128, 129, 192, 193, 2048, 4104), (1, 20, 32, 33, 64, 65),
                                       (1, 2, 3, 8, 9)):
        for needs_grad, training, capturing in itertools.product((False, True), repeat=3):
          drop = training and net.dropout > 0.0
          want = _todays_route(net, N, K, C, needs_grad, drop, capturing)
          assert net._route(N, K, C, needs_grad, drop, capturing) == want
          assert net._route(N, K, C, needs_grad, drop, capturing, sparse_typed_operators=False) == want
          seen.add(want)
  assert seen == {'fused', 'fused_train_hip', 'fused_train_torch', 'mid', 'mid_train_hip', 'large_hip',
                  'library', 'torch'}


def test_each_switch_governs_its_own_kind_of_batch():
  typed_on = _typed(G, 3)
  assert typed_on._route(300, 20, 2, *TRAIN, sparse_one_operator=True) == 'torch'
  untyped_on = _typed(G, 3, switches=dict(large_backward_impl='hip', large_typed_backward_impl='torch'))
  assert untyped_on._route(300, 20, 3, *TRAIN, sparse_typed_operators=True) == 'torch'
  # the factored envelope leaves `_large_backward_supported` its answers
  for sw in ({}, dict(large_backward_impl='hip'), dict(large_backward_impl='hip', gemm_mode='bf16'),
             dict(large_backward_impl='hip', backward_impl='torch'), dict(large_backward_impl='hip', large_sparse=False)):
    net = _module(G, {}, dict(ON, **sw))
    want = (net.large_backward_impl == 'hip' and net.backward_impl == 'hip' and net._large_hip_supported(20, 2)
            and net.gemm_mode != 'bf16' and net.large_split_planes != 1 and net.large_sparse
            and net._channel_order() is None and net.filter_kind == 0)
    assert net._large_backward_supported(20, 2) == want, sw


def test_forward_asks_the_flag_word_only_where_it_can_matter():
  """`_sparse_typed_operators` answers False for a dense L, an untyped batch and every switch position outside
  the envelope WITHOUT touching the images (host objects stand in for them: a read would raise)."""
  import torch
  from lanczosnet_amd import ops

  class NoRead(object):
    values = object()

    @property
    def flags(self):
      raise AssertionError('the flag word was read')

  def batch(**kw):
    sl = ops.SparseLaplacian(2, 300, torch.zeros(2, dtype=torch.int32), NoRead(), None, None, channels=3,
                             images=NoRead())
    for k, v in kw.items():
      setattr(sl, k, v)
    return sl
  net = _typed(G, 3).train()
  assert net._sparse_typed_operators(torch.zeros(2, 300, 300, 3), False, False) is False
  assert net._sparse_typed_operators(batch(images=None, channels=2), False, False) is False   # untyped
  assert net._sparse_typed_operators(batch(channels=2), False, False) is False
  assert net._sparse_typed_operators(batch(channels=9), False, False) is False
  assert net._sparse_typed_operators(batch(N=65537), False, False) is False
  assert net._sparse_typed_operators(batch(), True, False) is False      # dropout
  assert net._sparse_typed_operators(batch(), False, True) is False      # capture
  with torch.no_grad():
    assert net._sparse_typed_operators(batch(), False, False) is False
  for sw in (dict(large_typed_backward_impl='torch'), dict(gemm_mode='bf16'), dict(backward_impl='torch'),
             dict(large_split_planes=1), dict(large_sparse=False), dict(filter_kind=1),
             dict(large_typed_backward_impl='torch', large_backward_impl='hip')):
    assert _typed(G, 3, switches=sw).train()._sparse_typed_operators(batch(), False, False) is False
  novals = batch()
  novals.images = type('NoValues', (NoRead,), dict(values=None))()
  assert net._sparse_typed_operators(novals, False, False) is False
  with pytest.raises(AssertionError, match='flag word was read'):
    net._sparse_typed_operators(batch(), False, False)
  # the untyped predicate does not read a typed batch's flag word either
  assert _typed(G, 3, switches=dict(large_backward_impl='hip')).train()._sparse_one_operator(batch(), False, False) \
      is False


def test_header_bindings_and_library_carry_the_new_entries():
  from lanczosnet_amd import _lib
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  log = hdr.split('#define LNZ_ABI_VERSION')[0]
  lib = _lib.load()
  assert lib.lnz_abi_version() == 7
  for name in ('lnz_large_sparse_conv_split_f32', 'lnz_large_grad_input_channels'):
    assert name in log, 'not in the change log'
    assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SIGNATURES
    assert hasattr(lib, name)
  inc = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'torch_ext_abi.inc')).read()
  assert 'raw_large_sparse_conv_split_f32' in inc and 'raw_large_grad_input_channels' in inc
  src = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'conv_sparse_grad.hip')).read()
  assert 'atomic' not in src.split('namespace {', 1)[1]
  # ONE gather kernel: the split gather is a mode of it
  gather = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'conv_sparse.hip')).read()
  assert len(re.findall(r'__global__[^;{]*\bsparse_\w*(?:gather|conv)\w*kernel\(', gather)) == 1
  # argument checks answer on the host, before any launch
  import ctypes as C
  null, one, two = C.c_void_p(0), C.c_void_p(64), C.c_void_p(1 << 30)
  split, inp = lib.lnz_large_sparse_conv_split_f32, lib.lnz_large_grad_input_channels
  assert split(null, null, null, 32, null, 1, 8, 3, null, null) == _lib.LNZ_EINVAL
  assert split(one, null, one, 32, one, 1, 8, 3, two, null) == _lib.LNZ_EINVAL          # no values
  for R in (1, 9):
    assert split(one, one, one, 32, one, 1, 8, R, two, null) == _lib.LNZ_ENOTSUP
  assert split(one, one, one, 36, one, 1, 8, 3, two, null) == _lib.LNZ_EINVAL           # row_cap
  assert split(one, one, one, 32, one, 1, 65537, 3, two, null) == _lib.LNZ_ENOTSUP      # 16-bit columns
  assert split(one, one, one, 32, C.c_void_p(68), 1, 8, 3, two, null) == _lib.LNZ_EINVAL   # alignment
  assert inp(null, null, null, null, 1, 8, 4, 3, 8, null, null) == _lib.LNZ_EINVAL
  for R, K, d in ((0, 4, 8), (9, 4, 8), (3, 65, 8), (3, 4, 129)):
    assert inp(one, one, one, one, 1, 8, K, R, d, two, null) == _lib.LNZ_ENOTSUP, (R, K, d)
  assert inp(one, one, one, one, 1, 8, 4, 3, 8, one, null) == _lib.LNZ_EINVAL           # dX aliases dZ
  # ... or any later channel of it: channel 2 of [3][1][8][128] floats starts 8192 bytes in
  assert inp(one, one, one, one, 1, 8, 4, 3, 8, C.c_void_p(64 + 8192), null) == _lib.LNZ_EINVAL
  assert inp(one, one, null, null, 1, 8, 4, 3, 8, two, null) == _lib.LNZ_EINVAL         # K > 0 needs V and dY


def test_exact_kernel_cases_meet_their_preconditions():
  import large_typed_train_fixture as F
  worst = F.all_exact_cases()
  print('worst |partial sum| bound over the exact cases: %g (limit %g)' % (worst, F.EXACT_LIMIT))
  assert 0 < worst < F.EXACT_LIMIT
  assert [s for s in F.INPUT_SHAPES if s[2] == 0] and {s[3] for s in F.INPUT_SHAPES} >= {3, 8}


def test_typed_gather_batches_are_what_they_claim():
  import edge_graphs as eg
  import large_typed_train_fixture as F
  for name in F.GATHER_CASES:
    graphs, N, E = F.gather_case(name)
    cap = eg.conv_cap(N)
    cnt = [F.channel_row_entries(g, E) for g in graphs if g['n'] > 0]
    assert max(int(c.max()) for c in cnt) <= cap, name
    for c in cnt:     # the typed channels partition the neighbours
      assert ((c[1:] - 1).sum(axis=0) == c[0] - 1).all()
    if name == 'n301 E2':
      assert graphs[-1]['n'] == 0 and N % 8 != 0
      assert {1, 8, 9, cap} <= set(cnt[0][0].tolist())
    if name == 'B10 E7':
      assert len(graphs) == 10 and E + 1 == 8
      assert np_mean([float((c[1:] == 1).mean()) for c in cnt]) > 0.3    # single-entry rows abound
    if name == 'n2100 E2':
      assert cap == 72 and int(cnt[0][0].max()) == 72


def np_mean(x):
  return sum(x) / len(x)
