"""Host side of the opt-in HIP backward for DENSE collated batches beyond 128 nodes (`large_dense_backward_impl`,
lnz_large_sparse_image_symmetry): the routes `'large_dense_train_hip'` and
`'large_dense_channels_train_hip'` and their envelope, asked of `_LanczosNetBase._route` with no GPU; the predicate
that decides them, asked where it must not look at the tensor; the new entry in the header, the bindings and the
library; the status rule's numpy restatement (tests/symmetry_mirror.py) on hand-made images."""
import itertools
import os
import re

import numpy as np
import pytest

import symmetry_mirror as SM
from test_large_train_cpu import _todays_route, host_image, one_function_serves_the_large_routes
from test_route_cpu import CASES, G, Q, _module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = (True, False, False)          # (needs_grad, drop, capturing)
ON = dict(large_dense_backward_impl='hip', large_backward_impl='torch', large_typed_backward_impl='torch',
          large_split_planes=3, large_sparse=True, large_sparse_channels='one')
ONE, EACH = 'large_dense_train_hip', 'large_dense_channels_train_hip'
NAME = 'lnz_large_sparse_image_symmetry'


def _net(name=G, channels=2, over=None, switches=None):
  over = dict(over or {}, num_bond_type=channels - 1)
  if name == Q:
    over = dict(dict(hidden_dim=[128] * 7, num_layer=7), **over)
  return _module(name, over, dict(ON, **(switches or {})))


def test_the_switch_defaults_to_the_torch_route():
  from lanczosnet_amd.model import _large
  src = open(_large.__file__).read()
  assert "large_dense_backward_impl = os.environ.get('LANCZOSNET_LARGE_BACKWARD_DENSE', 'torch')" in src
  if 'LANCZOSNET_LARGE_BACKWARD_DENSE' not in os.environ:
    assert _large._LargeMixin.large_dense_backward_impl == 'torch'


def test_the_default_keywords_reproduce_every_answer_over_a_grid():
  """The grid of tests/test_large_train_cpu.py with the dense switch on (and, in a second pass, all three)."""
  seen = set()
  for every in (False, True):
    on = dict(ON, large_backward_impl='hip', large_typed_backward_impl='hip', large_sparse_channels='each') \
        if every else ON
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
          assert net._route(N, K, C, needs_grad, drop, capturing, dense_one_operator=False,
                            dense_channel_operators=False) == want
          seen.add(want)
  assert seen == {'fused', 'fused_train_hip', 'fused_train_torch', 'mid', 'mid_train_hip', 'large_hip',
                  'library', 'torch'}


@pytest.mark.parametrize('name,over,switches,N,K,C,flags,want', CASES)
def test_the_route_table_is_unchanged_with_the_switch_on(name, over, switches, N, K, C, flags, want):
  assert _module(name, over, dict(ON, **switches))._route(N, K, C, *flags) == want


def test_the_keywords_are_keyword_only():
  net = _net()
  with pytest.raises(TypeError):
    net._route(300, 20, 2, *TRAIN, False, False, True)


def test_routes_are_taken_inside_the_envelope():
  from lanczosnet_amd.model import lanczos_net
  for name, C in itertools.product((G, Q), (1, 2, 3, 8)):
    net = _net(name, C)
    for N, K in itertools.product((129, 193, 2048, 16384), (1, 20, 64)):
      assert net._route(N, K, C, *TRAIN, dense_one_operator=True) == ONE, (name, C, N, K)
  for name, C in itertools.product((G, Q), (3, 8)):
    net = _net(name, C, switches=dict(large_sparse_channels='each'))
    for N, K in itertools.product((129, 2048), (1, 64)):
      assert net._route(N, K, C, *TRAIN, dense_channel_operators=True) == EACH, (name, C, N, K)
  one_function_serves_the_large_routes()
  operand_description_of_a_dense_tensor()
  doc = lanczos_net._LanczosNetBase._route.__doc__
  assert "'%s'" % ONE in doc and "'%s'" % EACH in doc


def operand_description_of_a_dense_tensor():
  """'one': R = 1 whatever the channel count, the image riding on the tensor; 'each': R = channels, the images
  riding on it; n_nodes is None in both.  An image that does not ride on THIS state of the tensor is refused."""
  import torch
  from lanczosnet_amd import ops
  from lanczosnet_amd.model._large import _SparseOperators
  for C in (1, 2, 3):
    L = torch.zeros(2, 130, 130, C)
    img = host_image(2, 130)
    ops.attach_sparse_image(L, img)
    op = _SparseOperators(L)
    assert (op.B, op.N, op.channels, op.R) == (2, 130, C, 1)
    assert op.img is img and op.n_nodes is None
  for C in (3, 8):
    L = torch.zeros(2, 130, 130, C)
    imgs = host_image(2, 130, R=C)
    ops.attach_sparse_images(L, imgs)
    op = _SparseOperators(L, each=True)
    assert (op.B, op.N, op.channels, op.R) == (2, 130, C, C)
    assert op.img is imgs and op.n_nodes is None
    with pytest.raises(AssertionError):
      _SparseOperators(L)                       # no single image rides on it
  L.add_(1.0)                                   # (the tensor changed: its images are stale)
  with pytest.raises(AssertionError):
    _SparseOperators(L, each=True)
  L = torch.zeros(2, 130, 130, 2)
  ops.attach_sparse_image(L, host_image(2, 130, values=False))
  with pytest.raises(AssertionError):
    _SparseOperators(L)


@pytest.mark.parametrize('case,over,switches,call', [
    ('neither keyword', {}, {}, dict(one=False, each=False)),
    ('N = 128', {}, {}, dict(Ns=(33, 100, 128))),
    ('N = 128, mid backward on', {}, dict(mid_backward_impl='hip'), dict(Ns=(33, 128))),
    ('no gradients', {}, {}, dict(flags=(False, False, False))),
    ('dropout in training', dict(dropout=0.5), {}, dict(flags=(True, True, False))),
    ('capture in progress', {}, {}, dict(flags=(True, False, True))),
    ('large_dense_backward_impl torch', {}, dict(large_dense_backward_impl='torch'), {}),
    ('only the other two switches', {}, dict(large_dense_backward_impl='torch', large_backward_impl='hip',
                                             large_typed_backward_impl='hip'), {}),
    ('backward_impl torch', {}, dict(backward_impl='torch'), {}),
    ('bf16 mode', {}, dict(gemm_mode='bf16'), {}),
    ('one-plane mode', {}, dict(large_split_planes=1), {}),
    ('sparse layers off', {}, dict(large_sparse=False), {}),
    ('hidden width 64', dict(hidden_dim=[64] * 7), {}, {}),
    ('input width 129', dict(input_dim=129), {}, {}),
    ('short scales', dict(short_diffusion_dist=[1, 2]), {}, {}),
    ('seventeen long scales', dict(long_diffusion_dist=list(range(1, 18))), {}, {}),
    ('K = 65', {}, {}, dict(K=65)),
    ('nine channels', {}, {}, dict(C=9)),
    ('a channel order', {}, dict(_channel_order=lambda: [1, 0]), {}),
    ('dense filters', {}, dict(filter_kind=1), {}),
    ("distinct channels under 'one'", {}, dict(large_sparse_channels='one'), dict(C=3, one=False)),
    ("two distinct channels under 'each'", {}, dict(large_sparse_channels='each'), dict(C=2, one=False)),
])
def test_outside_the_envelope_the_answer_is_todays(case, over, switches, call):
  call = dict(dict(one=True, each=True, flags=TRAIN, K=20, C=2, Ns=(129, 193, 2048, 4104)), **call)
  C = call['C']
  net = _net(G, C, over, switches)
  for N in call['Ns']:
    got = net._route(N, call['K'], C, *call['flags'], dense_one_operator=call['one'],
                     dense_channel_operators=call['each'])
    assert got not in (ONE, EACH), case
    assert got == _todays_route(net, N, call['K'], C, *call['flags']), case
    assert got == net._route(N, call['K'], C, *call['flags']), case


def test_each_switch_governs_its_own_kind_of_batch():
  dense_on = _net(G, 2)
  assert dense_on._route(300, 20, 2, *TRAIN, sparse_one_operator=True) == 'torch'
  assert _net(G, 3)._route(300, 20, 3, *TRAIN, sparse_typed_operators=True) == 'torch'
  old_on = _net(G, 2, switches=dict(large_dense_backward_impl='torch', large_backward_impl='hip',
                                    large_typed_backward_impl='hip', large_sparse_channels='each'))
  assert old_on._route(300, 20, 2, *TRAIN, dense_one_operator=True) == 'torch'
  assert old_on._route(300, 20, 2, *TRAIN, sparse_one_operator=True) == 'large_train_hip'


def test_the_predicate_looks_at_the_tensor_only_where_the_answer_can_matter(monkeypatch):
  """`_dense_operators` answers None for a SparseLaplacian and for every switch position outside the envelope
  WITHOUT touching the tensor: the stand-in's `.stride` raises, and so does every image read and launch."""
  import torch
  from lanczosnet_amd import ops

  class NoTouch(torch.Tensor):
    """(a float32 [2,300,300,2] tensor that claims to live on the device: no GPU is needed to ask)"""
    is_cuda = True

    def stride(self, *a):
      raise AssertionError('the tensor was touched')

  def boom(*a, **kw):
    raise AssertionError('the tensor was touched')
  for fn in ('attached_sparse_image', 'attached_sparse_images', 'large_sparse_image', 'large_sparse_image_channels',
             'large_sparse_image_symmetry'):
    monkeypatch.setattr(ops, fn, boom)

  def dense(N=300, C=2, dtype=torch.float32, cuda=True):
    t = torch.zeros(2, N, N, C, dtype=dtype).as_subclass(NoTouch)
    t.is_cuda = cuda
    return t
  net = _net(G, 2).train()
  sl = ops.SparseLaplacian(2, 300, torch.zeros(2, dtype=torch.int32), object(), None, None)
  assert net._dense_operators(sl, 20, False, False) is None
  assert net._dense_operators(dense(), 20, True, False) is None       # dropout
  assert net._dense_operators(dense(), 20, False, True) is None       # capture
  with torch.no_grad():
    assert net._dense_operators(dense(), 20, False, False) is None
  assert net._dense_operators(dense(N=128), 20, False, False) is None
  assert net._dense_operators(dense(N=33), 20, False, False) is None
  assert net._dense_operators(dense(), 65, False, False) is None
  assert net._dense_operators(dense(C=3), 20, False, False) is None   # not the model's channels
  assert net._dense_operators(dense(dtype=torch.float64), 20, False, False) is None
  assert net._dense_operators(dense(cuda=False), 20, False, False) is None
  for sw in (dict(large_dense_backward_impl='torch'), dict(gemm_mode='bf16'), dict(backward_impl='torch'),
             dict(large_split_planes=1), dict(large_sparse=False), dict(filter_kind=1),
             dict(large_dense_backward_impl='torch', large_backward_impl='hip', large_typed_backward_impl='hip')):
    assert _net(G, 2, switches=sw).train()._dense_operators(dense(), 20, False, False) is None, sw
  assert _net(G, 2, dict(dropout=0.5)).train()._dense_operators(dense(), 20, True, False) is None
  # inside the envelope the tensor IS asked
  with pytest.raises(AssertionError, match='the tensor was touched'):
    net._dense_operators(dense(), 20, False, False)
  # the two old predicates do not look at a dense tensor
  both = _net(G, 2, switches=dict(large_backward_impl='hip', large_typed_backward_impl='hip')).train()
  assert both._sparse_one_operator(dense(), False, False) is False
  assert both._sparse_typed_operators(dense(), False, False) is False


def test_header_bindings_and_library_carry_the_new_entry():
  from lanczosnet_amd import _lib
  hdr = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()
  log = hdr.split('#define LNZ_ABI_VERSION')[0]
  lib = _lib.load()
  assert lib.lnz_abi_version() == 7
  assert NAME in log, 'not in the change log'
  assert re.search(r'\bint %s\(' % NAME, hdr) and NAME in _lib.SIGNATURES
  assert hasattr(lib, NAME)
  inc = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'torch_ext_abi.inc')).read()
  assert 'raw_large_sparse_image_symmetry' in inc
  mk = open(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'Makefile')).read()
  assert 'sparse_symmetry.hip' in mk
  assert os.path.exists(os.path.join(ROOT, 'lanczosnet_amd', 'csrc', 'sparse_symmetry.hip'))


def test_argument_checks_answer_on_the_host():
  import ctypes as C
  from lanczosnet_amd import _lib
  sym = getattr(_lib.load(), NAME)
  null, one = C.c_void_p(0), C.c_void_p(64)
  assert sym(null, null, null, 32, 1, 1, 8, null, null) == _lib.LNZ_EINVAL
  assert sym(one, null, one, 32, 1, 1, 8, one, null) == _lib.LNZ_EINVAL          # values are required
  assert sym(one, one, null, 32, 1, 1, 8, one, null) == _lib.LNZ_EINVAL
  assert sym(one, one, one, 32, 1, 1, 8, null, null) == _lib.LNZ_EINVAL
  for R, B, N in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (-1, 1, 8)):
    assert sym(one, one, one, 32, R, B, N, one, null) == _lib.LNZ_EINVAL, (R, B, N)
  assert sym(one, one, one, 32, 9, 1, 8, one, null) == _lib.LNZ_ENOTSUP           # R <= 8
  assert sym(one, one, one, 32, 1, 1, 65537, one, null) == _lib.LNZ_ENOTSUP       # 16-bit columns
  for cap in (0, 24, 36, 31):
    assert sym(one, one, one, cap, 1, 1, 8, one, null) == _lib.LNZ_EINVAL, cap


# ---- the status rule, restated in numpy, on hand-made images -----------------------------------------------------
def _ring(B, N):
  """[B,N,N] float32: a weighted ring with a diagonal, symmetric bit for bit."""
  rs = np.random.RandomState(3)
  L = np.zeros((B, N, N), np.float32)
  for b in range(B):
    w = rs.rand(N).astype(np.float32) + 0.5
    i = np.arange(N)
    L[b, i, (i + 1) % N] = w
    L[b, (i + 1) % N, i] = w
    L[b, i, i] = rs.rand(N).astype(np.float32) + 0.1
  return L


def test_numpy_restatement_of_the_status_rule():
  B, N, cap = 3, 12, 32
  L = _ring(B, N)
  shuffled = lambda k: np.random.RandomState(k).permutation(k)   # noqa: E731  (entry order is NOT ascending)
  for order in (None, shuffled):
    assert SM.status_rule(*SM.image_of(L, cap, order), cap).tolist() == [0, 0, 0]
  # a missing mirror, in graph 1 only
  M = L.copy()
  M[1, 4, 5] = 0.0
  assert SM.status_rule(*SM.image_of(M, cap, shuffled), cap).tolist() == [0, 1, 0]
  # one ulp is accepted, two are not; the sign is part of the value
  M = L.copy()
  M[2, 5, 4] = np.nextafter(M[2, 5, 4], np.float32(9))
  assert SM.status_rule(*SM.image_of(M, cap), cap).tolist() == [0, 0, 0]
  M[2, 5, 4] = np.nextafter(M[2, 5, 4], np.float32(9))
  assert SM.status_rule(*SM.image_of(M, cap), cap).tolist() == [0, 0, 2]
  M = L.copy()
  M[0, N - 1, 0] = -M[0, N - 1, 0]                                # the defect at row n - 1
  M[0, 7, 8] = 0.0
  assert SM.status_rule(*SM.image_of(M, cap), cap).tolist() == [3, 0, 0]
  M = np.zeros((1, 4, 4), np.float32)
  M[0, 0, 1], M[0, 1, 0] = np.float32(1e-45), np.float32(-1e-45)  # one apart as numbers of ulps, opposite signs
  assert SM.status_rule(*SM.image_of(M, cap), cap).tolist() == [2]
  # a diagonal entry is its own mirror; the padding (column 0, value 0) and what lies beyond it are not entries
  M = np.zeros((1, 9, 9), np.float32)
  M[0, 3, 3] = 2.0
  ent, val, cnt = SM.image_of(M, cap)
  assert cnt[0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0] and (ent[0, 3, 1:8] == 0).all() and ent[0, 3, 8] != 0
  assert SM.status_rule(ent, val, cnt, cap).tolist() == [0]
  # the mirror must lie among the first counts[j] entries of row j
  ent, val, cnt = SM.image_of(L, cap)
  cnt[0, 5] -= 1
  assert SM.status_rule(ent, val, cnt, cap).tolist() == [1, 0, 0]
  # channel-major images land in their own words
  ent, val, cnt = SM.image_of(L, cap)
  R3 = [np.stack([x, x, x]) for x in (ent, val, cnt)]
  R3[1][2, 1, 0, :] = 0.0
  R3[0][2, 1, 0, :] = 0
  R3[2][2, 1, 0] = 0                                              # channel 2, graph 1: row 0 emptied
  assert SM.status_rule(*R3, cap).tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0]
  assert SM.within_one_ulp(1.0, np.nextafter(np.float32(1), np.float32(2)))
  assert not SM.within_one_ulp(0.0, -0.0) and SM.within_one_ulp(np.float32(0), np.float32(1e-45))
