"""lnz_laplacian_l4 and lnz_laplacian (csrc/laplacian.hip) against oracle.get_laplacian in float64, per
molecule and channel, at the seams of lnz_laplacian_l4's launcher — the LDS byte count, N N E % 4 and the
pointer's alignment that choose between laplacian_l4_kernel<staged> and <direct> — with the route asserted
through ops.last_kernel() in every row, for all seven kinds (+ L6 at alpha 0.3 and 1.0), on counts of 0, 1,
N, one in between, N + 3 (clamped) and -2, bond-count and weighted non-symmetric adjacencies, zero and
negative row sums of I + A, and padding filled with junk and with NaN.

Nearly every other GPU test hands the L of ops.laplacian_l4 to both the kernel under test and its
reference, so a wrong Laplacian cancels out of them; here the builders themselves are held.  The cases, the
reference and the bar |got - ref| <= 2^-23 |ref| + 2^-40 max |ref| are builder_cases.py's;
test_builder_cases_cpu.py shows without a GPU that every case takes the route its row claims and that the
kernels' arithmetic, emulated in numpy, meets the bar."""
import numpy as np
import pytest
import torch

import builder_cases as bc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _t(x):
  return torch.from_numpy(np.array(x)).to(DEV)   # (a copy: the shared cases are read-only)


def _same_bits(a, b):
  return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _l4(adjs, counts, route):
  from lanczosnet_amd import ops
  L = ops.laplacian_l4(adjs if torch.is_tensor(adjs) else _t(adjs), _t(counts))
  assert ops.last_kernel() == bc.l4_kernel_name(route), ops.last_kernel()
  return L.cpu().numpy()


def _kind(adjs, counts, kind, alpha=0.5):
  from lanczosnet_amd import ops
  L = ops.laplacian(_t(adjs), _t(counts), kind, alpha)
  assert ops.last_kernel() == bc.kind_kernel_name(kind), ops.last_kernel()
  return L.cpu().numpy()


@pytest.mark.parametrize('label', [bt.label for bt, _ in bc.l4_batches()])
def test_laplacian_l4_meets_the_bar_on_its_claimed_route(label):
  bt, route = [x for x in bc.l4_batches() if x[0].label == label][0]
  ref = bc.reference(bt.N, bt.E, bt.content)
  got = _l4(bt.adjs, bt.counts, route)
  worst, differ = bc.check_bar(got, ref, bt.counts, label, l4_rule=True)
  print('%s laplacian_l4_kernel<%s>: worst achieved/bar %.3f, %d elements differ from float32(ref)'
        % (label, route, worst, differ))
  # a count of N + 3 is clamped (the bits of n = N), one of -2 is 0
  assert _same_bits(got[4], got[2]) and not got[5].any() and not got[0].any()
  # kind 4 of lnz_laplacian: the same bits wherever every row sum of I + A is >= 0; for a negative one the
  # reference's NaN row and column against lnz_laplacian_l4's zeros (check_bar's l4_rule above)
  k4 = _kind(bt.adjs, bt.counts, 'L4')
  if bt.content == 'negative_sum':
    bc.check_bar(k4, ref, bt.counts, label + ' kind 4')
    r = bt.N // 2
    assert np.isnan(k4[2, r, :, :2]).all() and np.isnan(k4[2, :, r, :2]).all()
    assert not got[2, r, :, :2].any() and not got[2, :, r, :2].any() and not np.isnan(got).any()
  else:
    assert _same_bits(k4, got)
  # what lies in the padding is never read: finite junk and NaN give the bits of zero padding
  for fill in ('junk', 'nan'):
    padded = bc.with_padding(bt, fill)
    assert _same_bits(_l4(padded, bt.counts, route), got), fill
    assert np.array_equal(_kind(padded, bt.counts, 'L4'), k4, equal_nan=True), fill


@pytest.mark.parametrize('N,E', bc.UNALIGNED_SHAPES)
def test_an_unaligned_adjacency_takes_the_direct_kernel_and_gives_the_same_bits(N, E):
  """A contiguous view that starts one float into a flat buffer: no 16-byte loads, the same bits."""
  for content in bc.CONTENTS:
    bt = bc.batch(N, E, content)
    want = _l4(bt.adjs, bt.counts, 'staged')
    numel = bt.adjs.size
    buf = torch.full((numel + 5,), float('nan'), device=DEV)
    view = buf[1:1 + numel].view(bt.adjs.shape)
    view.copy_(_t(bt.adjs))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert _same_bits(_l4(view, bt.counts, 'direct'), want), content
    bc.check_bar(want, bc.reference(N, E, content), bt.counts, bt.label, l4_rule=True)


@pytest.mark.parametrize('kind,alpha', bc.KINDS)
def test_every_kind_meets_the_bar_at_a_staged_size_and_a_direct_size(kind, alpha):
  for bt in bc.kind_batches():
    ref = bc.reference(bt.N, bt.E, bt.content, kind, alpha)
    got = _kind(bt.adjs, bt.counts, kind, alpha)
    worst, differ = bc.check_bar(got, ref, bt.counts, (bt.label, kind, alpha))
    print('%s %s alpha %.1f laplacian_kind_kernel<%s>: worst achieved/bar %.3f, %d elements differ from float32(ref)'
          % (bt.label, kind, alpha, kind[1], worst, differ))
    assert _same_bits(got[4], got[2]) and not got[5].any() and not got[0].any()
    for fill in ('junk', 'nan'):
      assert _same_bits(_kind(bc.with_padding(bt, fill), bt.counts, kind, alpha), got), (bt.label, fill)


def test_degree_arrays_beyond_lds_are_refused_by_both_entry_points():
  from lanczosnet_amd import ops, _lib
  N, E = bc.REFUSED_SHAPE
  adjs = torch.zeros((1, N, N, E), device=DEV)
  n = torch.tensor([3], dtype=torch.int32, device=DEV)
  with pytest.raises(_lib.NotSupported):
    ops.laplacian_l4(adjs, n)
  with pytest.raises(_lib.NotSupported):
    ops.laplacian(adjs, n, 'L4')
  with pytest.raises(_lib.NotSupported):
    ops.laplacian(adjs, n, 'L1')
