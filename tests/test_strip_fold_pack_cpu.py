"""Host side of the packed folded weights of the strip forward (lnz_pack_fold_weights,
lnz_forward_args.Wf): an additive change under ABI 7."""
import ctypes as C
import os
import re

from lanczosnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, 'include', 'lanczosnet_hip.h')).read()


def test_header_change_log_names_the_entry_point_and_the_version_stays():
  log = HDR[:HDR.index('#define LNZ_ABI_VERSION')]
  assert 'lnz_pack_fold_weights' in log and 'lnz_forward_args.Wf' in log
  assert re.search(r'#define LNZ_ABI_VERSION (\d+)', HDR).group(1) == '7' and _lib.ABI_VERSION == 7
  assert _lib.load().lnz_abi_version() == 7


def test_forward_args_carry_the_block_last():
  assert _lib.ForwardArgs._fields_[-1] == ('Wf', C.c_void_p)
  assert _lib.load().lnz_forward_args_size() == C.sizeof(_lib.ForwardArgs)
  assert _lib.ForwardArgs.Wf.offset + 8 == C.sizeof(_lib.ForwardArgs)
  assert not _lib.ForwardArgs().Wf          # zero-initialised: the in-register sum
  # ... and in the header: the last member of the struct
  body = HDR[HDR.index('typedef struct lnz_forward_args'):HDR.index('} lnz_forward_args;')]
  members = re.findall(r'(\w+)(?:\[\d+\])?;', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
  assert members[-1] == 'Wf' and members[-2] == 'rare_debug'


def test_size_query_agrees_with_the_layout():
  """Per layer dhid x din_l floats (one channel of that layer's conv pack), layers back to back, 2048
  floats of slack: independent of the number of folded channels (n_edge 3, 5, 7 share a shape)."""
  lib = _lib.load()
  for num_layer, din0, dhid in ((7, 64, 128), (1, 64, 128), (3, 128, 128)):
    per_layer = [dhid // 32 * (d // 8) * 64 * 4 for d in [din0] + [dhid] * (num_layer - 1)]
    assert lib.lnz_pack_fold_weights_size(num_layer, din0, dhid) == sum(per_layer) + 2048
  assert lib.lnz_pack_fold_weights_size(7, 64, 128) == 128 * 64 + 6 * 128 * 128 + 2048
  assert lib.lnz_pack_fold_weights_size(0, 64, 128) == 0 and lib.lnz_pack_fold_weights_size(17, 64, 128) == 0


def test_pack_entry_refuses_bad_arguments_before_any_launch():
  lib = _lib.load()
  w_off = (C.c_int64 * 16)()
  one = C.c_void_p(256)    # (never dereferenced: the checks come first)
  for args in ((None, w_off, 7, 64, 128, 0, 8, 7, one),      # no pack
               (one, w_off, 7, 64, 128, 0, 8, 2, one),       # no folded channel
               (one, w_off, 17, 64, 128, 0, 8, 7, one),      # more layers than w_off holds
               (one, w_off, 7, 60, 128, 0, 8, 7, one),       # input width not in 16-column steps
               (one, w_off, 7, 64, 128, 0, 8, 7, None)):     # no output
    assert lib.lnz_pack_fold_weights(*args, None) == _lib.LNZ_EINVAL, args
  w_off[1] = 6
  assert lib.lnz_pack_fold_weights(one, w_off, 7, 64, 128, 0, 8, 7, one, None) == _lib.LNZ_EINVAL
