"""CPU-only: the two pack images of the compact spectral-gains MLP (csrc/gains_body.hpp:
compact_source, the one function both packers' kernels call, exported for the host as
lnz_spectral_mlp_pack_source) against a numpy restatement of their index maps, and the order in
which the 4x4x1 last layer takes the k's against the padded form's accumulator chains."""
import numpy as np
import pytest

from gains_compact_worker import OFF_W0C, OFF_W6C, PACK_SIZE, compact_images, rev3


def _lib():
  from lanczosnet_amd import _lib
  return _lib.load()


def _source_image(lib, W0, W6, S):
  out = np.zeros(PACK_SIZE - OFF_W0C, np.float32)
  for f in range(OFF_W0C, PACK_SIZE):
    src = lib.lnz_spectral_mlp_pack_source(S, f)
    assert src >= -1, (S, f, src)
    if src >= 1 << 32:
      out[f - OFF_W0C] = W6.reshape(-1)[src - (1 << 32)]
    elif src >= 0:
      out[f - OFF_W0C] = W0.reshape(-1)[src]
  return out


def test_the_pack_grew_behind_the_slack_only():
  lib = _lib()
  for S in (1, 8, 16):
    assert lib.lnz_spectral_mlp_pack_size(S) == PACK_SIZE
  for f in (0, OFF_W0C - 1, PACK_SIZE, -1):
    assert lib.lnz_spectral_mlp_pack_source(8, f) == -2, f
  assert lib.lnz_spectral_mlp_pack_source(17, OFF_W0C) == -2
  assert PACK_SIZE - OFF_W0C == 1024 + 2048 and OFF_W0C % 4 == 0


@pytest.mark.parametrize('S', [1, 2, 3, 4, 5, 7, 8, 9, 12, 16])
def test_compact_images_follow_their_index_maps(S):
  """distinct integers as weights, so a wrong source index cannot hide"""
  lib = _lib()
  W0 = (1 + np.arange(128 * S, dtype=np.float32)).reshape(128, S)
  W6 = -(1 + np.arange(S * 128, dtype=np.float32)).reshape(S, 128)
  got, want = _source_image(lib, W0, W6, S), compact_images(W0, W6, S)
  assert got.tobytes() == want.tobytes()
  # every weight of W6 appears exactly once; of W0 exactly once up to S = 8 (the image's reach)
  assert sorted(-got[OFF_W6C - OFF_W0C:][got[OFF_W6C - OFF_W0C:] != 0]) == list(1 + np.arange(S * 128))
  w0 = got[:OFF_W6C - OFF_W0C]
  assert sorted(w0[w0 != 0]) == sorted(W0[:, :8].reshape(-1))


def test_the_last_layer_takes_the_ks_in_the_padded_chains_order():
  """Padded form, stream step q of dense_tile: MFMA u (.x .y .z .w = 0..3) multiplies column
  8 q + u on lanes 0..31 and 8 q + 4 + u on lanes 32..63 (lnz_pack_rows_k8), the lower lanes' k
  first; chain acc takes u = 0, 2 and chain acc1 u = 1, 3.  Compact form: register v = q >> 1 of
  the W6c image, broadcast block abid = 8 (q & 1) + j; acc takes j = 0..3, acc1 j = 4..7."""
  W6 = (1 + np.arange(128, dtype=np.float32)).reshape(1, 128)
  img = compact_images(np.zeros((128, 1), np.float32), W6, 1)[OFF_W6C - OFF_W0C:].reshape(4, 8, 64)
  for q in range(16):
    padded = {'acc': [8 * q + 4 * hh + u for u in (0, 2) for hh in (0, 1)],
              'acc1': [8 * q + 4 * hh + u for u in (1, 3) for hh in (0, 1)]}
    compact = {'acc': [int(img[0, q >> 1, 4 * (8 * (q & 1) + j)]) - 1 for j in range(0, 4)],
               'acc1': [int(img[0, q >> 1, 4 * (8 * (q & 1) + j)]) - 1 for j in range(4, 8)]}
    assert compact == padded, q
  assert [rev3(j) for j in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
