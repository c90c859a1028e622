"""numpy restatement of lnz_large_sparse_image_symmetry's status rule (include/lanczosnet_hip.h; csrc/sparse_symmetry.hip),
written from the rule and not from the kernel: a dictionary of every row's entries, looked up entry by entry."""
import numpy as np


def within_one_ulp(a, b):
  """a, b float32 scalars: same sign and bit patterns, as integers, at most 1 apart."""
  ia, ib = int(np.float32(a).view(np.uint32)), int(np.float32(b).view(np.uint32))
  if (ia >> 31) != (ib >> 31):
    return False
  return abs((ia & 0x7fffffff) - (ib & 0x7fffffff)) <= 1


def status_rule(entries, values, counts, cap):
  """entries / values [..., B, N, cap], counts [..., B, N] (one image, or R channel-major images) -> status
  [R * B] int32: bit 0 = an entry (i, j, v), k < counts[i], without an entry of column i among the first counts[j]
  entries of row j; bit 1 = the mirror's value is not within one ulp of v.  The diagonal is its own mirror."""
  entries = np.asarray(entries).astype(np.int64) & 0xffffffff
  values = np.asarray(values, dtype=np.float32)
  counts = np.asarray(counts)
  B, N = counts.shape[-2:]
  ent = entries.reshape(-1, B, N, cap)
  val = values.reshape(-1, B, N, cap)
  cnt = np.clip(counts.reshape(-1, B, N), 0, cap)
  R = ent.shape[0]
  status = np.zeros((R * B,), np.int32)
  for r in range(R):
    for b in range(B):
      rows = []
      for i in range(N):
        d = {}
        for k in range(int(cnt[r, b, i])):
          d.setdefault(int(ent[r, b, i, k] & 0xffff), val[r, b, i, k])   # (the first of a column, as a search finds it)
        rows.append(d)
      for i in range(N):
        for k in range(int(cnt[r, b, i])):
          j, v = int(ent[r, b, i, k] & 0xffff), val[r, b, i, k]
          if j == i:
            continue
          if j >= N or i not in rows[j]:
            status[r * B + b] |= 1
          elif not within_one_ulp(v, rows[j][i]):
            status[r * B + b] |= 2
  return status


def image_of(dense, cap, order=None):
  """A hand-made image of dense [B, N, N] float32 on the host: entries (bf16 of the value truncated — the check
  never reads it — << 16 | column), values, counts; rows padded with (column 0, value 0) to a multiple of eight and
  garbage beyond.  order: a permutation applied to every row's entries (None: ascending columns)."""
  dense = np.asarray(dense, dtype=np.float32)
  B, N, _ = dense.shape
  ent = np.full((B, N, cap), 0x7fff0000 | (N - 1), np.int64)    # garbage beyond the padding: a live-looking entry
  val = np.full((B, N, cap), 123.0, np.float32)
  cnt = np.zeros((B, N), np.int32)
  for b in range(B):
    for i in range(N):
      cols = np.nonzero(dense[b, i])[0]
      if order is not None:
        cols = cols[order(len(cols))]
      assert len(cols) <= cap
      k = len(cols)
      cnt[b, i] = k
      ent[b, i, :k] = ((dense[b, i, cols].view(np.uint32).astype(np.int64) >> 16) << 16) | cols
      val[b, i, :k] = dense[b, i, cols]
      pad = (k + 7) // 8 * 8
      ent[b, i, k:pad] = 0
      val[b, i, k:pad] = 0.0
  return ent.astype(np.uint32).view(np.int32), val, cnt
