"""Matrix-core work the fused forward kernel ISSUES for a given tile plan (measurement helper, pure
numpy: used by bench.py's `roofline` and checked against `rocprofv3 --pmc
SQ_INSTS_VALU_MFMA_MOPS_F32` in tests/test_flop_model.py).

`lanczosnet_forward_kernel<4,*,0,0>` (csrc/conv_forward.hip, diagonal gains, eigen-space long
channels) runs 32-row node tiles; a tile's four wavefronts own 32 output columns each and issue, per
conv layer with input width d_in,

    GEMM1      (n_short + n_long + n_edge) * d_in / 2        X W_c^T, never skipped
    lift-back  4 * popcount(smask)                           V T, 8-slot groups that hold Ritz pairs
    GEMM2      (n_edge - n_ident) * 4 * popcount(g2mask)     M_c Z_c, 8-row groups that hold real
                                                             nodes; identity channels add Z instead
    projection 4 * popcount(g2mask)                          V^T X' for the next layer (not the last)

`v_mfma_f32_32x32x2_f32` instructions, plus the first layer's projection (waves whose 32 columns lie
inside din0) and the head (one wave per tile, dhid / 2 instructions).  g2mask / smask follow
`row_group_mask` (conv_forward.hip:139): molecule A fills groups from row 0, molecule B from the
split row.  One instruction = 2 * 32 * 32 * 2 = 4096 flop = 8 counts of the PMC counter (512 flop
per count).

`lanczosnet_forward16_kernel` (retired: the strip kernel took every launch it could take; its model
stays, pinned to the counter run profiles/r04_forward16_pmc.json) ran the same algebra on 32-row tiles
with `v_mfma_f32_16x16x4_f32`, 2048 flop = 4 counter units, eight waves of 16 output columns on every
tile of the workgroup, and issued per tile, wave and layer

    GEMM1      (n_long + n_edge) * d_in / 2                  (8 instructions per 16-k step)
    lift-back  8 * popcount(slot subtiles)                   16-row subtiles that hold Ritz pairs
    GEMM2      (n_edge - n_ident) * 8 * popcount(row subtiles)
    projection 8 * popcount(row subtiles)                    (not the last layer)

plus the first layer's projection (waves whose 16 columns lie inside din0) and the head (one wave per
tile, dhid / 2 instructions of the 32x32x2 kind).

`lanczosnet_strip_kernel` (csrc/conv_strip.hip: the inference forward on the strip plan of
lnz_plan_strips — S subtiles of 16 rows per workgroup, molecules at 4-row granularity) issues per
strip, wave and layer

    GEMM1      (n_long + n_edge) * d_in / 16 * 4 * S
    lift-back  4 * blocks                                    blocks = 3 S - 2: every subtile pair (I, J),
    GEMM2      4 * n_edge * blocks                           |I - J| <= 1 (branch free: a pair no molecule
    projection 4 * blocks      (not the last layer)          touches, or an identity channel's, has zero
                                                             fragments and is multiplied all the same)

plus the first layer's projection (din0 / 16 waves) and the head (S waves, 64 instructions), all of
the 16x16x4 kind.  It takes the launches `strips_selected` says.  (That is the channel loop over the edge
types: `strip_mfma_issued`.  The inference forward folds the rare bond-type channels where that is
cheaper, `lanczosnet_strip_kernel<0,0,1,false,false>`: `strip_rare_mfma_issued` below.)
"""
import numpy as np

FLOP_PER_MFMA = 2 * 32 * 32 * 2          # v_mfma_f32_32x32x2_f32
FLOP_PER_MFMA16 = 2 * 16 * 16 * 4        # v_mfma_f32_16x16x4_f32
FLOP_PER_MOPS_COUNT = 512                # SQ_INSTS_VALU_MFMA_MOPS_F32 unit


def _row_groups(n_a, n_b, split):
  ga = (n_a + 7) >> 3
  gb = ((n_b + 7) >> 3) if n_b > 0 else 0
  return ga + gb if split < 32 else ga   # B's groups start at split / 8: disjoint from A's


def _subtiles16(n_a, n_b, split):
  """16-row subtiles of a tile that hold a row of A (from row 0) or B (from the split row), as the
  retired 16 x 16-tile kernel skipped them."""
  mask = (1 << ((n_a + 7) >> 3)) - 1
  if split < 32 and n_b > 0:
    mask |= ((1 << ((n_b + 7) >> 3)) - 1) << (split >> 3)
  return (1 if mask & 3 else 0) + (1 if mask & 12 else 0)


def forward16_selected(cfg):
  """Is this LanczosNet model's shape one the 16 x 16-MFMA family takes (the strip kernel of
  csrc/conv_strip.hip, lnz::strip_forward_eligible), given a strip plan?  Without one the
  exact-fp32 inference forward runs on the 32 x 32 tiles of csrc/conv_forward.hip."""
  hid = cfg['hidden_dim']
  return (len(cfg['short_diffusion_dist']) == 0 and all(h == 128 for h in hid) and
          cfg['input_dim'] % 64 == 0 and cfg['input_dim'] <= 128 and
          len(cfg['long_diffusion_dist']) <= 12)


def tiles_from_plan(plan_entries, extents, ident=None, K=20):
  """plan_entries: int array [cap * 4, 3] (molecule A, molecule B | -1, split row) as written by
  lnz_plan_tiles; extents [B] = last real node + 1 per molecule; ident [B] = identity-channel
  bits of the edge channels (Lp.ident) or None.  Returns one dict per tile in use."""
  out = []
  pe = np.asarray(plan_entries).reshape(-1, 3)
  ext = np.asarray(extents)
  for ta, tb, split in pe:
    if ta < 0:
      continue
    n_a = int(ext[ta])
    n_b = int(ext[tb]) if tb >= 0 else 0
    idb = 0
    if ident is not None:
      idb = int(ident[ta]) & 0xffffffff
      if tb >= 0:
        idb &= int(ident[tb]) & 0xffffffff
    sp = int(split) if tb >= 0 else 32
    out.append(dict(nA=n_a, nB=n_b, split=sp, ident=idb,
                    pg=_row_groups(n_a, n_b, sp), ps=_row_groups(min(n_a, K), min(n_b, K), sp),
                    pg16=_subtiles16(n_a, n_b, sp), ps16=_subtiles16(min(n_a, K), min(n_b, K), sp)))
  return out


def forward_mfma_issued(tiles, cfg, nwv=4):
  """tiles: tiles_from_plan(...) output; cfg: model dict (input_dim, hidden_dim, num_layer,
  short/long diffusion lists, num_bond_type).  Returns a dict with the issued instruction count,
  the count a full 32-row single-molecule tile would issue (no skipping), flops for both and the
  fraction of tile rows that hold real nodes."""
  n_short, n_long = len(cfg['short_diffusion_dist']), len(cfg['long_diffusion_dist'])
  n_edge = cfg['num_bond_type'] + 1
  C = n_short + n_long + n_edge
  din0, dhid, nl = cfg['input_dim'], cfg['hidden_dim'][0], cfg['num_layer']
  assert n_short == 0, 'short-diffusion powers issue p-1 extra GEMM2 chains: not modelled'

  def per_tile(pg, ps, n_ident):
    tot = 0
    for l in range(nl):
      d_in = din0 if l == 0 else dhid
      per_wave = C * (d_in // 2) + (4 * ps if n_long else 0) + (n_edge - n_ident) * 4 * pg
      if n_long and l + 1 < nl:
        per_wave += 4 * pg
      tot += nwv * per_wave
    if n_long:
      tot += min(nwv, (din0 + 31) // 32) * 4 * pg   # first layer's projection
    tot += dhid // 2                                 # head: one wave per tile
    return tot

  issued = 0
  rows_real = 0
  emask = (1 << n_edge) - 1
  for t in tiles:
    issued += per_tile(t['pg'], t['ps'], bin(t['ident'] & emask).count('1'))
    rows_real += t['nA'] + t['nB']
  full = per_tile(4, 4 if cfg['num_eig_vec'] > 24 else (cfg['num_eig_vec'] + 7) // 8, 0) * len(tiles)
  return dict(tiles=len(tiles), mfma_issued=int(issued), mfma_unskipped=int(full),
              flops_issued=int(issued) * FLOP_PER_MFMA, flops_unskipped=int(full) * FLOP_PER_MFMA,
              mops_counts=int(issued) * (FLOP_PER_MFMA // FLOP_PER_MOPS_COUNT),
              useful_row_frac=rows_real / (32.0 * max(1, len(tiles))))


def forward16_mfma_issued(tiles, cfg):
  """The same record as forward_mfma_issued for lanczosnet_forward16_kernel.  `mfma_issued` counts
  v_mfma_f32_16x16x4_f32 instructions (2048 flop) plus the head's 32x32x2 instructions counted
  double (4096 flop): flops_issued = 2048 * mfma_issued.  That kernel is retired (the strip kernel
  took all its launches); the model stays as the record of its committed counter run,
  profiles/r04_forward16_pmc.json, which tests/test_flop_model.py pins it to."""
  n_long = len(cfg['long_diffusion_dist'])
  n_edge = cfg['num_bond_type'] + 1
  C = n_long + n_edge
  din0, dhid, nl = cfg['input_dim'], cfg['hidden_dim'][0], cfg['num_layer']
  assert len(cfg['short_diffusion_dist']) == 0 and dhid == 128

  def per_tile(pg, ps, n_ident):
    tot = 0
    for l in range(nl):
      d_in = din0 if l == 0 else dhid
      per_wave = C * (d_in // 2) + (8 * ps if n_long else 0) + (n_edge - n_ident) * 8 * pg
      if n_long and l + 1 < nl:
        per_wave += 8 * pg
      tot += 8 * per_wave
    if n_long:
      tot += (din0 // 16) * 8 * pg                   # first layer's projection
    tot += 2 * (dhid // 2)                           # head: one wave per tile, 32x32x2
    return tot

  issued = 0
  rows_real = 0
  emask = (1 << n_edge) - 1
  K = cfg['num_eig_vec']
  for t in tiles:
    pg16 = t['pg16'] if 'pg16' in t else _subtiles16(t['nA'], t['nB'], t['split'])
    ps16 = t['ps16'] if 'ps16' in t else _subtiles16(min(t['nA'], K), min(t['nB'], K), t['split'])
    issued += per_tile(pg16, ps16, bin(t['ident'] & emask).count('1'))
    rows_real += t['nA'] + t['nB']
  full = per_tile(2, 2, 0) * len(tiles)
  return dict(tiles=len(tiles), mfma_issued=int(issued), mfma_unskipped=int(full),
              flops_issued=int(issued) * FLOP_PER_MFMA16, flops_unskipped=int(full) * FLOP_PER_MFMA16,
              mops_counts=int(issued) * (FLOP_PER_MFMA16 // FLOP_PER_MOPS_COUNT),
              useful_row_frac=rows_real / (32.0 * max(1, len(tiles))))


STRIP_INTS = 80   # LNZ_STRIP_INTS


def strips_selected(cfg, B, N):
  """Mirror of lnz::strip_forward_eligible for launches that carry a strip plan (every batch with
  N <= 32: ops.strip_plan_wanted)."""
  if not forward16_selected(cfg):
    return False
  return N <= 32


def strips_from_plan(strips, ident=None):
  """strips: the int32 array written by lnz_plan_strips ([cap * 80 + 1], last word = strips in use);
  ident [B] = identity-channel bits of the edge channels or None.  Returns one dict per strip:
  subtiles, blocks (number of subtile pairs some molecule touches), per-subtile block counts and
  identity bits, real rows."""
  p = np.asarray(strips)
  cap = (p.size - 1) // STRIP_INTS
  out = []
  for s in range(int(p[cap * STRIP_INTS])):
    e = p[s * STRIP_INTS:(s + 1) * STRIP_INTS]
    nm, sub = int(e[0]), int(e[1])
    owner = -np.ones(16 * sub, int)
    idb = [0xffffffff if ident is not None else 0] * sub
    rows_real = 0
    for i in range(nm):
      b, st, n = (int(x) for x in e[2 + 3 * i:5 + 3 * i])
      rows = 4 if n <= 4 else (n + 3) // 4 * 4
      owner[st:st + rows] = i
      rows_real += n
      if ident is not None:
        for I in range(st // 16, (st + rows - 1) // 16 + 1):
          idb[I] &= int(ident[b]) & 0xffffffff
    blk = []
    for I in range(sub):
      mine = set(owner[16 * I:16 * I + 16]) - {-1}
      blk.append(sum(1 for J in (I - 1, I, I + 1)
                     if 0 <= J < sub and mine & (set(owner[16 * J:16 * J + 16]) - {-1})))
    out.append(dict(sub=sub, blk=blk, ident=idb, rows_real=rows_real, mols=nm))
  return out


def strip_mfma_issued(strips, cfg):
  """The record of forward_mfma_issued for lanczosnet_strip_kernel; `mfma_issued` counts
  v_mfma_f32_16x16x4_f32 instructions (2048 flop)."""
  n_long = len(cfg['long_diffusion_dist'])
  n_edge = cfg['num_bond_type'] + 1
  C = n_long + n_edge
  din0, dhid, nl = cfg['input_dim'], cfg['hidden_dim'][0], cfg['num_layer']
  din0 = (din0 + 63) // 64 * 64
  emask = (1 << n_edge) - 1
  issued = full = rows_real = rows_tile = 0
  useful = 0   # the instructions of blocks some molecule touches, identity channels left out
  for t in strips:
    S, touched = t['sub'], sum(t['blk'])
    blocks = 3 * S - 2
    g2_useful = sum(b * (n_edge - bin(i & emask).count('1')) for b, i in zip(t['blk'], t['ident']))
    for l in range(nl):
      d_in = din0 if l == 0 else dhid
      proj = 1 if (n_long and l + 1 < nl) else 0
      issued += 8 * (C * (d_in // 16) * 4 * S + 4 * blocks * ((1 if n_long else 0) + proj) + 4 * n_edge * blocks)
      useful += 8 * (C * (d_in // 16) * 4 * S + 4 * touched * ((1 if n_long else 0) + proj) + 4 * g2_useful)
    if n_long:
      issued += (din0 // 16) * 4 * blocks
      useful += (din0 // 16) * 4 * touched
    issued += S * 64
    useful += S * 64
    full = issued
    rows_real += t['rows_real']
    rows_tile += 16 * S
  return dict(tiles=len(strips), mfma_issued=int(issued), mfma_unskipped=int(full),
              flops_issued=int(issued) * FLOP_PER_MFMA16, flops_unskipped=int(full) * FLOP_PER_MFMA16,
              mops_counts=int(issued) * (FLOP_PER_MFMA16 // FLOP_PER_MOPS_COUNT),
              useful_row_frac=rows_real / float(max(1, rows_tile)),
              mfma_in_touched_blocks=int(useful),
              subtiles=int(sum(t['sub'] for t in strips)),
              max_subtiles_per_strip=int(max(t['sub'] for t in strips)))


# ---- the folded form of the rare bond-type channels (csrc/conv_strip.hip, strip_forward RARE) ----
RARE_MAXV, RARE_MAXF, RARE_MAXS = 8, 5, 5   # virtual subtiles, folded channels, subtiles of a strip


def touch_masks(L, mask):
  """The touched-row rule of the strip kernel, restated: L [B,N,N,C] float32, mask [B,N].  Returns
  uint32 [B,C]: bit i of (b, c) is set when row i or column i of channel c holds a non-zero element
  off the diagonal, or when its diagonal element is not the identity the folded GEMM1 supplies on
  that row: exactly 1 on a node the mask keeps, exactly 0 elsewhere (a node that the mask leaves out
  but the operator keeps — a hole, diagonal 1 — is touched)."""
  L = np.asarray(L, np.float32)
  B, N = L.shape[:2]
  off = L != 0.0
  eye = np.eye(N, dtype=bool)[None, :, :, None]
  off = off & ~eye
  t = off.any(axis=2) | off.any(axis=1)                              # [B,N,C]: row | column
  diag = np.einsum('biic->bic', L)
  t |= diag != (np.asarray(mask) != 0).astype(np.float32)[:, :, None]
  bits = (np.uint64(1) << np.arange(N, dtype=np.uint64))[None, :, None]
  return (t * bits).sum(axis=1).astype(np.uint32)


def strip_touch_counts(strips, touch, n_edge):
  """strips: the int32 strip plan (as for strips_from_plan); touch: uint32 [B,C] of touch_masks (C =
  n_edge edge channels).  Returns, per strip, the touched rows of every folded channel 2 ..
  n_edge-1 (rows of a molecule beyond its extent's 4-row block are not in the strip)."""
  p = np.asarray(strips)
  cap = (p.size - 1) // STRIP_INTS
  out = []
  for s in range(int(p[cap * STRIP_INTS])):
    e = p[s * STRIP_INTS:(s + 1) * STRIP_INTS]
    cnt = [0] * max(0, n_edge - 2)
    for i in range(int(e[0])):
      b, _, n = (int(x) for x in e[2 + 3 * i:5 + 3 * i])
      rows = 4 if n <= 4 else (n + 3) // 4 * 4
      for f in range(len(cnt)):
        cnt[f] += bin(int(touch[b][2 + f]) & ((1 << rows) - 1)).count('1')
    out.append(cnt)
  return out


def rare_cost(S, touch_count, n_fold):
  """The kernel's cost rule, in MFMAs per wave and 128 input columns: (folded form, channel loop,
  virtual subtiles).  Folded: one GEMM1 on the summed weights (32 S) and, per virtual subtile of 16
  touched rows, a 16-row GEMM1 (32) and its scatter (4 S).  Channel loop: GEMM1 and GEMM2 of every
  folded channel."""
  nv = sum((c + 15) // 16 for c in touch_count)
  return 32 * S + nv * (32 + 4 * S), (32 * S + 4 * (3 * S - 2)) * n_fold, nv


def strip_takes_rare(S, touch_count, n_fold):
  """Does a strip of S subtiles take the folded form?  (all of 2 .. n_edge-1 or none)"""
  if S > RARE_MAXS or n_fold < 1 or n_fold > RARE_MAXF:
    return False
  folded, plain, nv = rare_cost(S, touch_count, n_fold)
  return nv <= RARE_MAXV and folded < plain


def strip_rare_mfma_issued(strips, touch_counts, cfg):
  """strip_mfma_issued for the kernel with the folded form (lanczosnet_strip_kernel<0,0,1,false,false>):
  strips from strips_from_plan, touch_counts from strip_touch_counts (None: nothing is folded).  A
  strip that takes the folded form (strip_takes_rare) issues per wave and layer

      GEMM1      (n_long + 2) * d_in / 16 * 4 * S         long scales, edge types 0 and 1
      folded     d_in / 16 * 4 * S                        X (sum_{e >= 2} W_e)^T
      rare       d_in / 16 * 4 + 4 * S   per virtual subtile (16 touched rows of one channel)
      GEMM2      4 * 2 * blocks                           edge types 0 and 1
      lift-back, projection, first projection, head       as strip_mfma_issued

  and every other strip what strip_mfma_issued counts.  Adds `rare_strips`, `virtual_subtiles` and the
  per-wave count of a 128-wide middle layer for the worst and the mean strip of S = max subtiles."""
  n_long = len(cfg['long_diffusion_dist'])
  n_edge = cfg['num_bond_type'] + 1
  C = n_long + n_edge
  n_fold = n_edge - 2
  din0, dhid, nl = cfg['input_dim'], cfg['hidden_dim'][0], cfg['num_layer']
  din0 = (din0 + 63) // 64 * 64
  issued = plain = 0
  rare_strips = nvt = 0
  per_layer = []
  for i, t in enumerate(strips):
    S = t['sub']
    blocks = 3 * S - 2
    tc = touch_counts[i] if touch_counts is not None else None
    rare = tc is not None and strip_takes_rare(S, tc, n_fold)
    nv = rare_cost(S, tc, n_fold)[2] if rare else 0
    rare_strips += int(rare)
    nvt += nv
    for l in range(nl):
      d_in = din0 if l == 0 else dhid
      proj = 1 if (n_long and l + 1 < nl) else 0
      blk = 4 * blocks * ((1 if n_long else 0) + proj)
      old = C * (d_in // 16) * 4 * S + blk + 4 * n_edge * blocks
      new = old if not rare else ((n_long + 3) * (d_in // 16) * 4 * S + nv * ((d_in // 16) * 4 + 4 * S) +
                                  blk + 4 * 2 * blocks)
      issued += 8 * new
      plain += 8 * old
      if l == 1:
        per_layer.append((S, new))
    extra = ((din0 // 16) * 4 * blocks if n_long else 0) + S * 64
    issued += extra
    plain += extra
  smax = max(t['sub'] for t in strips)
  top = [c for s, c in per_layer if s == smax]
  return dict(tiles=len(strips), mfma_issued=int(issued), mfma_channel_loop=int(plain),
              flops_issued=int(issued) * FLOP_PER_MFMA16,
              mops_counts=int(issued) * (FLOP_PER_MFMA16 // FLOP_PER_MOPS_COUNT),
              rare_strips=rare_strips, virtual_subtiles=nvt,
              per_wave_layer_worst=int(max(top)), per_wave_layer_mean=float(np.mean(top)))


FLOP_PER_MFMA16X32_F16 = 2 * 16 * 16 * 32


def strip_split_mfma_issued(strips, cfg):
  """lanczosnet_strip_kernel<.., HALF> (gemm_mode 1): v_mfma_f32_16x16x32_f16 instructions (16384 flop)
  one launch issues — per layer and wave GEMM1 = channels x four 32-k blocks x three products x S
  subtiles (every layer is 128 wide there), and each block-diagonal product (the edge types' GEMM2,
  the lift, the next layer's projection) = three products per subtile PAIR a row subtile touches.
  The first layer's projection and the head stay on v_mfma_f32_16x16x4_f32 (counted apart)."""
  n_long = len(cfg['long_diffusion_dist'])
  n_edge = cfg['num_bond_type'] + 1
  C = n_long + n_edge
  nl = cfg['num_layer']

  def pairs(S):   # (2 p, 2 p + 1) pairs over the row subtiles' neighbourhoods {I - 1, I, I + 1}
    n = 0
    for I in range(S):
      p0 = max(I - 1, 0) >> 1
      n += 1
      if 2 * (p0 + 1) < S and 2 * (p0 + 1) <= I + 1:
        n += 1
    return n

  f16 = f32 = 0
  for t in strips:
    S = t['sub']
    for l in range(nl):
      prods = n_edge + (1 if n_long else 0) + (1 if (n_long and l + 1 < nl) else 0)
      f16 += 8 * 3 * (C * 4 * S + prods * pairs(S))
    if n_long:
      f32 += 8 * 4 * (3 * S - 2)
    f32 += S * 64
  return dict(mfma_f16_issued=int(f16), mfma_f32_issued=int(f32),
              flops_issued=int(f16) * FLOP_PER_MFMA16X32_F16 + int(f32) * FLOP_PER_MFMA16)


def gpnn_flop_per_row_step(D, C, num_prop_cluster, num_prop_cut, msg_hidden=128, state_hidden=512):
  """gpnn_forward_kernel: the products of one outer step per state row (model/gpnn.py:216-230), every padded
  row counted, aggregates and the cells' elementwise work left out —
    the GGNN step      C (2 D h + 2 h D + 2 D 3D) + 2 D 3D          (msg_func[c], gi, gh; h = 128)
    a partition step   2 D h + 2 h D + 2 D 3D + 2 D 3D              (msg_func[0], the partition cell's gi and gh)
    state_func         2 (3 D) H + 2 H D                            (H = 512)
  D 128, C 7, counts (1, 1): 1,245,184 + 2 x 262,144 + 524,288 = 2,293,760."""
  gate = 2 * D * 3 * D
  msg = 2 * D * msg_hidden + 2 * msg_hidden * D
  ggnn_step = C * (msg + gate) + gate
  partition_step = msg + 2 * gate
  state_mlp = 2 * 3 * D * state_hidden + 2 * state_hidden * D
  return dict(ggnn_step=ggnn_step, partition_step=partition_step, state_mlp=state_mlp,
              total=ggnn_step + (num_prop_cluster + num_prop_cut) * partition_step + state_mlp)
