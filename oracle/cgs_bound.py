"""The two data-dependent rules of the project's Lanczos kernels, stated once in float64 (csrc/wave.hpp
lnz::CgsBound and lnz::matrix_scale_pow2): when the second classical
Gram-Schmidt pass runs, and what a breakdown is relative to.  tests/algo_mirror.py (the full-length
kernels' mirror) and oracle/lanczos_kstep.py (the K-step kernels' restatement) both call these."""
import numpy as np

TOL = 1e-8          # breakdown: beta <= TOL * (the matrix' scale, matrix_scale below)
EPS = 2.220446049250313e-16
CGS_AGAIN = 0.99    # second pass where the first removed more than this part of |x|^2 ...
ORTH_BOUND2 = 1e-18  # ... or where the bound on the new vector's squared loss of orthogonality passes this


def matrix_scale(A):
  """2^ceil(log2 max |a_ij|) (0 for the zero matrix): the power of two the breakdown tolerance is
  taken relative to — a matrix times a power of two takes the same decisions."""
  A = np.asarray(A)
  amax = float(np.abs(A).max()) if A.size else 0.0
  if amax == 0.0:
    return 0.0
  m, e = np.frexp(amax)
  return float(np.ldexp(1.0, e - 1 if m == 0.5 else e))


class OrthBound:
  """lnz::CgsBound (csrc/wave.hpp): bounds on the squared loss of orthogonality of the last two
  accepted basis vectors (cur, prev) and of the candidate the last Gram-Schmidt call produced."""

  def __init__(self):
    self.cur = self.prev = self.cand = 0.0
    self.second_passes = 0
    self.worst = 0.0   # (the largest accepted bound: statistics)

  def accept(self):
    self.prev, self.cur = self.cur, self.cand
    self.worst = max(self.worst, self.cand)


def cgs2(Qt, w, j, rule='bound', ob=None, restart=False, frac=CGS_AGAIN):
  """Classical Gram-Schmidt against the stored basis, once or twice (csrc/lanczos_ritz.hip cgs2_32).
  One pass against a basis whose Gram matrix is I + E leaves Q^T x' = -E c: relative to the new
  vector |E c| / |x'|, and c lives on the last two vectors (alpha, beta) — the loss of orthogonality
  follows e_new <= g max(e_cur, e_prev) + eps |x| / |x'| with g = |c| / |x'|, |x'|^2 = |x|^2 - |c|^2.
  Where g > 1 step after step (a spectrum spread evenly: alpha ~ 2 beta) this compounds.
  rule 'bound' (the kernels'): the second pass runs where the first removed more than `frac` (99 %
  in the full-length kernels, 1 - 1e-6 in the K-step kernels) of
  |x|^2, where the bound (carried in squares, (a + b)^2 <= 9/8 a^2 + 9 b^2) passes ORTH_BOUND2, and
  for a restart vector (its c is spread over all basis vectors, each within the bound);
  'fraction': the `frac` rule alone — the kernels' rule until the spread spectra, kept to show what
  it does; 'always'."""
  ob = ob if ob is not None else OrthBound()
  floor = 9.0 * EPS * EPS
  emax = ORTH_BOUND2 if restart else max(ob.cur, ob.prev)
  # the part of |x|^2 the first pass may remove: g2 (floor + 9/8 emax) + floor <= ORTH_BOUND2 with
  # g2 = cc2 / (xx - cc2), solved for cc2 / xx — known before the pass (lnz::CgsBound::threshold)
  room = ORTH_BOUND2 - floor
  thr = {'fraction': frac, 'always': 0.0,
         'bound': 0.0 if restart else min(frac, room / (floor + 1.125 * max(ob.cur, ob.prev) + room))}[rule]
  xx = float(w @ w)
  c = Qt[:j + 1] @ w
  w = w - Qt[:j + 1].T @ c
  coef = c[j]
  cc2 = float(c @ c)
  again = rule == 'always' or not (cc2 <= thr * xx)
  if again:
    ob.second_passes += 1
    c = Qt[:j + 1] @ w
    w = w - Qt[:j + 1].T @ c
    coef += c[j]
  g2 = cc2 / max(xx - cc2, 1e-30 * xx) if xx > 0.0 else 0.0
  ge = 1.125 * g2 * emax
  ob.cand = ge * emax + floor if again else floor * g2 + (ge + floor)
  return w, coef
