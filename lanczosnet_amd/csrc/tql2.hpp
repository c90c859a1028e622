// The scalar arithmetic of one implicit-shift QL sweep (EISPACK tql2 recurrences) on a symmetric
// tridiagonal (d, e): the shift, one rotation, the closing step — THE one implementation, shared by
// the QL fallbacks of lanczos_ritz.hip (d / e in lane registers), lanczos_ritz_wg.hip (per-wave LDS
// copies) and lanczos_large.hip (lane registers).  Where d, e and the eigenvectors live, the search
// for a negligible coupling, prefetching, fences and stores stay with the kernels.
//
// A sweep on rows l..m (e_m negligible, |e_i| > eps * tst1 for l <= i < m):
//   sh = ql_shift(d_l, d_{l+1}, e_l);  d_l = sh.dl, d_{l+1} = sh.dl1, d_i -= sh.hh for i >= l + 2
//   QlRotation rot(d_m);
//   for i = m - 1 .. l:  rot.step<NEWTON>(e_i, d_i, e_{i+1}, d_{i+1});
//                        (z_i, z_{i+1}) <- (rot.c z_i - rot.s z_{i+1}, rot.s z_i + rot.c z_{i+1})
//   rot.close(e_{l+1} as it was before the rotations, e_l as it is after them, sh.dl1, e_l, d_l)
//
// (tridiag_eigh_kernel of lanczos_ritz.hip is a fourth QL sweep with other arithmetic — the library
// rsqrt, p = c d_i - s g — and does not use this header.)
#pragma once
#include "wave.hpp"

namespace lnz {

// Wilkinson shift from (d_l, d_{l+1}, e_l): the new d_l, d_{l+1}, and what leaves the rest of the diagonal
struct QlShift {
  double dl, dl1, hh;
};
__device__ __forceinline__ QlShift ql_shift(double d_l, double d_l1, double e_l) {
  double p = (d_l1 - d_l) / (2.0 * e_l);
  double rr = sqrt(p * p + 1.0);
  if (p < 0) rr = -rr;
  const double dl = e_l / (p + rr);
  const double dl1 = e_l * (p + rr);
  return {dl, dl1, d_l - dl};
}

struct QlRotation {
  double c = 1.0, c2 = 1.0, c3 = 1.0, s = 0.0, s2 = 0.0, p;
  __device__ __forceinline__ explicit QlRotation(double d_m) : p(d_m) {}

  // the rotation of rows i, i + 1 from (e_i, d_i): -> e_{i+1}, d_{i+1}; c, s for the eigenvectors.
  // 1 / sqrt(tt) by rsq_nr<NEWTON> (tt is a normal double: |e_i| > eps * tst1) — the IEEE sqrt +
  // divide expand to ~40 dependent fp64 instructions on the rotation-to-rotation critical path.
  template <int NEWTON>
  __device__ __forceinline__ void step(double ei, double di, double& e_next, double& d_next) {
    c3 = c2;
    c2 = c;
    s2 = s;
    const double g = c * ei;
    const double hp = c * p;
    const double tt = fma(p, p, ei * ei);
    const double num = fma(p, di, -(ei * g));  // (p d_i - e_i g): off the rsqrt chain
    const double y = rsq_nr<NEWTON>(tt);
    const double rad = tt * y;
    e_next = s * rad;
    s = ei * y;
    c = p * y;
    p = y * num;  // = c d_i - s g
    d_next = hp + s * (c * g + s * di);
  }

  // after the rotation of rows l, l + 1: the new e_l and d_l
  __device__ __forceinline__ void close(double el1, double e_l, double dl1, double& e_new, double& d_new) {
    p = -s * s2 * c3 * el1 * e_l / dl1;
    e_new = s * p;
    d_new = c * p;
  }
};

}  // namespace lnz
