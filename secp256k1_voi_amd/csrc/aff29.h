// aff29.h — affine doubling and addition over the lazy 9x29 field (fe29.h), one safegcd inversion each: the odd
// multiples and lead points of the wide joint tables (keyed.hip, k_ksw_odd / k_ksw_lead), built once per key set.
// Shared with ops.hip, which exposes them to the tests (S2K_HP_AFF_DBL / S2K_HP_AFF_ADD).
#pragma once
#include "fe29.h"
#include "fe29_inv.h"

namespace s2k {

// affine doubling and addition on y^2 = x^3 + b for any b (the formulas contain no curve constant: they hold on the key's
// isomorphic curve), one safegcd inversion each; operands and results with 1 unit
S2K_DEV void aff_double(fe29& x, fe29& y) {
  const fe29 inv = fe29_inv_gcd(fe29_add(y, y));                                        // 1 / 2y
  const fe29 lam = fe29_mul(fe29_mul_int(fe29_sqr(x), 3), inv);                          // 3 x^2 / 2y  ([3] x [1])
  const fe29 x3 = fe29_sqr_plus(lam, fe29_negate(fe29_add(x, x), 2));                    // lambda^2 - 2x
  y = fe29_mul_plus(lam, fe29_add(x, fe29_negate(x3, 1)), fe29_negate(y, 1));            // lambda (x - x3) - y
  x = x3;
}
S2K_DEV void aff_add(const fe29& x1, const fe29& y1, const fe29& x2, const fe29& y2, fe29& x3, fe29& y3) {
  const fe29 di = fe29_inv_gcd(fe29_add(x2, fe29_negate(x1, 1)));                        // 1 / (x2 - x1)
  const fe29 nya = fe29_negate(y1, 1);
  const fe29 lam = fe29_mul(fe29_add(y2, nya), di);                                      // ([3] x [1])
  x3 = fe29_sqr_plus(lam, fe29_negate(fe29_add(x1, x2), 2));                             // lambda^2 - x1 - x2
  y3 = fe29_mul_plus(lam, fe29_add(x1, fe29_negate(x3, 1)), nya);                        // lambda (x1 - x3) - y1
}

}  // namespace s2k
