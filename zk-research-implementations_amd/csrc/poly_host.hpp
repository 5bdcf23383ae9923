// Small univariate evaluations and interpolations on the host (hfield.hpp):
// what poly.hip runs below ZK_POLY_HOST_MAX instead of a launch and two copies.
// The same O(n^2) formulation as the kernels of poly.hpp, not the reference's
// O(n^3) loop; values are Montgomery images. Host code only, no HIP: compiled
// on its own by tests/native/poly_asan_check.cpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "hfield.hpp"

namespace zkh {
using zk::Fe;

template <class F>
inline Fe h_fe_inv(const Fe& x) {  // x^(p - 2), field.hpp fe_inv on 64-bit limbs
  Fe r = zk::fe_one<F>();
  for (int w = 7; w >= 0; --w) {
    const uint32_t e = zk::p_minus_2_word<F>(w);
    for (int b = 31; b >= 0; --b) {
      r = zk::hfe_mul<F>(r, r);
      if ((e >> b) & 1u) r = zk::hfe_mul<F>(r, x);
    }
  }
  return r;
}

// evaluate :20-26 at m points by Horner; no coefficients: 0 everywhere
template <class F>
inline void host_poly_evaluate(const Fe* coeffs, uint64_t d, const Fe* xs, uint64_t m, Fe* out) {
  for (uint64_t i = 0; i < m; ++i) {
    Fe acc = zk::fe_zero<F>();
    for (uint64_t k = d; k-- > 0;) acc = zk::hfe_add<F>(zk::hfe_mul<F>(acc, xs[i]), coeffs[k]);
    out[i] = acc;
  }
}

// interpolate :48-74: out[0 .. n) = the coefficients of the polynomial of
// degree < n through (xs[i], ys[i]), untrimmed. false: two x are equal.
//   d_i = prod_{j != i} (x_i - x_j), inverted together (Montgomery's trick, one power);
//   A(x) = prod_j (x - x_j); result = sum_i (y_i / d_i) A(x) / (x - x_i), each
//   quotient by synthetic division.
template <class F>
inline bool host_poly_interpolate(const Fe* xs, const Fe* ys, uint64_t n, Fe* out) {
  if (n == 0) return true;
  std::vector<Fe> dd(n), pre(n);
  Fe run = zk::fe_one<F>();
  for (uint64_t i = 0; i < n; ++i) {
    Fe acc = zk::fe_one<F>();
    for (uint64_t j = 0; j < n; ++j)
      if (j != i) acc = zk::hfe_mul<F>(acc, zk::hfe_sub<F>(xs[i], xs[j]));
    if (zk::fe_is_zero<F>(acc)) return false;
    dd[i] = acc;
    pre[i] = run;  // d_0 ... d_(i-1)
    run = zk::hfe_mul<F>(run, acc);
  }
  Fe inv = h_fe_inv<F>(run);
  for (uint64_t i = n; i-- > 0;) {  // dd[i] <- y_i / d_i
    const Fe di_inv = zk::hfe_mul<F>(inv, pre[i]);
    inv = zk::hfe_mul<F>(inv, dd[i]);
    dd[i] = zk::hfe_mul<F>(ys[i], di_inv);
  }
  std::vector<Fe> A(n + 1, zk::fe_zero<F>()), q(n);
  A[0] = zk::fe_one<F>();
  for (uint64_t j = 0; j < n; ++j) {  // A <- A (x - x_j)
    for (uint64_t k = j + 1; k-- > 0;) {
      const Fe low = zk::hfe_mul<F>(A[k], xs[j]);
      A[k + 1] = zk::hfe_add<F>(A[k + 1], A[k]);
      A[k] = zk::hfe_sub<F>(zk::fe_zero<F>(), low);
    }
  }
  for (uint64_t k = 0; k < n; ++k) out[k] = zk::fe_zero<F>();
  for (uint64_t i = 0; i < n; ++i) {
    q[n - 1] = A[n];  // 1
    for (uint64_t k = n - 1; k > 0; --k) q[k - 1] = zk::hfe_add<F>(A[k], zk::hfe_mul<F>(xs[i], q[k]));
    for (uint64_t k = 0; k < n; ++k) out[k] = zk::hfe_add<F>(out[k], zk::hfe_mul<F>(dd[i], q[k]));
  }
  return true;
}
}  // namespace zkh
