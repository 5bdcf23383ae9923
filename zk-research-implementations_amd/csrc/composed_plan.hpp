// Sum-check over any sum of products of multilinear tables, the
// host-only part (no HIP, no zk_ctx, hfield.hpp arithmetic): validation and
// caps, interpolation through the points 0..degree, one host round (the sums at
// the points, then the fold) for any shape, the verifier and `combine`.
// Compiled into the library through composed.hip and, on the CPU alone, into
// tests/native/composed_plan_check.cpp.
//
// The polynomial is f = sum_t prod_d table[factors[t * degree + d]] over
// `ntables` distinct tables of 2^nvars elements; an index may repeat within a
// term and across terms. Round k (sum_check_protocol.rs:86-166 with
// SumPoly::reduce done in full): y_i = sum_j f_k(i, j) for i = 0..degree,
// variable 0 (the MSB) bound to i as partial_evaluate(0, i) binds it; the
// polynomial of degree <= degree through (i, y_i), trailing zeros trimmed; its
// coefficient bytes absorbed; one challenge r_k; every table folded by r_k.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "gkr_rounds.hpp"
#include "hfield.hpp"

namespace zkc {
constexpr uint32_t kComposedMaxTables = 16;
constexpr uint32_t kComposedMaxTerms = 16;
constexpr uint32_t kComposedMaxDegree = 4;  // the highest degree whose round kernels compile without scratch (composed.hpp)
constexpr uint32_t kComposedMaxVars = 26;
constexpr uint32_t kComposedHostLgDefault = 6;  // ZK_COMPOSED_HOST_LG (composed.hip)
constexpr uint32_t kComposedHostLgMax = 16;

// the library's error codes (zk_sumcheck.h), restated so this header stands alone
enum { C_OK = 0, C_EINVAL = 1, C_EUNSUPPORTED = 5 };

// Shape checks and caps. `*err` names what failed.
inline int composed_validate(uint32_t ntables, uint32_t nvars, const uint8_t* factors, uint32_t nterms, uint32_t degree,
                             const char** err) {
  *err = nullptr;
  auto bad = [&](int rc, const char* m) {
    *err = m;
    return rc;
  };
  if (!factors) return bad(C_EINVAL, "factors is null");
  if (ntables == 0 || nterms == 0 || degree == 0) return bad(C_EINVAL, "ntables, nterms and degree must be at least 1");
  if (ntables > kComposedMaxTables) return bad(C_EUNSUPPORTED, "more than 16 tables");
  if (nterms > kComposedMaxTerms) return bad(C_EUNSUPPORTED, "more than 16 terms");
  if (degree > kComposedMaxDegree) return bad(C_EUNSUPPORTED, "degree above the cap (ZK_COMPOSED_MAX_DEGREE)");
  if (nvars > kComposedMaxVars) return bad(C_EUNSUPPORTED, "more than 26 variables");
  for (uint32_t i = 0; i < nterms * degree; ++i)
    if (factors[i] >= ntables) return bad(C_EINVAL, "a factor names a table >= ntables");
  return C_OK;
}

// What the round kernels read of a shape besides the tables: per term, bit d
// set when factor d is the first mention of its table over all terms (that
// thread stores the table's fold), and the tables no term names (folded after
// the terms, so that every table is folded once per round).
struct ComposedMasks {
  uint8_t store[kComposedMaxTerms];
  uint8_t unused[kComposedMaxTables];
  uint32_t nunused = 0;
};
inline ComposedMasks composed_masks(uint32_t ntables, const uint8_t* factors, uint32_t nterms, uint32_t degree) {
  ComposedMasks m{};
  bool seen[kComposedMaxTables] = {false};
  for (uint32_t t = 0; t < nterms; ++t)
    for (uint32_t d = 0; d < degree; ++d) {
      const uint8_t i = factors[t * degree + d];
      if (!seen[i]) m.store[t] |= (uint8_t)(1u << d);
      seen[i] = true;
    }
  for (uint32_t i = 0; i < ntables; ++i)
    if (!seen[i]) m.unused[m.nunused++] = (uint8_t)i;
  return m;
}

// Montgomery image of a small integer
template <class F>
Fe fe_small(uint32_t x) {
  Fe c{};
  c.v[0] = x;
  return zk::hfe_to_mont<F>(c);
}

// Interpolation through (0, y_0) .. (D, y_D): coefficient k = sum_i m[k][i] y_i
// with m the inverse Vandermonde matrix of the points 0..D, built once per
// field and degree from the Lagrange basis L_i(x) = prod_{j != i} (x - j) / (i - j)
// — the unique polynomial UnivariatePoly::interpolate returns
// (univariate_polynomial_dense.rs:48-74), so the same field values.
template <class F>
struct InterpMatrix {
  uint32_t D;
  Fe m[kComposedMaxDegree + 1][kComposedMaxDegree + 1];
  explicit InterpMatrix(uint32_t deg) : D(deg) {
    using namespace zk;
    const Fe zero = fe_zero<F>();
    for (uint32_t i = 0; i <= D; ++i) {
      Fe li[kComposedMaxDegree + 2];  // numerator coefficients, low first
      for (auto& x : li) x = zero;
      li[0] = fe_one<F>();
      int len = 1;
      Fe denom = fe_one<F>();
      for (uint32_t j = 0; j <= D; ++j) {
        if (j == i) continue;
        const Fe xj = fe_small<F>(j);
        for (int k = len; k >= 0; --k) {  // li *= (x - j)
          const Fe up = k > 0 ? li[k - 1] : zero;
          li[k] = hfe_sub<F>(up, hfe_mul<F>(xj, k < len ? li[k] : zero));
        }
        ++len;
        const Fe diff = i > j ? fe_small<F>(i - j) : hfe_sub<F>(zero, fe_small<F>(j - i));
        denom = hfe_mul<F>(denom, diff);
      }
      const Fe inv = fe_inv<F>(denom);
      for (uint32_t k = 0; k <= D; ++k) m[k][i] = hfe_mul<F>(li[k], inv);
    }
  }
};
template <class F>
const InterpMatrix<F>& interp_matrix(uint32_t degree) {  // degree in 1 .. kComposedMaxDegree
  static const InterpMatrix<F> tab[kComposedMaxDegree] = {InterpMatrix<F>(1), InterpMatrix<F>(2), InterpMatrix<F>(3),
                                                          InterpMatrix<F>(4)};
  static_assert(kComposedMaxDegree == 4, "one matrix per degree");
  return tab[degree - 1];
}
// y[0..degree] -> coefficients c[0..degree] (low first); returns the trimmed count
template <class F>
int composed_interpolate(uint32_t degree, const Fe* y, Fe* c) {
  using namespace zk;
  const InterpMatrix<F>& im = interp_matrix<F>(degree);
  for (uint32_t k = 0; k <= degree; ++k) {
    uint64_t acc[9] = {0};
    for (uint32_t i = 0; i <= degree; ++i) h64::mac_wide(acc, h64::of(im.m[k][i]), h64::of(y[i]));
    c[k] = wide_to_fe<F>(acc);
  }
  int m = (int)degree + 1;
  while (m > 0 && fe_is_zero<F>(c[m - 1])) --m;
  return m;
}

// UnivariatePoly::evaluate (univariate_polynomial_dense.rs:20-26)
template <class F>
Fe composed_eval(const Fe* cf, int m, const Fe& x) {
  using namespace zk;
  Fe s = fe_zero<F>();
  for (int i = m; i-- > 0;) s = hfe_add<F>(hfe_mul<F>(s, x), cf[i]);
  return s;
}

// The proof as the driver collects it: (degree + 1) coefficients per round
// (Montgomery, zero past the trimmed count), the challenges, every table at
// the challenge point.
struct ComposedOut {
  std::vector<Fe> coeffs;
  std::vector<uint8_t> ncoeffs;
  std::vector<Fe> challenges;
  std::vector<Fe> table_evals;
};

// Round k from its sums y[0..degree]: interpolate, trim, absorb, draw r_k.
template <class F>
Fe composed_finish_round(zk_transcript* tr, uint32_t degree, const Fe* y, uint32_t k, ComposedOut& out) {
  using namespace zk;
  Fe c[kComposedMaxDegree + 1];
  const int m = composed_interpolate<F>(degree, y, c);
  zkh::absorb<F>(tr, c, (size_t)m);  // (nothing when it trims to nothing)
  out.ncoeffs[k] = (uint8_t)m;
  for (uint32_t i = 0; i <= degree; ++i) out.coeffs[(size_t)(degree + 1) * k + i] = (int)i < m ? c[i] : fe_zero<F>();
  const Fe r = zkh::challenge<F>(tr);
  out.challenges[k] = r;
  return r;
}

template <class F>
void composed_host_fold(std::vector<std::vector<Fe>>& T, const Fe& r) {
  for (auto& t : T) {
    const size_t h = t.size() / 2;
    for (size_t j = 0; j < h; ++j) t[j] = zk::hfe_add<F>(t[j], zk::hfe_mul<F>(r, zk::hfe_sub<F>(t[j + h], t[j])));
    t.resize(h);
  }
}

// y_i = sum_j sum_t prod_d T[factors[t][d]](i, j) for i = 0..degree over the
// pairs (j, j + h) of the current tables. A factor at point i + 1 is the factor
// at i plus (hi - lo); the last product of each term is summed unreduced, one
// accumulator per point.
template <class F>
void composed_host_sums(const std::vector<std::vector<Fe>>& T, const uint8_t* factors, uint32_t nterms, uint32_t degree,
                        Fe* y) {
  using namespace zk;
  const size_t h = T[0].size() / 2;
  const uint32_t np = degree + 1;
  uint64_t acc[kComposedMaxDegree + 1][9] = {{0}};
  for (size_t j = 0; j < h; ++j)
    for (uint32_t t = 0; t < nterms; ++t) {
      Fe prod[kComposedMaxDegree + 1];
      for (uint32_t d = 0; d < degree; ++d) {
        const std::vector<Fe>& X = T[factors[t * degree + d]];
        const Fe diff = hfe_sub<F>(X[j + h], X[j]);
        Fe v = X[j];
        for (uint32_t i = 0; i < np; ++i) {
          if (i) v = hfe_add<F>(v, diff);
          if (d + 1 == degree) h64::mac_wide(acc[i], h64::of(d ? prod[i] : fe_one<F>()), h64::of(v));
          else prod[i] = d ? hfe_mul<F>(prod[i], v) : v;
        }
      }
    }
  for (uint32_t i = 0; i < np; ++i) y[i] = wide_to_fe<F>(acc[i]);
}

// Rounds k0 .. nvars-1 on the host over the current tables T (2^(nvars - k0)
// entries each), then out.table_evals from the last fold.
template <class F>
void composed_host_rounds(std::vector<std::vector<Fe>>& T, const uint8_t* factors, uint32_t nterms, uint32_t degree,
                          uint32_t k0, uint32_t nvars, zk_transcript* tr, ComposedOut& out) {
  for (uint32_t k = k0; k < nvars; ++k) {
    Fe y[kComposedMaxDegree + 1];
    composed_host_sums<F>(T, factors, nterms, degree, y);
    const Fe r = composed_finish_round<F>(tr, degree, y, k, out);
    composed_host_fold<F>(T, r);
  }
  out.table_evals.resize(T.size());
  for (size_t i = 0; i < T.size(); ++i) out.table_evals[i] = T[i][0];
}

inline void composed_out_init(ComposedOut& o, uint32_t nvars, uint32_t degree, const Fe& zero) {
  o.coeffs.assign((size_t)(degree + 1) * nvars, zero);
  o.ncoeffs.assign(nvars, 0);
  o.challenges.assign(nvars, zero);
}

// gkr_verify (sum_check_protocol.rs:117-150) with a degree bound, the one
// round verifier of every sum-check here. coef(k, i) gives coefficient i of
// round k as a Montgomery image; it is asked round by round, only for the
// rounds reached and the coefficients counted, so a caller may convert and
// validate there. Per round: s(0) + s(1) against the claim, the coefficients
// absorbed, r_k drawn and appended to `challenges`, the claim moved to s(r_k).
// Says where it stopped: at nrounds having passed every round, or at the first
// round with more than degree + 1 coefficients or the wrong sum (claim and
// challenges as they stood before that round).
enum class RoundStop { passed, too_many_coeffs, wrong_sum };
struct RoundsEnd {
  RoundStop why;
  uint32_t round;
};
template <class F, class Coef>
RoundsEnd verify_rounds(uint32_t degree, const uint8_t* ncoeffs, uint32_t nrounds, Coef&& coef, zk_transcript* tr,
                        Fe& claim, std::vector<Fe>& challenges) {
  using namespace zk;
  for (uint32_t k = 0; k < nrounds; ++k) {
    const int m = ncoeffs[k];
    if (m > (int)degree + 1) return {RoundStop::too_many_coeffs, k};
    Fe c[kComposedMaxDegree + 1];
    for (int i = 0; i < m; ++i) c[i] = coef(k, (uint32_t)i);
    const Fe s01 = hfe_add<F>(composed_eval<F>(c, m, fe_zero<F>()), composed_eval<F>(c, m, fe_one<F>()));
    if (!fe_eq<F>(s01, claim)) return {RoundStop::wrong_sum, k};
    zkh::absorb<F>(tr, c, (size_t)m);
    const Fe r = zkh::challenge<F>(tr);
    challenges.push_back(r);
    claim = composed_eval<F>(c, m, r);
  }
  return {RoundStop::passed, nrounds};
}

// The rounds of a composed sum-check. cf: (degree + 1) Montgomery coefficients
// per round. A round with more than degree + 1 coefficients, or with
// s(0) + s(1) != claim, rejects: false, and the caller reports final claim 0
// and one zero challenge.
template <class F>
bool composed_verify(uint32_t degree, const Fe* cf, const uint8_t* ncoeffs, uint32_t nrounds, Fe claim,
                     zk_transcript* tr, Fe& final_claim, std::vector<Fe>& challenges) {
  challenges.clear();
  auto coef = [&](uint32_t k, uint32_t i) { return cf[(size_t)(degree + 1) * k + i]; };
  if (verify_rounds<F>(degree, ncoeffs, nrounds, coef, tr, claim, challenges).why != RoundStop::passed) return false;
  final_claim = claim;
  return true;
}

// sum_t prod_d ev[factors[t][d]]
template <class F>
Fe composed_combine(const Fe* ev, const uint8_t* factors, uint32_t nterms, uint32_t degree) {
  using namespace zk;
  Fe s = fe_zero<F>();
  for (uint32_t t = 0; t < nterms; ++t) {
    Fe p = ev[factors[t * degree]];
    for (uint32_t d = 1; d < degree; ++d) p = hfe_mul<F>(p, ev[factors[t * degree + d]]);
    s = hfe_add<F>(s, p);
  }
  return s;
}
}  // namespace zkc
