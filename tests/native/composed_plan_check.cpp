// Checker for tests/test_composed_plan_cpu.py (test infrastructure, not the
// product): drives csrc/composed_plan.hpp on the CPU alone, no library loaded.
//   self                          validation, caps and the store / unused masks; prints "ok cap=<degree cap>"
//   interp <field> <degree>       y_0 .. y_degree on stdin -> "m c_0 .. c_degree" (trimmed count, coefficients)
//   rounds <field> <nvars> <ntables> <nterms> <degree> f_0 .. f_(nterms*degree-1)
//                                 the tables on stdin (ntables x 2^nvars values); every round on the host on a
//                                 fresh transcript; prints per round "k m c_0 .. c_degree r", then
//                                 "evals e_0 .. e_(ntables-1)", then "combine v"; fails unless the verifier
//                                 accepts the proof and its final claim equals combine
// Field: 0 (BN254 Fr), 1 (BN254 Fq), 2 (BLS12-381 Fr). Every field value is one canonical hex integer.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "composed_plan.hpp"

using namespace zk;
using namespace zkc;

template <class F>
Fe read_fe() {
  char s[80];
  if (scanf("%79s", s) != 1) exit(2);
  const size_t n = strlen(s);
  h64::V v{};
  for (size_t i = 0; i < n && i < 64; ++i) {  // hex digits, least significant last
    const char ch = s[n - 1 - i];
    const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    v.l[i / 16] |= d << (4 * (i % 16));
  }
  return hfe_to_mont<F>(h64::fe(v));
}
template <class F>
void print_fe(const Fe& m, const char* end) {
  const h64::V o = h64::of(hfe_from_mont<F>(m));
  printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%s", o.l[3], o.l[2], o.l[1], o.l[0], end);
}

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                  \
    }                                                            \
  } while (0)

static int self_check() {
  const char* err = nullptr;
  uint8_t f[kComposedMaxTerms * (kComposedMaxDegree + 1) + 1] = {0};
  CHECK(composed_validate(1, 0, f, 1, 1, &err) == C_OK && err == nullptr);
  CHECK(composed_validate(16, 26, f, 16, kComposedMaxDegree, &err) == C_OK);
  CHECK(composed_validate(1, 0, nullptr, 1, 1, &err) == C_EINVAL && err);
  CHECK(composed_validate(0, 3, f, 1, 1, &err) == C_EINVAL);
  CHECK(composed_validate(1, 3, f, 0, 1, &err) == C_EINVAL);
  CHECK(composed_validate(1, 3, f, 1, 0, &err) == C_EINVAL);
  CHECK(composed_validate(17, 3, f, 1, 1, &err) == C_EUNSUPPORTED);
  CHECK(composed_validate(1, 3, f, 17, 1, &err) == C_EUNSUPPORTED);
  CHECK(composed_validate(1, 3, f, 1, kComposedMaxDegree + 1, &err) == C_EUNSUPPORTED);
  CHECK(composed_validate(1, 27, f, 1, 1, &err) == C_EUNSUPPORTED);
  const uint8_t g[6] = {0, 1, 2, 0, 3, 3};
  CHECK(composed_validate(4, 3, g, 2, 3, &err) == C_OK);
  CHECK(composed_validate(3, 3, g, 2, 3, &err) == C_EINVAL);  // index 3 >= 3 tables
  // first mentions: term 0 stores all three, term 1 only its first 3
  ComposedMasks m = composed_masks(6, g, 2, 3);
  CHECK(m.store[0] == 7 && m.store[1] == 2);
  CHECK(m.nunused == 2 && m.unused[0] == 4 && m.unused[1] == 5);
  m = composed_masks(4, g, 2, 3);
  CHECK(m.nunused == 0);
  // every table is stored exactly once, however the indices repeat
  const uint8_t rep[8] = {1, 1, 1, 1, 0, 1, 0, 2};
  m = composed_masks(3, rep, 2, 4);
  int stores[3] = {0, 0, 0};
  for (int t = 0; t < 2; ++t)
    for (int d = 0; d < 4; ++d)
      if ((m.store[t] >> d) & 1) ++stores[rep[4 * t + d]];
  CHECK(stores[0] == 1 && stores[1] == 1 && stores[2] == 1 && m.nunused == 0);
  printf("ok cap=%u\n", kComposedMaxDegree);
  return 0;
}

template <class F>
int interp(uint32_t degree) {
  Fe y[kComposedMaxDegree + 1], c[kComposedMaxDegree + 1];
  for (uint32_t i = 0; i <= degree; ++i) y[i] = read_fe<F>();
  const int m = composed_interpolate<F>(degree, y, c);
  printf("%d", m);
  for (uint32_t i = 0; i <= degree; ++i) {
    printf(" ");
    print_fe<F>(c[i], "");
  }
  printf("\n");
  // the polynomial passes through its points again
  for (uint32_t i = 0; i <= degree; ++i)
    if (!fe_eq<F>(composed_eval<F>(c, m, fe_small<F>(i)), y[i])) return 1;
  return 0;
}

template <class F>
int rounds(int argc, char** argv) {
  const uint32_t nvars = (uint32_t)atoi(argv[3]), ntables = (uint32_t)atoi(argv[4]), nterms = (uint32_t)atoi(argv[5]),
                 degree = (uint32_t)atoi(argv[6]);
  if (nterms > 64 || degree > 64 || (uint32_t)argc != 7 + nterms * degree) return 2;
  std::vector<uint8_t> factors(nterms * degree);
  for (size_t i = 0; i < factors.size(); ++i) factors[i] = (uint8_t)atoi(argv[7 + i]);
  const char* err = nullptr;
  if (const int rc = composed_validate(ntables, nvars, factors.data(), nterms, degree, &err)) {
    printf("error=%d %s\n", rc, err);
    return 0;
  }
  if (nvars > 16) return 2;
  std::vector<std::vector<Fe>> T(ntables, std::vector<Fe>((size_t)1 << nvars));
  for (auto& t : T)
    for (auto& x : t) x = read_fe<F>();
  zk_transcript tr;
  ComposedOut o;
  composed_out_init(o, nvars, degree, fe_zero<F>());
  composed_host_rounds<F>(T, factors.data(), nterms, degree, 0, nvars, &tr, o);
  for (uint32_t k = 0; k < nvars; ++k) {
    printf("%u %u ", k, (unsigned)o.ncoeffs[k]);
    for (uint32_t i = 0; i <= degree; ++i) print_fe<F>(o.coeffs[(size_t)(degree + 1) * k + i], " ");
    print_fe<F>(o.challenges[k], "\n");
  }
  printf("evals");
  for (const Fe& e : o.table_evals) {
    printf(" ");
    print_fe<F>(e, "");
  }
  printf("\ncombine ");
  print_fe<F>(composed_combine<F>(o.table_evals.data(), factors.data(), nterms, degree), "\n");
  // the verifier accepts what the prover made, with the true sum as the claim
  if (nvars > 0) {
    const Fe* c0 = o.coeffs.data();
    const int m0 = o.ncoeffs[0];
    const Fe claim = hfe_add<F>(composed_eval<F>(c0, m0, fe_zero<F>()), composed_eval<F>(c0, m0, fe_one<F>()));
    zk_transcript tv;
    Fe fin;
    std::vector<Fe> chal;
    if (!composed_verify<F>(degree, o.coeffs.data(), o.ncoeffs.data(), nvars, claim, &tv, fin, chal)) return 1;
    if (!fe_eq<F>(fin, composed_combine<F>(o.table_evals.data(), factors.data(), nterms, degree))) return 1;
    for (uint32_t k = 0; k < nvars; ++k)
      if (!fe_eq<F>(chal[k], o.challenges[k])) return 1;
  }
  return 0;
}

template <class Fn>
int by_field(int field, Fn&& fn) {
  switch (field) {
    case 0: return fn(Bn254Fr{});
    case 1: return fn(Bn254Fq{});
    case 2: return fn(Bls12_381Fr{});
    default: return 2;
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string op(argv[1]);
  if (op == "self") return self_check();
  if (op == "interp" && argc == 4) {
    const uint32_t degree = (uint32_t)atoi(argv[3]);
    if (degree < 1 || degree > kComposedMaxDegree) return 2;
    return by_field(atoi(argv[2]), [&](auto f) { return interp<decltype(f)>(degree); });
  }
  if (op == "rounds" && argc >= 7) return by_field(atoi(argv[2]), [&](auto f) { return rounds<decltype(f)>(argc, argv); });
  return 2;
}
