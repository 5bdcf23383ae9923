// Checker for tests/test_lookup_plan_cpu.py (test infrastructure, not the
// product): drives csrc/lookup_plan.hpp on the CPU alone, no library loaded.
//   self                 validation, the caps and every error; the slot count; the host inversion against one
//                        Fermat power per element with zeros at every place; the table's evaluation against the
//                        padded table folded in full; prints "ok run=64 block=256"
//   table <field>        a table on stdin -> "slots ..", "digest hex" (or "error=<code> <message>")
//   counts <field>       a table, then n count and the column -> "m c0 c1 ..", "missing k"
//   eval <field>         a table, then n and a point -> the padded table's extension there
//   transcript           (BLS12-381 Fr) a table, n, the column and the four commitments (x y each, in the order
//                        h_f h_t f m) on stdin. Runs the whole prover on the host on a fresh transcript and prints
//                        "alpha x", "tau ..", "lambda x", "polys n c.. | ..", "point ..", "evals ..", "rho x",
//                        "next x" (one more challenge: the end state), then verifies its own proof: "verified 1"
// A table on stdin: T, then T values. Field values are canonical hex.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "lookup_plan.hpp"

using namespace zk;
using namespace zkl;

static void read_words(uint64_t* out, int nwords) {  // one hex integer -> little-endian 64-bit words
  char s[200];
  if (scanf("%199s", s) != 1) exit(2);
  const size_t n = strlen(s);
  for (int i = 0; i < nwords; ++i) out[i] = 0;
  for (size_t i = 0; i < n && i < (size_t)16 * nwords; ++i) {
    const char ch = s[n - 1 - i];
    const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    out[i / 16] |= d << (4 * (i % 16));
  }
}
static uint32_t read_u32() {
  unsigned long v;
  if (scanf("%lu", &v) != 1) exit(2);
  return (uint32_t)v;
}
template <class F>
static Fe read_fe() {
  h64::V v{};
  read_words(v.l, 4);
  return hfe_to_mont<F>(h64::fe(v));
}
template <class F>
static void print_fe(const Fe& m, const char* end) {
  const h64::V o = h64::of(hfe_from_mont<F>(m));
  printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%s", o.l[3], o.l[2], o.l[1], o.l[0], end);
}

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

// T and the values (canonical words); the checks of lookup_validate_table and lookup_entries
template <class F>
static int read_table(uint32_t field, std::vector<Fe>& tm, const char** err) {
  const uint32_t T = read_u32();
  std::vector<uint64_t> vals(4 * (size_t)(T ? T : 1));
  for (uint32_t j = 0; j < T; ++j) read_words(vals.data() + 4 * (size_t)j, 4);
  const int rc = lookup_validate_table(field, vals.data(), T, err);
  if (rc) return rc;
  return lookup_entries<F>(vals.data(), T, false, tm, err);
}

template <class F>
static int self_field() {
  // the host inversion: zeros first, last, in a row, everywhere; one element; in place
  for (size_t count : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)130}) {
    for (int pattern = 0; pattern < 4; ++pattern) {
      std::vector<Fe> v(count), want(count);
      for (size_t i = 0; i < count; ++i) {
        v[i] = zkc::fe_small<F>((uint32_t)(i * 2654435761u + 17));
        const bool z = pattern == 3 || (pattern == 1 && (i == 0 || i + 1 == count)) || (pattern == 2 && i % 3 != 1);
        if (z) v[i] = fe_zero<F>();
        want[i] = hfe_inv<F>(v[i]);
        CHECK(fe_is_zero<F>(v[i]) == fe_is_zero<F>(want[i]));
        CHECK(fe_is_zero<F>(v[i]) || fe_eq<F>(hfe_mul<F>(v[i], want[i]), fe_one<F>()));
      }
      std::vector<Fe> out(count);
      host_batch_inverse<F>(v.data(), count, out.data());
      for (size_t i = 0; i < count; ++i) CHECK(fe_eq<F>(out[i], want[i]));
      host_batch_inverse<F>(v.data(), count, v.data());
      for (size_t i = 0; i < count; ++i) CHECK(fe_eq<F>(v[i], want[i]));
    }
  }
  // the table's evaluation against the padded table folded in full, T = 1, 2^n and in between
  for (uint32_t n = 1; n <= 5; ++n)
    for (uint32_t T = 1; T <= (1u << n); ++T) {
      std::vector<Fe> tm(T), pt(n);
      for (uint32_t j = 0; j < T; ++j) tm[j] = zkc::fe_small<F>(j * 40503u + 11);
      for (uint32_t k = 0; k < n; ++k) pt[k] = zkc::fe_small<F>(k * 7919u + 3 + T);
      std::vector<Fe> pad((size_t)1 << n);
      for (size_t j = 0; j < pad.size(); ++j) pad[j] = tm[j < T ? j : T - 1];
      CHECK(fe_eq<F>(lookup_table_eval<F>(tm.data(), T, pt.data(), n), zkh::mle_eval_host<F>(pad, pt)));
    }
  return 0;
}

static int self_check() {
  const char* err = nullptr;
  const uint64_t one_value[4] = {1, 0, 0, 0};
  CHECK(lookup_validate_table(2, one_value, 1, &err) == L_OK && err == nullptr);
  CHECK(lookup_validate_table(2, one_value, 1u << 24, &err) == L_OK);  // the cap itself
  CHECK(lookup_validate_table(2, one_value, 0, &err) == L_EINVAL && err);
  CHECK(lookup_validate_table(2, nullptr, 1, &err) == L_EINVAL && err);
  CHECK(lookup_validate_table(3, one_value, 1, &err) == L_EINVAL && err);
  CHECK(lookup_validate_table(2, one_value, (1u << 24) + 1, &err) == L_EUNSUPPORTED && err);
  CHECK(lookup_validate_vars(1, 1, &err) == L_OK && lookup_validate_vars(2, 1, &err) == L_OK);
  CHECK(lookup_validate_vars(3, 1, &err) == L_EINVAL && err);  // T > 2^n
  CHECK(lookup_validate_vars(1, 0, &err) == L_EINVAL && err);
  CHECK(lookup_validate_vars(1u << 24, 24, &err) == L_OK);
  CHECK(lookup_validate_vars(1, 25, &err) == L_EUNSUPPORTED && err);
  CHECK(lookup_validate_count(4, 1, 2, &err) == L_OK && lookup_validate_count(4, 1u << 24, 2, &err) == L_OK);
  CHECK(lookup_validate_count(4, 0, 2, &err) == L_EINVAL && err);
  CHECK(lookup_validate_count(5, 1, 2, &err) == L_EINVAL && err);
  CHECK(lookup_validate_count(4, (1u << 24) + 1, 2, &err) == L_EUNSUPPORTED && err);
  // a value >= p: p itself, and p - 1 accepted
  {
    using F = Bls12_381Fr;
    uint64_t v[8];
    for (int i = 0; i < 4; ++i) v[i] = v[4 + i] = h64::P<F>(i);
    v[4] -= 1;
    std::vector<Fe> tm;
    CHECK(lookup_entries<F>(v, 1, false, tm, &err) == L_EINVAL && err);
    CHECK(lookup_entries<F>(v + 4, 1, false, tm, &err) == L_OK && tm.size() == 1);
    CHECK(lookup_entries<F>(v, 1, true, tm, &err) == L_EINVAL);
  }
  // the slot count: the power of two at least 2 T
  CHECK(lookup_slot_log(1) == 1 && lookup_slot_log(2) == 2 && lookup_slot_log(3) == 3 && lookup_slot_log(4) == 3);
  CHECK(lookup_slot_log(5) == 4 && lookup_slot_log(1u << 24) == 25);
  CHECK(lookup_hash(0, 1) == 0 && lookup_hash(1, 4) == (kLookupHashMul >> 28) && lookup_hash(0xFFFFFFFFu, 25) < (1u << 25));
  static_assert(kBatchInvWaveTile == 4096 && kBatchInvBlockTile == 16384, "the plan's tiles");
  if (self_field<Bn254Fr>() || self_field<Bn254Fq>() || self_field<Bls12_381Fr>()) return 1;
  printf("ok run=%u block=%u\n", kBatchInvRun, kBatchInvBlock);
  return 0;
}

template <class F>
static int run_table(uint32_t field, const std::string& mode) {
  const char* err = nullptr;
  std::vector<Fe> tm;
  const int rc = read_table<F>(field, tm, &err);
  if (rc) {
    printf("error=%d %s\n", rc, err);
    return 0;
  }
  const uint32_t T = (uint32_t)tm.size();
  const std::vector<uint32_t> slots = lookup_build_slots<F>(tm.data(), T);
  if (mode == "table") {
    printf("slots");
    for (uint32_t s : slots) printf(" %u", s);
    uint8_t dg[32];
    lookup_digest<F>(field, tm.data(), T, dg);
    printf("\ndigest ");
    for (uint8_t b : dg) printf("%02x", b);
    printf("\n");
    return 0;
  }
  const uint32_t n = read_u32();
  if (mode == "counts") {
    const uint32_t count = read_u32();
    const int rv = lookup_validate_count(T, count, n, &err);
    if (rv) {
      printf("error=%d %s\n", rv, err);
      return 0;
    }
    std::vector<Fe> f(count);
    for (auto& x : f) x = read_fe<F>();
    std::vector<uint32_t> counts;
    const uint64_t missing = lookup_host_counts<F>(tm.data(), T, slots.data(), f.data(), count, counts);
    printf("m");
    for (uint32_t c : counts) printf(" %u", c);
    printf("\nmissing %" PRIu64 "\n", missing);
    return 0;
  }
  const int rv = lookup_validate_vars(T, n, &err);
  if (rv) {
    printf("error=%d %s\n", rv, err);
    return 0;
  }
  if (mode == "eval") {
    std::vector<Fe> pt(n);
    for (auto& x : pt) x = read_fe<F>();
    print_fe<F>(lookup_table_eval<F>(tm.data(), T, pt.data(), n), "\n");
    return 0;
  }
  // transcript
  const size_t N = (size_t)1 << n;
  std::vector<Fe> f(N);
  for (auto& x : f) x = read_fe<F>();
  uint64_t cm[48];  // h_f, h_t, f, m: x[6] then y[6] each
  for (int i = 0; i < 8; ++i) read_words(cm + 6 * i, 6);
  uint8_t dg[32];
  lookup_digest<F>(field, tm.data(), T, dg);
  zk_transcript tr;
  LookupChallenges ch;
  ch.alpha = lookup_begin<F>(&tr, dg, n, cm + 12 * LK_F);
  lookup_draw<F>(&tr, n, cm + 12 * LK_HF, ch);
  std::vector<std::vector<Fe>> tb = lookup_host_tables<F>(tm.data(), T, slots.data(), f.data(), n, ch);
  zkc::committed_absorb_commitments(&tr, cm, 4);
  zkc::ComposedOut out;
  zkc::composed_out_init(out, n, kLookupDegree, fe_zero<F>());
  zkc::composed_host_rounds<F>(tb, kLookupFactors, kLookupTerms, kLookupDegree, 0, n, &tr, out);
  const Fe rho = zkc::committed_draw_rho<F>(&tr, out.table_evals.data(), kLookupTables);
  printf("alpha ");
  print_fe<F>(ch.alpha, "\ntau");
  for (const Fe& x : ch.tau) {
    printf(" ");
    print_fe<F>(x, "");
  }
  printf("\nlambda ");
  print_fe<F>(ch.lambda, "\npolys ");
  for (uint32_t k = 0; k < n; ++k) {
    printf("%u", out.ncoeffs[k]);
    for (uint32_t i = 0; i < out.ncoeffs[k]; ++i) {
      printf(" ");
      print_fe<F>(out.coeffs[4 * k + i], "");
    }
    printf(" | ");
  }
  printf("\npoint");
  for (const Fe& x : out.challenges) {
    printf(" ");
    print_fe<F>(x, "");
  }
  printf("\nevals");
  for (const Fe& x : out.table_evals) {
    printf(" ");
    print_fe<F>(x, "");
  }
  printf("\nrho ");
  print_fe<F>(rho, "\nnext ");
  print_fe<F>(zkh::challenge<F>(&tr), "\n");
  // the verifier's replay, up to the opening
  zk_transcript tv;
  LookupChallenges cv;
  cv.alpha = lookup_begin<F>(&tv, dg, n, cm + 12 * LK_F);
  lookup_draw<F>(&tv, n, cm + 12 * LK_HF, cv);
  zkc::committed_absorb_commitments(&tv, cm, 4);
  Fe fin;
  std::vector<Fe> r;
  bool ok = zkc::composed_verify<F>(kLookupDegree, out.coeffs.data(), out.ncoeffs.data(), n, fe_zero<F>(), &tv, fin, r);
  ok = ok && fe_eq<F>(fin, zkc::composed_combine<F>(out.table_evals.data(), kLookupFactors, kLookupTerms, kLookupDegree));
  ok = ok && lookup_public_ok<F>(cv, r.data(), n, out.table_evals.data(),
                                 lookup_table_eval<F>(tm.data(), T, r.data(), n));
  printf("verified %d\n", ok ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "self") return self_check();
  if (mode == "transcript") return run_table<Bls12_381Fr>(2, mode);
  if (argc < 3) return 2;
  const uint32_t field = (uint32_t)atoi(argv[2]);
  switch (field) {
    case 0: return run_table<Bn254Fr>(field, mode);
    case 1: return run_table<Bn254Fq>(field, mode);
    case 2: return run_table<Bls12_381Fr>(field, mode);
  }
  printf("error=1 unknown field\n");
  return 0;
}
