// Checker for tests/test_committed_plan_cpu.py (test infrastructure, not the
// product): drives csrc/committed_plan.hpp on the CPU alone, no library loaded.
//   self                    mask validation and its errors, the mask helpers, the powers of rho and the combined
//                           value on the boundary scalars 0, 1, p - 1, the 96-byte point encoding; prints "ok cap=16"
//   rho <k>                 rho and k values on stdin -> "p_0 .. p_(k-1)" then "v": rho^j and sum_j rho^j value_j
//   bytes                   x and y (384-bit hex) on stdin -> the 96 bytes as hex
//   transcript <nvars> <ntables> <nterms> <degree> <mask> f_0 .. f_(nterms*degree-1)
//                           stdin: the committed tables' commitments (x y each, index order), then the tables
//                           (ntables x 2^nvars values). Runs the transcript of a committed sum-check on a fresh
//                           transcript with every round on the host: absorbs the commitments, the composed
//                           sum-check, draws rho. Prints "chal r_0 .. r_(nvars-1)", "evals e_0 ..", "rho x",
//                           "pows ..", "v x" (the batch's weights and opened value).
// Fr is BLS12-381's throughout. Field values are canonical hex integers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "committed_plan.hpp"

using namespace zk;
using namespace zkc;
using F = Bls12_381Fr;

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
static Fe read_fe() {
  h64::V v{};
  read_words(v.l, 4);
  return hfe_to_mont<F>(h64::fe(v));
}
static void print_fe(const Fe& m, const char* end) {
  const h64::V o = h64::of(hfe_from_mont<F>(m));
  printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%s", o.l[3], o.l[2], o.l[1], o.l[0], end);
}
static Fe small(uint32_t x) { return fe_small<F>(x); }

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static int self_check() {
  const char* err = nullptr;
  CHECK(committed_validate(6, 3, 3, 0b010110, &err) == C_OK && err == nullptr);
  CHECK(committed_validate(1, 1, 1, 1, &err) == C_OK);
  CHECK(committed_validate(16, 26, 26, 0xFFFF, &err) == C_OK);
  CHECK(committed_validate(6, 3, 3, 0, &err) == C_EINVAL && err);            // nothing committed
  CHECK(committed_validate(6, 3, 3, 1u << 6, &err) == C_EINVAL && err);      // a bit at ntables
  CHECK(committed_validate(6, 3, 3, 1u << 31, &err) == C_EINVAL);
  CHECK(committed_validate(16, 3, 3, 1u << 16, &err) == C_EINVAL);
  CHECK(committed_validate(6, 3, 4, 1, &err) == C_EINVAL && err);            // not the setup's variable count
  CHECK(committed_validate(6, 0, 1, 1, &err) == C_EINVAL);                   // nvars = 0: a setup has >= 1
  CHECK(mask_count(0) == 0 && mask_count(0b010110) == 3 && mask_count(0xFFFFFFFFu) == 32);
  const int all[6] = {10, 11, 12, 13, 14, 15};
  int sel[6] = {0};
  CHECK(committed_select(0b010110u, 6, all, sel) == 3 && sel[0] == 11 && sel[1] == 12 && sel[2] == 14);
  CHECK(committed_select(0b100001u, 6, all, sel) == 2 && sel[0] == 10 && sel[1] == 15);

  // powers of rho and the combined value on the boundary scalars
  const Fe zero = fe_zero<F>(), one = fe_one<F>(), pm1 = hfe_sub<F>(zero, one);
  Fe pw[kLincombMaxTables];
  rho_powers<F>(zero, 16, pw);
  CHECK(fe_eq<F>(pw[0], one));
  for (int j = 1; j < 16; ++j) CHECK(fe_eq<F>(pw[j], zero));
  rho_powers<F>(one, 16, pw);
  for (int j = 0; j < 16; ++j) CHECK(fe_eq<F>(pw[j], one));
  rho_powers<F>(pm1, 16, pw);
  for (int j = 0; j < 16; ++j) CHECK(fe_eq<F>(pw[j], j % 2 ? pm1 : one));
  rho_powers<F>(small(3), 1, pw);  // one table: weight 1 whatever rho is
  CHECK(fe_eq<F>(pw[0], one));
  Fe vals[kLincombMaxTables];
  for (int j = 0; j < 16; ++j) vals[j] = pm1;
  rho_powers<F>(one, 16, pw);
  CHECK(fe_eq<F>(rho_combine<F>(pw, vals, 16), hfe_sub<F>(zero, small(16))));  // 16 (p - 1) = -16
  rho_powers<F>(pm1, 16, pw);
  CHECK(fe_eq<F>(rho_combine<F>(pw, vals, 16), zero));                          // the signs cancel in pairs
  CHECK(fe_eq<F>(rho_combine<F>(pw, vals, 15), pm1));
  CHECK(fe_eq<F>(rho_combine<F>(pw, vals, 2), zero));                           // (p-1) + (p-1)(p-1) = 0
  rho_powers<F>(zero, 16, pw);
  CHECK(fe_eq<F>(rho_combine<F>(pw, vals, 16), pm1));                           // only table 0 counts
  for (int j = 0; j < 16; ++j) vals[j] = zero;
  rho_powers<F>(small(7), 16, pw);
  CHECK(fe_eq<F>(rho_combine<F>(pw, vals, 16), zero));
  vals[2] = one;
  CHECK(fe_eq<F>(rho_combine<F>(pw, vals, 16), small(49)));

  // the 96 bytes of a point: x then y, least significant byte first; infinity is all zero
  uint64_t xy[12];
  for (int i = 0; i < 12; ++i) xy[i] = 0x0807060504030201ull + 0x1010101010101010ull * (uint64_t)i;
  uint8_t b[96];
  g1_bytes(xy, b);
  for (int i = 0; i < 96; ++i) CHECK(b[i] == (uint8_t)(((i / 8) << 4) + (i % 8) + 1));
  memset(xy, 0, sizeof xy);
  memset(b, 0xEE, sizeof b);
  g1_bytes(xy, b);
  for (int i = 0; i < 96; ++i) CHECK(b[i] == 0);
  printf("ok cap=%u\n", kLincombMaxTables);
  return 0;
}

static int rho_mode(uint32_t k) {
  if (k < 1 || k > kLincombMaxTables) return 2;
  const Fe rho = read_fe();
  Fe vals[kLincombMaxTables], pw[kLincombMaxTables];
  for (uint32_t j = 0; j < k; ++j) vals[j] = read_fe();
  rho_powers<F>(rho, k, pw);
  for (uint32_t j = 0; j < k; ++j) print_fe(pw[j], j + 1 < k ? " " : "\n");
  print_fe(rho_combine<F>(pw, vals, k), "\n");
  return 0;
}

static int bytes_mode() {
  uint64_t xy[12];
  read_words(xy, 6);
  read_words(xy + 6, 6);
  uint8_t b[96];
  g1_bytes(xy, b);
  for (int i = 0; i < 96; ++i) printf("%02x", b[i]);
  printf("\n");
  return 0;
}

static int transcript_mode(int argc, char** argv) {
  const uint32_t nvars = (uint32_t)atoi(argv[2]), ntables = (uint32_t)atoi(argv[3]), nterms = (uint32_t)atoi(argv[4]),
                 degree = (uint32_t)atoi(argv[5]), mask = (uint32_t)strtoul(argv[6], nullptr, 0);
  if (nterms > 64 || degree > 64 || (uint32_t)argc != 7 + nterms * degree) return 2;
  std::vector<uint8_t> factors(nterms * degree);
  for (size_t i = 0; i < factors.size(); ++i) factors[i] = (uint8_t)atoi(argv[7 + i]);
  const char* err = nullptr;
  int rc = composed_validate(ntables, nvars, factors.data(), nterms, degree, &err);
  if (!rc) rc = committed_validate(ntables, nvars, nvars, mask, &err);
  if (rc) {
    printf("error=%d %s\n", rc, err);
    return 0;
  }
  if (nvars > 12) return 2;
  const uint32_t nc = mask_count(mask);
  std::vector<uint64_t> points(12 * (size_t)nc);
  for (uint32_t j = 0; j < nc; ++j) {
    read_words(points.data() + 12 * j, 6);
    read_words(points.data() + 12 * j + 6, 6);
  }
  std::vector<std::vector<Fe>> T(ntables, std::vector<Fe>((size_t)1 << nvars));
  for (auto& t : T)
    for (auto& x : t) x = read_fe();
  zk_transcript tr;
  committed_absorb_commitments(&tr, points.data(), nc);
  ComposedOut o;
  composed_out_init(o, nvars, degree, fe_zero<F>());
  composed_host_rounds<F>(T, factors.data(), nterms, degree, 0, nvars, &tr, o);
  const Fe rho = committed_draw_rho<F>(&tr, o.table_evals.data(), ntables);
  printf("chal");
  for (const Fe& r : o.challenges) {
    printf(" ");
    print_fe(r, "");
  }
  printf("\nevals");
  for (const Fe& e : o.table_evals) {
    printf(" ");
    print_fe(e, "");
  }
  printf("\nrho ");
  print_fe(rho, "\n");
  Fe pw[kLincombMaxTables], ev[kLincombMaxTables];
  committed_select(mask, ntables, o.table_evals.data(), ev);
  rho_powers<F>(rho, nc, pw);
  printf("pows");
  for (uint32_t j = 0; j < nc; ++j) {
    printf(" ");
    print_fe(pw[j], "");
  }
  printf("\nv ");
  print_fe(rho_combine<F>(pw, ev, nc), "\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string op(argv[1]);
  if (op == "self") return self_check();
  if (op == "rho" && argc == 3) return rho_mode((uint32_t)atoi(argv[2]));
  if (op == "bytes") return bytes_mode();
  if (op == "transcript" && argc >= 7) return transcript_mode(argc, argv);
  return 2;
}
