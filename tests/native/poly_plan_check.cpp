// Checks and prints the launch plans of csrc/poly_plan.hpp (test
// infrastructure, host code only). For every n = 0..300 and a spread up to
// 2^16 it checks, per tree level: the input nodes tile [0, n) exactly, so do the
// output nodes, a last node without a sibling keeps its offset and length, and
// the kernel's map from an output index to (pair, k) covers every index once.
// It checks the weights split for the same n and the evaluation split for a
// grid of (m, d), and field.hpp's fe_inv (and its 64-bit host twin) against
// x * x^-1 = 1 on all three fields. Then it prints
//   consts block=.. eval_tile=.. tree_tile=.. tree_split=.. fill=.. host_max=.. interp_max=.. table_max_log=.. eval_max_products=..
//   knob <value>=<threshold>                          per argument that is not n=..
//   tree n=<n> <log_len>:<in_nodes>:<last_in>:<out_nodes>:<last_out>:<pass> ...
//   weights n=<n> cus=<c> parts=<p> len=<l>
//   eval m=<m> d=<d> cus=<c> chunks=<k> len=<l>
// for the n, (m, d) it checked with a name, and "poly_plan_check ok".
// Compiled and read by tests/test_poly_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poly_host.hpp"
#include "poly_plan.hpp"

using namespace zkh;

static int failures = 0;
#define EXPECT(c)                                                                  \
  do {                                                                             \
    if (!(c)) {                                                                    \
      if (failures < 20) fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                                  \
    }                                                                              \
  } while (0)

static void check_tree(uint64_t n, bool print) {
  const std::vector<PolyLevel> pl = poly_tree_plan(n);
  if (print) printf("tree n=%llu", (unsigned long long)n);
  uint64_t expect_nodes = n;  // level 0 has n leaves of one point
  for (size_t li = 0; li < pl.size(); ++li) {
    const PolyLevel& lv = pl[li];
    const uint64_t len = (uint64_t)1 << lv.log_len;
    EXPECT(lv.log_len == li && lv.in_nodes == expect_nodes && lv.in_nodes >= 2);
    // the parts of a level: one while a pair fits a block, else at most one per step of the longest walk
    const uint32_t S = poly_tree_split(lv.log_len);
    EXPECT(S >= 1 && S <= kPolyTreeSplit && (2 * len > kPolyBlock ? (uint64_t)S * kPolyTreeTile <= len : S == 1));
    // the nodes tile the arrays: offsets t len, lengths len but the last, summing to n
    EXPECT(poly_node_offset(lv, lv.in_nodes - 1, false) + lv.last_in_len == n && lv.last_in_len >= 1 && lv.last_in_len <= len);
    EXPECT(poly_node_offset(lv, lv.out_nodes - 1, true) + lv.last_out_len == n && lv.last_out_len >= 1 && lv.last_out_len <= 2 * len);
    EXPECT((lv.in_nodes - 1) * len + lv.last_in_len == n && (lv.out_nodes - 1) * 2 * len + lv.last_out_len == n);
    EXPECT(lv.out_nodes == (lv.in_nodes + 1) / 2 && lv.pass_through == (lv.in_nodes % 2 == 1));
    if (lv.pass_through) {  // the copied node keeps offset and length
      EXPECT(poly_node_offset(lv, lv.in_nodes - 1, false) == poly_node_offset(lv, lv.out_nodes - 1, true));
      EXPECT(lv.last_in_len == lv.last_out_len);
    } else {
      EXPECT(lv.last_out_len == len + lv.last_in_len);
    }
    // the kernel's map g -> (pair offset, k): every output index once, inside its node
    if (n <= 5000 || li + 3 >= pl.size()) {
      std::vector<unsigned char> hit(n, 0);
      for (uint64_t g = 0; g < n; ++g) {
        const uint64_t off = (g >> (lv.log_len + 1)) << (lv.log_len + 1), rem = n - off, t = off >> (lv.log_len + 1);
        EXPECT(t < lv.out_nodes && off == poly_node_offset(lv, t, true));
        const uint64_t out_len = t + 1 == lv.out_nodes ? lv.last_out_len : 2 * len;
        if (rem <= len) {
          EXPECT(lv.pass_through && t + 1 == lv.out_nodes);
        } else {
          const uint64_t a = len, b = rem - len < len ? rem - len : len;
          EXPECT(a + b == out_len);
        }
        EXPECT(g - off < out_len && !hit[g]);
        hit[g] = 1;
      }
    }
    expect_nodes = lv.out_nodes;
    if (print)
      printf(" %u:%llu:%llu:%llu:%llu:%d", lv.log_len, (unsigned long long)lv.in_nodes, (unsigned long long)lv.last_in_len,
             (unsigned long long)lv.out_nodes, (unsigned long long)lv.last_out_len, lv.pass_through ? 1 : 0);
  }
  EXPECT(n <= 1 ? pl.empty() : (expect_nodes == 1 && pl.back().last_out_len == n));
  if (print) printf("\n");
}

static void check_weights(uint64_t n, uint32_t cus, bool print) {
  const PolyWeightsPlan wp = poly_weights_plan(n, cus);
  EXPECT(wp.parts >= 1 && wp.part_len >= kPolyBlock && wp.part_len % kPolyBlock == 0);
  EXPECT((uint64_t)wp.parts * wp.part_len >= n && (n == 0 || (uint64_t)(wp.parts - 1) * wp.part_len < n));  // every j once, no empty part
  if (print) printf("weights n=%llu cus=%u parts=%u len=%llu\n", (unsigned long long)n, cus, wp.parts, (unsigned long long)wp.part_len);
}

static void check_eval(uint64_t m, uint64_t d, uint32_t cus, bool print) {
  const PolyEvalPlan ep = poly_eval_plan(m, d, cus);
  EXPECT(ep.chunks >= 1 && ep.chunks <= 65535);  // gridDim.y
  if (ep.chunks == 1) {
    EXPECT(ep.chunk_len == d);
  } else {
    EXPECT(ep.chunk_len % kPolyEvalTile == 0 && ep.chunk_len > 0);
    EXPECT((uint64_t)ep.chunks * ep.chunk_len >= d && (uint64_t)(ep.chunks - 1) * ep.chunk_len < d);  // every coefficient once, no empty run
    EXPECT(poly_ceil_div(m, kPolyBlock) < (uint64_t)kPolyFill * cus && d > kPolyEvalTile);
  }
  if (print)
    printf("eval m=%llu d=%llu cus=%u chunks=%u len=%llu\n", (unsigned long long)m, (unsigned long long)d, cus, ep.chunks,
           (unsigned long long)ep.chunk_len);
}

template <class F>
static void check_inverse() {
  zk::Fe x = zk::fe_one<F>();
  const zk::Fe three = zk::fe_add<F>(zk::fe_add<F>(x, x), x);
  for (int i = 0; i < 40; ++i) {
    x = zk::fe_add<F>(zk::fe_mul<F>(x, three), zk::fe_one<F>());  // 1, 4, 13, ... then wrapping values
    x = zk::fe_mul<F>(x, x);
    if (zk::fe_is_zero<F>(x)) continue;
    const zk::Fe a = zk::fe_inv<F>(x), b = h_fe_inv<F>(x);
    EXPECT(zk::fe_eq<F>(a, b));
    EXPECT(zk::fe_eq<F>(zk::fe_mul<F>(a, x), zk::fe_one<F>()));
  }
  EXPECT(zk::fe_is_zero<F>(zk::fe_inv<F>(zk::fe_zero<F>())));
  // p - 2, word by word: p - (p - 2) = 2
  uint64_t borrow = 0, diff0 = 0;
  for (int k = 0; k < 8; ++k) {
    const uint64_t dd = (uint64_t)F::P[k] - zk::PMinus2<F>::W[k] - borrow;
    borrow = (dd >> 63) & 1;
    if (k == 0) diff0 = (uint32_t)dd;
    else EXPECT((uint32_t)dd == 0);
  }
  EXPECT(diff0 == 2 && borrow == 0);
}

int main(int argc, char** argv) {
  printf("consts block=%u eval_tile=%u tree_tile=%u tree_split=%u fill=%u host_max=%u interp_max=%llu table_max_log=%u eval_max_products=%llu\n",
         kPolyBlock, kPolyEvalTile, kPolyTreeTile, kPolyTreeSplit, kPolyFill, kPolyHostMaxDefault, (unsigned long long)kPolyInterpMax,
         kPolyTableMaxLog, (unsigned long long)kPolyEvalMaxProducts);
  std::vector<uint64_t> named;
  for (int i = 1; i < argc; ++i) {
    if (strncmp(argv[i], "n=", 2) == 0) named.push_back(strtoull(argv[i] + 2, nullptr, 0));
    else printf("knob %s=%u\n", argv[i], poly_host_max(*argv[i] ? strtol(argv[i], nullptr, 0) : -1));
  }
  for (uint64_t n = 0; n <= 300; ++n) check_tree(n, false);
  for (uint64_t n : {511ull, 512ull, 513ull, 767ull, 1000ull, 1025ull, 4095ull, 4097ull, 12345ull, 32768ull, 32769ull, 49152ull, 65535ull, 65536ull})
    check_tree(n, false);
  for (uint64_t n : named) check_tree(n, true);
  for (uint32_t cus : {1u, 8u, 256u, 304u}) {
    for (uint64_t n = 0; n <= 300; ++n) check_weights(n, cus, false);
    for (uint64_t n : {1000ull, 8192ull, 12345ull, 65535ull, 65536ull}) check_weights(n, cus, cus == 256);
    for (uint64_t m : {0ull, 1ull, 3ull, 255ull, 256ull, 257ull, 1000ull, 262143ull, 262144ull, 1ull << 20, 1ull << 28})
      for (uint64_t d : {0ull, 1ull, 4ull, 511ull, 512ull, 513ull, 1553ull, 4096ull, 100000ull, 1ull << 20, 1ull << 28})
        check_eval(m, d, cus, cus == 256 && (m <= 3 || m == 1000) && (d == 513 || d == 1553 || d == (1ull << 20)));
  }
  check_inverse<zk::Bn254Fr>();
  check_inverse<zk::Bn254Fq>();
  check_inverse<zk::Bls12_381Fr>();
  if (failures) {
    fprintf(stderr, "poly_plan_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("poly_plan_check ok\n");
  return 0;
}
