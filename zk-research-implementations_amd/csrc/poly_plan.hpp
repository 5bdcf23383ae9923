// Launch plans of the univariate polynomial kernels (poly.hpp): how batch
// evaluation splits its coefficients, how the interpolation weights split
// their j range, and the levels of the product tree. Pure host code, no HIP,
// no side effects; compiled on its own by tests/native/poly_plan_check.cpp.
//
// Interpolation (univariate_polynomial_dense.rs:48-74) of n points runs as
//   d_i = prod_{j != i} (x_i - x_j),  s_i = y_i / d_i,
//   result = sum_i s_i prod_{j != i} (x - x_j)
// and the sum goes up a product tree: leaf i is (M, N) = (x - x_i, s_i), a
// parent is (M_l M_r, N_l M_r + N_r M_l), the root's N is the interpolant.
// Every M is monic, so a node over `len` points stores the len low
// coefficients of M and the len coefficients of N: each level is two arrays of
// exactly n elements, node t of level l at offset t 2^l. All nodes of a level
// have 2^l points but the last, which has the rest; when a level has an odd
// number of nodes its last node has no sibling and passes through unchanged.
#pragma once
#include <stdint.h>

#include <vector>

namespace zkh {
constexpr uint32_t kPolyBlock = 256;             // lanes per block (zk::kBlock)
constexpr uint64_t kPolyInterpMax = 1ull << 16;  // points; ZK_EUNSUPPORTED above (2.5 n^2 ~ 10^10 products)
constexpr uint32_t kPolyTableMaxLog = 28;        // coefficients or points of one evaluation; ZK_EUNSUPPORTED above
// npoints x ncoeffs of one evaluation call: 2^40 ~ 1.1 x 10^12 products, about
// ten seconds at the 116 G modmul/s of profiles/r1_arith_rates.txt (116 x 10^9 x 10 s
// = 1.16 x 10^12, rounded down to a power of two). ZK_EUNSUPPORTED above.
constexpr uint64_t kPolyEvalMaxProducts = 1ull << 40;
constexpr uint32_t kPolyEvalTile = 512;  // coefficients staged in LDS at a time (16 KiB)
constexpr uint32_t kPolyTreeTile = 128;  // left-operand coefficients staged per step of a tree block
constexpr uint32_t kPolyTreeSplit = 8;   // parts the steps of a large tree level are dealt over (measured: 1, 2, 4, 8)
constexpr uint32_t kPolyFill = 4;        // blocks per CU a launch aims at before it stops splitting
constexpr uint32_t kPolyHostMaxDefault = 96;  // ZK_POLY_HOST_MAX: at most this many points run on the host (the measured crossover)

// ZK_POLY_HOST_MAX as given (empty, negative or above 2^16: the default)
inline uint32_t poly_host_max(long knob) {
  return knob >= 0 && knob <= (long)kPolyInterpMax ? (uint32_t)knob : kPolyHostMaxDefault;
}

inline uint64_t poly_ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Evaluation of d coefficients at m points: one lane per point. With fewer
// point tiles than the chip has room for, the coefficients are cut into
// `chunks` runs of chunk_len (a multiple of kPolyEvalTile; the last run has the
// rest) over blockIdx.y; cell (c, i) = Horner(run c)(x_i), and a second kernel
// sums cell(c, i) x_i^(c chunk_len). chunks = 1: no second kernel.
struct PolyEvalPlan {
  uint32_t chunks;
  uint64_t chunk_len;
};
inline PolyEvalPlan poly_eval_plan(uint64_t m, uint64_t d, uint32_t num_cus) {
  const uint64_t tiles = m ? poly_ceil_div(m, kPolyBlock) : 1;
  const uint64_t want = (uint64_t)kPolyFill * (num_cus ? num_cus : 1);
  if (tiles >= want || d <= kPolyEvalTile) return {1, d};
  uint64_t chunks = poly_ceil_div(want, tiles);
  const uint64_t most = poly_ceil_div(d, kPolyEvalTile);
  if (chunks > most) chunks = most;
  const uint64_t len = poly_ceil_div(poly_ceil_div(d, chunks), kPolyEvalTile) * kPolyEvalTile;
  return {(uint32_t)poly_ceil_div(d, len), len};
}

// The weights d_i over n points: one lane per i, the j range cut into `parts`
// runs of part_len (a multiple of the block) over blockIdx.y; the partial
// products are multiplied together by the kernel that inverts them.
struct PolyWeightsPlan {
  uint32_t parts;
  uint64_t part_len;
};
inline PolyWeightsPlan poly_weights_plan(uint64_t n, uint32_t num_cus) {
  const uint64_t tiles = n ? poly_ceil_div(n, kPolyBlock) : 1;  // of i, and of j
  const uint64_t want = (uint64_t)kPolyFill * (num_cus ? num_cus : 1);
  uint64_t parts = tiles >= want ? 1 : poly_ceil_div(want, tiles);
  if (parts > tiles) parts = tiles;
  const uint64_t len = poly_ceil_div(tiles, parts) * kPolyBlock;
  return {(uint32_t)(n ? poly_ceil_div(n, len) : 1), len};
}

// One level of the tree: in_nodes nodes of 2^log_len points (the last:
// last_in_len) become out_nodes nodes of 2^(log_len + 1) (the last:
// last_out_len). pass_through: in_nodes is odd and the last node is copied.
struct PolyLevel {
  uint32_t log_len;
  uint64_t in_nodes, last_in_len;
  uint64_t out_nodes, last_out_len;
  bool pass_through;
};
// Parts (blockIdx.y) of a level whose nodes have 2^log_len points: a block of a
// level with 2 len > kPolyBlock walks up to len / kPolyTreeTile steps of its left
// operand, dealt round robin over min(kPolyTreeSplit, len / kPolyTreeTile)
// parts whose partial sums a second kernel adds; smaller levels are one part.
inline uint32_t poly_tree_split(uint32_t log_len) {
  const uint64_t len = (uint64_t)1 << log_len;
  if (2 * len <= kPolyBlock) return 1;
  const uint64_t steps = len / kPolyTreeTile;
  return (uint32_t)(steps < kPolyTreeSplit ? (steps < 1 ? 1 : steps) : kPolyTreeSplit);
}
inline uint64_t poly_node_offset(const PolyLevel& lv, uint64_t t, bool out) { return t << (lv.log_len + (out ? 1 : 0)); }
inline std::vector<PolyLevel> poly_tree_plan(uint64_t n) {
  std::vector<PolyLevel> pl;
  for (uint32_t l = 0; n > ((uint64_t)1 << l); ++l) {
    PolyLevel lv;
    lv.log_len = l;
    lv.in_nodes = poly_ceil_div(n, (uint64_t)1 << l);
    lv.last_in_len = n - ((lv.in_nodes - 1) << l);
    lv.out_nodes = poly_ceil_div(n, (uint64_t)2 << l);
    lv.last_out_len = n - ((lv.out_nodes - 1) << (l + 1));
    lv.pass_through = (lv.in_nodes & 1) != 0;
    pl.push_back(lv);
  }
  return pl;
}
}  // namespace zkh
