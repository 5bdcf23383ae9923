// gfx950 kernels of the composed sum-check: the sums of
// f = sum_t prod_d table[factors[t][d]] at the points 0..D of the round's
// variable, over the input tables (k_composed_round0) or fused with the fold
// of the previous round's tables (k_composed_round, as k_gkr_round does for
// four tables). Device code; included once by composed.hip.
//
// Work split: one thread per pair (j, j + h), looping over the terms. The
// shape is run-time data, so nothing indexed by it may live in registers (a
// run-time-indexed register array goes to scratch): the table pointers, the
// factor indices and the store masks sit in the kernel-argument segment and
// are read with uniform (scalar) loads, and a thread holds only what one term
// needs — the running product at each of the D + 1 points, the current factor
// and its difference — plus one unreduced accumulator per point. The other
// split, a thread per (pair, term), would repeat the block's limb-sum epilogue
// (17 (D + 1) columns) per term and leave lanes idle whenever the term count
// does not divide the wave; its register saving is nil, because the
// accumulators, not the per-term state, are the larger part.
// A table that several terms name is loaded by each of them (the repeats hit
// the cache) and folded by each, but stored by the first alone
// (ComposedMasks::store), so every table is written once per round; tables
// that no term names are folded after the terms.
#pragma once
#include "composed_plan.hpp"
#include "kernels.hpp"

namespace zk {

struct ComposedArgs {
  const Fe* in[zkc::kComposedMaxTables];
  Fe* out[zkc::kComposedMaxTables];  // the folded tables (k_composed_round)
  uint8_t factors[zkc::kComposedMaxTerms * zkc::kComposedMaxDegree];  // term-major, D per term
  uint8_t store[zkc::kComposedMaxTerms];   // bit d: factor d of the term stores its table's fold
  uint8_t unused[zkc::kComposedMaxTables];  // tables no term names
  uint32_t nterms, nunused;
};

// Factor d of term t at pair j (d a template parameter: `prod` and `acc` are
// only ever indexed by constants), then the factors after it. FOLD: the tables
// are the previous round's (4h elements), folded by the challenge whose
// constants are ct into out (2h) on the way.
template <class F, int D, bool FOLD, int d>
__device__ __forceinline__ void composed_factor(const ComposedArgs& a, uint32_t t, uint64_t j, uint64_t h,
                                                const Fe (&ct)[10], Fe (&prod)[D + 1], Wide (&acc)[D + 1]) {
  const uint32_t i = a.factors[t * D + d];
  const Fe* __restrict__ X = a.in[i];
  Fe lo, hi;
  if constexpr (FOLD) {
    const Fe x0 = ld_fe(X, j), x1 = ld_fe(X, j + h), x2 = ld_fe(X, j + 2 * h), x3 = ld_fe(X, j + 3 * h);
    lo = fold1c<F, 0>(x0, x2, ct);
    hi = fold1c<F, 0>(x1, x3, ct);
    if ((a.store[t] >> d) & 1u) {
      st_fe(a.out[i], j, lo);
      st_fe(a.out[i], j + h, hi);
    }
  } else {
    lo = ld_fe(X, j);
    hi = ld_fe(X, j + h);
  }
  const Fe diff = fe_sub<F>(hi, lo);
  Fe v = lo;
#pragma unroll
  for (int p = 0; p <= D; ++p) {
    if (p) v = fe_add<F>(v, diff);  // the factor at point p: the one at p - 1 plus (hi - lo)
    if constexpr (d + 1 == D) wide_mac<F>(acc[p], d ? prod[p] : fe_one<F>(), v);
    else prod[p] = d ? fe_mul<F>(prod[p], v) : v;
  }
  if constexpr (d + 1 < D) composed_factor<F, D, FOLD, d + 1>(a, t, j, h, ct, prod, acc);
}

// One pair's contribution to the D + 1 accumulators.
template <class F, int D, bool FOLD>
__device__ __forceinline__ void composed_pair(const ComposedArgs& a, uint64_t j, uint64_t h, const Fe (&ct)[10],
                                              Wide (&acc)[D + 1]) {
#pragma unroll 1
  for (uint32_t t = 0; t < a.nterms; ++t) {
    Fe prod[D + 1];
    composed_factor<F, D, FOLD, 0>(a, t, j, h, ct, prod, acc);
  }
  if constexpr (FOLD) {
#pragma unroll 1
    for (uint32_t u = 0; u < a.nunused; ++u) {
      const uint32_t i = a.unused[u];
      const Fe* __restrict__ X = a.in[i];
      const Fe x0 = ld_fe(X, j), x1 = ld_fe(X, j + h), x2 = ld_fe(X, j + 2 * h), x3 = ld_fe(X, j + 3 * h);
      st_fe(a.out[i], j, fold1c<F, 0>(x0, x2, ct));
      st_fe(a.out[i], j + h, fold1c<F, 0>(x1, x3, ct));
    }
  }
}

template <int D, class Sc>
__device__ __forceinline__ void composed_finish(const Wide (&acc)[D + 1], Sc& sc, const RoundSink& sink) {
#pragma unroll
  for (int p = 0; p <= D; ++p) block_limb_sums(acc[p], sc, 17 * p);
  __syncthreads();
  grid_finish<17 * (D + 1)>(sc, sink);
}

// Round 0: y_p = sum_j f(p, j) for p = 0..D over the input tables (2h elements each).
template <class F, int D>
__global__ __launch_bounds__(kBlock) void k_composed_round0(const ComposedArgs a, uint64_t h, RoundSink sink) {
  Wide acc[D + 1];
#pragma unroll
  for (int p = 0; p <= D; ++p) acc[p] = wide_zero<F>();
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  __shared__ Fe none[10];  // (no fold in round 0: never read)
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < h; j += step) composed_pair<F, D, false>(a, j, h, none, acc);
  __shared__ LimbScratch<17> sc;
  composed_finish<D>(acc, sc, sink);
}

// Round k >= 1, fused: every table of the previous round (4h elements) folds
// by r_{k-1} into out (2h; out never aliases in: the host ping-pongs two
// workspaces) and this round's D + 1 sums are taken on the folded values.
template <class F, int D>
__global__ __launch_bounds__(kBlock) void k_composed_round(const ComposedArgs a, uint64_t h, RoundIn rin, RoundSink sink) {
  const Fe r = block_get_r(rin);
  __shared__ Fe ct[10];  // the fold by a round-constant challenge from its constant table (kernels.hpp fold1c), as k_gkr_round
  fold_consts<F, 1>(r, r, r, ct);
  Wide acc[D + 1];
#pragma unroll
  for (int p = 0; p <= D; ++p) acc[p] = wide_zero<F>();
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < h; j += step) composed_pair<F, D, true>(a, j, h, ct, acc);
  __shared__ LimbScratch<17> sc;
  composed_finish<D>(acc, sc, sink);
}

}  // namespace zk
