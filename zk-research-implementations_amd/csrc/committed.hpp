// gfx950 kernel of the committed sum-check: the linear
// combination of up to 16 tables, out[j] = sum_i coeff[i] table_i[j] + constant,
// which turns k openings at one point into one (kzg.hip kzg_batch_open) and is
// public as zk_dev_mle_lincomb (committed.hip). Included by both.
//
// One thread per element, grid-stride. It is a pure stream: every input element
// is read once, every output written once, 32 (ntables + 1) bytes per element.
// The table count is run-time data, so nothing indexed by it may live in
// registers (a run-time-indexed register array goes to scratch): the table
// pointers and the Montgomery coefficients sit in the kernel-argument segment,
// as k_composed_round keeps its shape data, and are read with uniform (scalar)
// loads; a thread holds one loaded element and one accumulator.
// The products are summed unreduced in one Wide (17 words = 544 bits) by
// wide_mac and reduced once per element by wide_redc. With every factor < p the
// sum of ntables products is < 16 p^2 < 2^514 for all three fields (p < 2^255:
// BLS12-381 Fr is the largest, 2^254.9), well inside the 544 bits; that bound
// is why ntables is capped at 16 (committed_plan.hpp kLincombMaxTables). The
// constant is added after the reduction.
#pragma once
#include "committed_plan.hpp"
#include "host.hpp"
#include "kernels.hpp"

namespace zk {

struct LincombArgs {
  const Fe* in[zkc::kLincombMaxTables];
  Fe coeff[zkc::kLincombMaxTables];  // Montgomery
  Fe constant;                       // Montgomery
  uint32_t ntables;
};

// out never aliases an input (the callers check): the inputs may repeat.
template <class F>
__global__ __launch_bounds__(kBlock) void k_lincomb(const LincombArgs a, uint64_t n, Fe* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
    Wide acc = wide_zero<F>();
#pragma unroll 1
    for (uint32_t i = 0; i < a.ntables; ++i) wide_mac<F>(acc, a.coeff[i], ld_fe(a.in[i], j));
    st_fe(out, j, fe_add<F>(wide_redc<F>(acc), a.constant));
  }
}

}  // namespace zk

namespace zkh {
// out[j] = sum_i coeffs[i] tables[i][j] + constant over n elements (Montgomery
// throughout; 1 <= ntables <= kLincombMaxTables, out distinct from every table)
template <class F>
void launch_lincomb(zk_ctx* c, const Fe* const* tables, uint32_t ntables, const Fe* coeffs, const Fe& constant,
                    uint64_t n, Fe* out) {
  zk::LincombArgs a{};
  for (uint32_t i = 0; i < ntables; ++i) {
    a.in[i] = tables[i];
    a.coeff[i] = coeffs[i];
  }
  a.constant = constant;
  a.ntables = ntables;
  launch(c, ZK_K_FOLD, 32.0 * (ntables + 1) * n, (double)ntables * n, zk::k_lincomb<F>,
         grid_for(c, n, zk::k_lincomb<F>), a, n, out);
}
}  // namespace zkh
