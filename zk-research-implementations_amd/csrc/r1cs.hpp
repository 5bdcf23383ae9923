// gfx950 kernels of the R1CS prover (device code; included by r1cs.hip). Both
// matrix passes of DESIGN.md 6k are one computation: the entries of A, B and C
// together are grouped by a key (r1cs_plan.hpp r1cs_group, the wired prover's
// counting sort and chunk cut), each entry carrying its other index and a 2-bit
// matrix tag in one word; a thread walks one chunk of at most kWiredChunk
// entries, gathers x[other] and accumulates value * x[other] unreduced into the
// accumulator its tag selects, one REDC per accumulator at the end.
//   by rows:    key = row,    x = z,          the sums are (Az, Bz, Cz)[row];
//   by columns: key = column, x = eq(rx, .),  the sums are the three matrices
//               bound to rx at that column, kept apart (the verifier's matrix
//               evaluation) or combined as a + rho b + rho^2 c (the prover's M).
// The values are stored once per grouping, Montgomery, in grouping order: a
// thread streams its own values and reads only x at random (32-byte gathers,
// latency- and occupancy-bound as wired.hpp's).
//
// The accumulator bound: a chunk holds at most 256 entries, every product is
// below p^2, so a sum is below 256 p^2 < 2^8 2^510 = 2^518 for the largest
// modulus (p < 2^255), inside Wide's 544 bits; k_wired_phase1 relies on the
// same bound.
//
// A row pass zeroes every row first (rows without entries stay zero); chunks of
// split rows go to partial-sum slots and a combining pass, one block per split
// row, adds them. Every store is a vector store (st_fe).
#pragma once
#include "r1cs_plan.hpp"
#include "wired.hpp"

namespace zk {

static_assert(zkw::kWiredChunk == 256, "the Wide accumulators hold 256 products (see above)");

// out_k[j] = 0 for j < n in the NC columns
template <class F, int NC>
__global__ __launch_bounds__(kBlock) void k_r1cs_zero(uint32_t n, Fe* __restrict__ o0, Fe* __restrict__ o1,
                                                      Fe* __restrict__ o2) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  st_fe(o0, j, fe_zero<F>());
  if (NC == 3) {
    st_fe(o1, j, fe_zero<F>());
    st_fe(o2, j, fe_zero<F>());
  }
}

// One thread per chunk. val[i], other[i]: the entries in grouping order.
// NC = 3: the three sums to (o0, o1, o2)[row], or, for a chunk of a split row,
// to slot ci - nsingle of (p0, p1, p2). NC = 1: a + rho b + rho^2 c to o0 / p0
// (the combination is linear, so the slots of a split row still add up to it).
template <class F, int NC>
__global__ __launch_bounds__(kBlock) void k_r1cs_gather(const Fe* __restrict__ x, const Fe* __restrict__ val,
                                                        const uint32_t* __restrict__ other,
                                                        const WiredChunk* __restrict__ chunks, uint32_t nchunks,
                                                        uint32_t nsingle, Fe rho, Fe rho2, Fe* __restrict__ o0,
                                                        Fe* __restrict__ o1, Fe* __restrict__ o2, Fe* __restrict__ p0,
                                                        Fe* __restrict__ p1, Fe* __restrict__ p2) {
  const uint32_t ci = blockIdx.x * kBlock + threadIdx.x;
  if (ci >= nchunks) return;
  const WiredChunk ch = chunks[ci];
  Wide a = wide_zero<F>(), b = wide_zero<F>(), c = wide_zero<F>();
  for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {  // count <= 256: each sum < 256 p^2 < 2^518
    const uint32_t o = other[i];
    const Fe v = ld_fe(val, i), xo = ld_fe(x, o & zkr::kR1csIndexMask);
    const uint32_t tag = o >> zkr::kR1csTagShift;
    if (tag == 0) wide_mac<F>(a, v, xo);
    else if (tag == 1) wide_mac<F>(b, v, xo);
    else wide_mac<F>(c, v, xo);
  }
  const Fe sa = wide_redc<F>(a), sb = wide_redc<F>(b), sc = wide_redc<F>(c);
  const bool whole = ci < nsingle;
  const uint32_t at = whole ? ch.row : ci - nsingle;
  if (NC == 1) {
    const Fe m = fe_add<F>(sa, fe_add<F>(fe_mul<F>(rho, sb), fe_mul<F>(rho2, sc)));
    st_fe(whole ? o0 : p0, at, m);
  } else {
    st_fe(whole ? o0 : p0, at, sa);
    st_fe(whole ? o1 : p1, at, sb);
    st_fe(whole ? o2 : p2, at, sc);
  }
}

// Combining pass: block r adds the slots of split row r in the NC columns
// (k_wired_combine is written for two).
template <class F, int NC>
__global__ __launch_bounds__(kBlock) void k_r1cs_combine(const WiredChunk* __restrict__ split,
                                                         const Fe* __restrict__ p0, const Fe* __restrict__ p1,
                                                         const Fe* __restrict__ p2, Fe* __restrict__ o0,
                                                         Fe* __restrict__ o1, Fe* __restrict__ o2) {
  __shared__ Fe sh[kBlock];
  const WiredChunk s = split[blockIdx.x];  // (row, first slot, slots)
  const Fe* const p[3] = {p0, p1, p2};
  Fe* const o[3] = {o0, o1, o2};
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    Fe x = fe_zero<F>();
    for (uint32_t i = threadIdx.x; i < s.count; i += kBlock) x = fe_add<F>(x, ld_fe(p[k], s.first + i));
    const Fe sum = wired_block_sum<F>(x, sh);
    if (threadIdx.x == 0) st_fe(o[k], s.row, sum);
    __syncthreads();  // sh is reused by the next column
  }
}

}  // namespace zk
