// gfx950 kernels of the wired GKR prover (device code; included by wired.hip).
// A wired layer (wired_plan.hpp) has G gates (op, left, right) over a value
// table w of 2^kb entries and a gate weight wt_g. The layer's sum-check runs in
// the same two phases over tables of 2^kb entries as the tree prover
// (kernels.hpp k_phase1_tables / k_phase2_tables), for any wiring:
//   phase 1 (b):  W(b) = w(b),  U(b) = sum_{left_g = b} wt_g (Add ? 1 : w(right_g)),
//                 V(b) = sum_{left_g = b, Add} wt_g w(right_g),  ONE(b) = 1,
//     so that sum_c f(b, c) = W U + V ONE;
//   phase 2 (c), b bound to u = r_b:  A(c) = sum_{right_g = c, Add} wt_g eq(u, left_g),
//                 M(c) likewise over Mul,  S(c) = w(u) + w(c),  P(c) = w(u) w(c).
// The sums are gathers through the layer's two gate groupings: 32-byte random
// reads of wt, w and eq, latency- and occupancy-bound. A row pass writes the
// table columns that need no wiring and zeroes the other two; a chunk pass, one
// thread per chunk of at most kWiredChunk gates, accumulates the products
// unreduced (wide_mac, one REDC per sum) and writes whole rows into the table
// and the chunks of split rows into partial-sum slots; a combining pass, one
// block per split row, adds a row's slots. Every store is a vector store.
#pragma once
#include "kernels.hpp"
#include "wired_plan.hpp"

namespace zk {

using zkw::WiredChunk;

constexpr uint32_t kWiredOpBit = 1u << 31;  // `other` entries: the gate's second wire, its op in the top bit

// out[g] = in[left_g] op in[right_g] for g < G, zero up to the padded length n2
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_layer(const Fe* __restrict__ in, const uint8_t* __restrict__ ops,
                                                        const uint32_t* __restrict__ left,
                                                        const uint32_t* __restrict__ right, uint32_t G, uint32_t n2,
                                                        Fe* __restrict__ out) {
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= n2) return;
  Fe r = fe_zero<F>();
  if (g < G) {
    const Fe a = ld_fe(in, left[g]), b = ld_fe(in, right[g]);
    r = ops[g] ? fe_mul<F>(a, b) : fe_add<F>(a, b);
  }
  st_fe(out, g, r);
}

// eq(pt, .) by doubling, MSB first (host_eq_table): entry j of the table over
// the first k coordinates becomes entries 2j (times 1 - pt[k]) and 2j + 1
// (times pt[k]). One pass applies S <= 3 coordinates: a thread takes entry j
// of `src` (nullptr: the empty product, 1) and writes its 2^S descendants,
// contiguous at j 2^S. src and dst are distinct buffers.
struct EqPts {
  Fe r[3];
};
template <class F, int S>
__global__ __launch_bounds__(kBlock) void k_eq_table(const Fe* __restrict__ src, uint32_t nsrc, const EqPts pts,
                                                     Fe* __restrict__ dst) {
  static_assert(S >= 1 && S <= 3, "a pass applies 1 to 3 coordinates");
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= nsrc) return;
  Fe t[1 << S];
  t[0] = src ? ld_fe(src, j) : fe_one<F>();
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const Fe rk = pts.r[k];
#pragma unroll
    for (int i = (1 << k) - 1; i >= 0; --i) {  // (descending: t[2i], t[2i+1] overwrite nothing still to be read)
      const Fe x = fe_mul<F>(t[i], rk);
      t[2 * i] = fe_sub<F>(t[i], x);
      t[2 * i + 1] = x;
    }
  }
#pragma unroll
  for (int i = 0; i < (1 << S); ++i) st_fe(dst, ((uint64_t)j << S) + i, t[i]);
}

// wt_g = alpha eqb[g] + beta eqc[g] (has_c = 0: alpha eqb[g], the output layer's eq(r0, g))
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_weights(const Fe* __restrict__ eqb, const Fe* __restrict__ eqc,
                                                          Fe alpha, Fe beta, uint32_t has_c, uint32_t G,
                                                          Fe* __restrict__ wt) {
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= G) return;
  Fe x = fe_mul<F>(alpha, ld_fe(eqb, g));
  if (has_c) x = fe_add<F>(x, fe_mul<F>(beta, ld_fe(eqc, g)));
  st_fe(wt, g, x);
}

// Row passes over the L = 2^kb table rows: the columns that need no wiring, zero in the two that do.
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_rows1(const Fe* __restrict__ w, uint32_t L, Fe* __restrict__ W,
                                                        Fe* __restrict__ U, Fe* __restrict__ V,
                                                        Fe* __restrict__ ONE) {
  const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= L) return;
  st_fe(W, b, ld_fe(w, b));
  st_fe(U, b, fe_zero<F>());
  st_fe(V, b, fe_zero<F>());
  st_fe(ONE, b, fe_one<F>());
}
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_rows2(const Fe* __restrict__ w, uint32_t L, Fe wrb,
                                                        Fe* __restrict__ A, Fe* __restrict__ S, Fe* __restrict__ M,
                                                        Fe* __restrict__ P) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= L) return;
  const Fe wc = ld_fe(w, c);
  st_fe(A, c, fe_zero<F>());
  st_fe(S, c, fe_add<F>(wrb, wc));
  st_fe(M, c, fe_zero<F>());
  st_fe(P, c, fe_mul<F>(wrb, wc));
}

// Where a chunk's two sums go: its table row, or (split rows) its slot.
__device__ __forceinline__ void wired_put(uint32_t ci, uint32_t nsingle, uint32_t row, const Fe& x, const Fe& y,
                                          Fe* __restrict__ X, Fe* __restrict__ Y, Fe* __restrict__ px,
                                          Fe* __restrict__ py) {
  if (ci < nsingle) {
    st_fe(X, row, x);
    st_fe(Y, row, y);
  } else {
    st_fe(px, ci - nsingle, x);
    st_fe(py, ci - nsingle, y);
  }
}

// Phase 1, grouped by left: gate[i] the gate ids, other[i] = right | op << 31.
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_phase1(const Fe* __restrict__ w, const Fe* __restrict__ wt,
                                                         const uint32_t* __restrict__ gate,
                                                         const uint32_t* __restrict__ other,
                                                         const WiredChunk* __restrict__ chunks, uint32_t nchunks,
                                                         uint32_t nsingle, Fe* __restrict__ U, Fe* __restrict__ V,
                                                         Fe* __restrict__ pu, Fe* __restrict__ pv) {
  const uint32_t ci = blockIdx.x * kBlock + threadIdx.x;
  if (ci >= nchunks) return;
  const WiredChunk ch = chunks[ci];
  const Fe one = fe_one<F>(), zero = fe_zero<F>();
  Wide u = wide_zero<F>(), v = wide_zero<F>();
  for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
    const uint32_t o = other[i];
    const bool mul = (o & kWiredOpBit) != 0;
    const Fe x = ld_fe(wt, gate[i]), wr = ld_fe(w, o & ~kWiredOpBit);
    wide_mac<F>(u, x, mul ? wr : one);
    wide_mac<F>(v, mul ? zero : x, wr);
  }
  wired_put(ci, nsingle, ch.row, wide_redc<F>(u), wide_redc<F>(v), U, V, pu, pv);
}

// Phase 2, grouped by right: other[i] = left | op << 31, eqb = eq(r_b, .) over the table rows.
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_phase2(const Fe* __restrict__ eqb, const Fe* __restrict__ wt,
                                                         const uint32_t* __restrict__ gate,
                                                         const uint32_t* __restrict__ other,
                                                         const WiredChunk* __restrict__ chunks, uint32_t nchunks,
                                                         uint32_t nsingle, Fe* __restrict__ A, Fe* __restrict__ M,
                                                         Fe* __restrict__ pa, Fe* __restrict__ pm) {
  const uint32_t ci = blockIdx.x * kBlock + threadIdx.x;
  if (ci >= nchunks) return;
  const WiredChunk ch = chunks[ci];
  const Fe zero = fe_zero<F>();
  Wide a = wide_zero<F>(), m = wide_zero<F>();
  for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
    const uint32_t o = other[i];
    const bool mul = (o & kWiredOpBit) != 0;
    const Fe x = ld_fe(wt, gate[i]), e = ld_fe(eqb, o & ~kWiredOpBit);
    wide_mac<F>(a, mul ? zero : x, e);
    wide_mac<F>(m, mul ? x : zero, e);
  }
  wired_put(ci, nsingle, ch.row, wide_redc<F>(a), wide_redc<F>(m), A, M, pa, pm);
}

// Sum of one element per thread over the block (valid in thread 0).
template <class F>
__device__ __forceinline__ Fe wired_block_sum(Fe x, Fe (&sh)[kBlock]) {
  const uint32_t t = threadIdx.x;
  sh[t] = x;
  __syncthreads();
  for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] = fe_add<F>(sh[t], sh[t + s]);
    __syncthreads();
  }
  return sh[0];
}

// Combining pass: block r adds the slots of split row r, in both columns.
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_combine(const WiredChunk* __restrict__ split,
                                                          const Fe* __restrict__ px, const Fe* __restrict__ py,
                                                          Fe* __restrict__ X, Fe* __restrict__ Y) {
  __shared__ Fe sh[kBlock];
  const WiredChunk s = split[blockIdx.x];  // (row, first slot, slots)
  Fe x = fe_zero<F>(), y = fe_zero<F>();
  for (uint32_t i = threadIdx.x; i < s.count; i += kBlock) {
    x = fe_add<F>(x, ld_fe(px, s.first + i));
    y = fe_add<F>(y, ld_fe(py, s.first + i));
  }
  const Fe sx = wired_block_sum<F>(x, sh);
  __syncthreads();
  const Fe sy = wired_block_sum<F>(y, sh);
  if (threadIdx.x == 0) {
    st_fe(X, s.row, sx);
    st_fe(Y, s.row, sy);
  }
}

// sum_j w[j] e[j] over n entries: block b's part, reduced, in out[b] (the host adds the few parts).
// With e = eq(r, .) this is w(r), for tables of any length (k_mle_eval2 stops at 2^14).
template <class F>
__global__ __launch_bounds__(kBlock) void k_wired_dot(const Fe* __restrict__ w, const Fe* __restrict__ e, uint64_t n,
                                                      Fe* __restrict__ out) {
  __shared__ Fe sh[kBlock];
  Wide acc = wide_zero<F>();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride)
    wide_mac<F>(acc, ld_fe(w, j), ld_fe(e, j));
  const Fe s = wired_block_sum<F>(wide_redc<F>(acc), sh);
  if (threadIdx.x == 0) st_fe(out, blockIdx.x, s);
}

}  // namespace zk
