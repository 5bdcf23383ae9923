// gfx950 kernels of the lookup argument, included by lookup.hip:
// the batched field inversion, the multiplicity count (a probe into the
// handle's open-addressing table with vector atomics on 32-bit counters) and
// the three small streams the helper columns need.
//
// k_batch_inverse: Montgomery's trick, one Fermat power per run of
// kBatchInvRun = 64 elements, every lane of the wave inverting a product of its
// own, so no lane idles through the power: 1 product per element going up,
// 380 / 64 for the power, 2 coming down. A wave owns 64 * 64 consecutive
// elements and lane l takes l, l + 64, l + 128 ..: each access of the wave is
// one contiguous 2 KiB. The running products are not held in registers (64
// elements would be 512 VGPRs) but stored in `pre` and read back on the way
// down: `pre` is `out` itself when out is not in, a scratch table when it is.
// No LDS, no barrier; a lane holds three elements at a time.
//   up:    acc_k = a_0 .. a_k with a_k = in_k, or 1 where in_k = 0;  pre_k = acc_k
//   power: inv = acc_(len-1)^-1
//   down:  k = len-1 .. 1:  out_k = inv * pre_(k-1);  inv = inv * a_k;  out_0 = inv
// with out_k = 0 where in_k = 0. Step k of the way down reads in_k and
// pre_(k-1) before it writes out_k, and no later step reads index k of either:
// in == out and pre == out are both safe (the pointers carry no restrict).
#pragma once
#include "host.hpp"
#include "kernels.hpp"
#include "lookup_plan.hpp"

namespace zk {
static_assert(zkl::kBatchInvBlock == kBlock, "the launch wrapper's block is the plan's");

template <class F>
__global__ __launch_bounds__(kBlock) void k_batch_inverse(const Fe* in, Fe* pre, Fe* out, uint64_t count) {
  constexpr uint64_t W = zkl::kBatchInvWave;
  const uint64_t wave = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / W;
  const uint64_t base = wave * zkl::kBatchInvWaveTile + (threadIdx.x & (W - 1));
  if (base >= count) return;
  const uint64_t left = (count - base + W - 1) / W;  // elements of this lane's run below count
  const uint32_t len = left < zkl::kBatchInvRun ? (uint32_t)left : zkl::kBatchInvRun;
  const Fe one = fe_one<F>();
  Fe acc = one;
#pragma unroll 1
  for (uint32_t k = 0; k < len; ++k) {
    const Fe x = ld_fe(in, base + k * W);
    acc = fe_mul<F>(acc, fe_is_zero<F>(x) ? one : x);
    st_fe(pre, base + k * W, acc);
  }
  Fe inv = fe_inv<F>(acc);
#pragma unroll 1
  for (uint32_t k = len - 1; k >= 1; --k) {
    const Fe x = ld_fe(in, base + k * W);
    const Fe p = ld_fe(pre, base + (k - 1) * W);
    const bool z = fe_is_zero<F>(x);
    const Fe o = fe_mul<F>(inv, p);
    inv = fe_mul<F>(inv, z ? one : x);
    st_fe(out, base + k * W, z ? x : o);
  }
  const Fe x0 = ld_fe(in, base);
  st_fe(out, base, fe_is_zero<F>(x0) ? x0 : inv);
}

// One lane per column entry: the home slot from the low word of the canonical
// value (one product), then linear probing with the full 8-word comparison
// against the Montgomery table. At least half the slots are empty, so every
// probe ends. A hit adds 1 to its value's first index, a miss to the one
// counter behind the table's.
template <class F>
__global__ __launch_bounds__(kBlock) void k_lookup_probe(const Fe* __restrict__ f, uint64_t count,
                                                         const Fe* __restrict__ tm, const uint32_t* __restrict__ slots,
                                                         uint32_t slot_log, uint32_t* counts, uint32_t* missing) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint32_t mask = (1u << slot_log) - 1;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
    const Fe x = ld_fe(f, i);
    uint32_t s = zkl::lookup_hash(fe_from_mont<F>(x).v[0], slot_log);
    for (;; s = (s + 1) & mask) {
      const uint32_t j = slots[s];
      if (j == zkl::kLookupEmpty) {
        atomicAdd(missing, 1u);
        break;
      }
      if (fe_eq<F>(ld_fe(tm, j), x)) {
        atomicAdd(counts + j, 1u);
        break;
      }
    }
  }
}

// m[j] = the Montgomery image of counts[j] for j < T, 0 for T <= j < N
template <class F>
__global__ __launch_bounds__(kBlock) void k_lookup_counts_to_fe(const uint32_t* __restrict__ counts, uint32_t T,
                                                                Fe* __restrict__ m, uint64_t N) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += stride) {
    Fe c = fe_zero<F>();
    if (j < T) {
      c.v[0] = counts[j];
      c = fe_to_mont<F>(c);
    }
    st_fe(m, j, c);
  }
}

// out[j] = t[min(j, T - 1)] for j < N
__global__ __launch_bounds__(kBlock) void k_lookup_pad(const Fe* __restrict__ t, uint32_t T, Fe* __restrict__ out,
                                                       uint64_t N) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += stride)
    st_fe(out, j, ld_fe(t, j < T ? j : T - 1));
}

// out[j] = a[j] b[j] for j < N; out may be a or b
template <class F>
__global__ __launch_bounds__(kBlock) void k_lookup_mul(const Fe* a, const Fe* b, Fe* out, uint64_t N) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += stride)
    st_fe(out, j, fe_mul<F>(ld_fe(a, j), ld_fe(b, j)));
}

}  // namespace zk

namespace zkh {
// out[i] = in[i]^-1 over count Montgomery elements on the device; pre: the
// running products' table (out itself unless out is in).
template <class F>
void launch_batch_inverse(zk_ctx* c, const Fe* in, Fe* pre, Fe* out, uint64_t count) {
  const uint64_t waves = (count + zkl::kBatchInvWaveTile - 1) / zkl::kBatchInvWaveTile;
  const uint64_t per_block = zkl::kBatchInvBlock / zkl::kBatchInvWave;
  const uint32_t grid = (uint32_t)((waves + per_block - 1) / per_block);
  launch(c, ZK_K_LAYER, 160.0 * count, (3.0 + 380.0 / zkl::kBatchInvRun) * count, zk::k_batch_inverse<F>, grid, in, pre,
         out, count);
}
}  // namespace zkh
