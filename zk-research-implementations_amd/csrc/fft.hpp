// Radix-2 NTT over the scalar fields on gfx950 (fft/src/fft.rs): the pass
// kernel of the Stockham plan in fft_plan.hpp and the small kernels of
// zk_poly_mul. Tables are Montgomery images, 32 B per element.
//
// A pass with 2^a-point tile DFTs: a block takes a tile of R = 2^a rows of
// C = 2^log_c consecutive elements (row r, column j: x[j + r n/R]), scales
// them by the inter-pass twiddle on the way into LDS, runs the a radix-2
// stages there (decimation in frequency, in place: X[k] ends in row
// bitrev(k)), and stores X[k] of column j to (j / Ns) Ns R + (j mod Ns) + k Ns.
// Loads walk the tile row by row (runs of C elements); stores walk the output
// addresses in order (runs of min(C, Ns) R or C elements) and fetch their
// element from the bit-reversed row, so the permutation costs LDS reads only.
#pragma once
#include "fft_plan.hpp"
#include "field.hpp"
#include "kernels.hpp"

namespace zk {

// What one pass needs besides its input and output tables.
struct FftPass {
  uint64_t n;       // elements
  uint32_t m;       // log2 n
  uint32_t a;       // stages of this pass (R = 2^a rows)
  uint32_t log_ns;  // log2 Ns (0: no twiddle)
  uint32_t log_c;   // log2 C
  uint32_t log_w;   // stage_roots[t] = w_n^(t n / 2^log_w), t < 2^(log_w - 1)
  uint32_t h;       // twiddle split: w_n^e = hi[e >> h] lo[e & (2^h - 1)]
  uint32_t scale;   // inverse with one pass: multiply by n_inv on the way in
  const Fe* stage_roots;
  const Fe* hi;
  const Fe* lo;  // (the last pass of an inverse: lo[i] n^-1)
  Fe n_inv;
};

// LDS tile: two planes of 16-byte halves (an element's low and high four
// limbs), one b128 access each; four padding slots per 64 elements keep the
// bit-reversed rows of the store phase in different banks. (Eight planes of
// 32-bit limbs measured 1.3 % slower: DESIGN.md 6f.)
constexpr uint32_t kFftTileElems = 1u << zkh::kFftTileElemsLog;
__device__ __forceinline__ uint32_t fft_slot(uint32_t e) { return e + ((e >> 6) << 2); }
constexpr uint32_t kFftSlots = kFftTileElems + (kFftTileElems >> 6) * 4;
struct FftTile {
  uint4 w[2][kFftSlots];
  __device__ __forceinline__ Fe get(uint32_t e) const {
    const uint32_t s = fft_slot(e);
    const uint4 a = w[0][s], b = w[1][s];
    Fe r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
  }
  __device__ __forceinline__ void put(uint32_t e, const Fe& x) {
    const uint32_t s = fft_slot(e);
    w[0][s] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    w[1][s] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
  }
};

// One pass (dft :6-29, a of its recursion levels at once). INV only selects
// the single-pass inverse's n^-1; the direction itself is in the tables.
// Grid-stride over the n / (R C) tiles. `in` may equal `out` only when the
// whole transform is one tile (one block reads everything before it writes).
template <class F, bool INV>
__global__ __launch_bounds__(kBlock) void k_fft_pass(const Fe* in, Fe* out, const FftPass p) {
  __shared__ FftTile tile;
  const uint32_t t = threadIdx.x;
  const uint32_t a = p.a, log_c = p.log_c, log_ns = p.log_ns;
  const uint32_t E = 1u << (a + log_c), C = 1u << log_c, R = 1u << a;
  const uint64_t row_stride = p.n >> a, ns_mask = ((uint64_t)1 << log_ns) - 1;
  const uint64_t tiles = p.n >> (a + log_c);
  const uint32_t log_l = log_c < log_ns ? log_c : log_ns;  // store runs: 2^log_l columns
  for (uint64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const uint64_t j0 = tl << log_c;
    // ---- load (+ inter-pass twiddle) ----
    for (uint32_t e = t; e < E; e += kBlock) {
      const uint32_t jj = e & (C - 1), r = e >> log_c;
      Fe x = ld_fe(in, j0 + jj + r * row_stride);
      if (log_ns > 0) {
        const uint64_t jm = (j0 + jj) & ns_mask;
        const uint64_t ex = ((uint64_t)r * jm) << (p.m - log_ns - a);  // < n
        const Fe tw = fe_mul<F>(ld_fe(p.hi, ex >> p.h), ld_fe(p.lo, ex & (((uint64_t)1 << p.h) - 1)));
        x = fe_mul<F>(x, tw);
      } else if (INV && p.scale) {
        x = fe_mul<F>(x, p.n_inv);
      }
      tile.put(e, x);
    }
    __syncthreads();
    // ---- a radix-2 stages, decimation in frequency ----
    for (int s = (int)a - 1; s >= 0; --s) {
      const uint32_t half = 1u << s;
      for (uint32_t b = t; b < E / 2; b += kBlock) {
        const uint32_t jj = b & (C - 1), rr = b >> log_c;
        const uint32_t i = rr & (half - 1);
        const uint32_t r = ((rr >> s) << (s + 1)) | i;
        const uint32_t e0 = (r << log_c) | jj, e1 = e0 + (half << log_c);
        const Fe x = tile.get(e0), y = tile.get(e1);
        tile.put(e0, fe_add<F>(x, y));
        Fe d = fe_sub<F>(x, y);
        if (s > 0) d = fe_mul<F>(d, ld_fe(p.stage_roots, (uint64_t)i << (p.log_w - s - 1)));  // (s = 0: the root is 1)
        tile.put(e1, d);
      }
      __syncthreads();
    }
    // ---- store, in output address order ----
    for (uint32_t o = t; o < E; o += kBlock) {
      const uint32_t jlo = o & ((1u << log_l) - 1);
      const uint32_t k = (o >> log_l) & (R - 1);
      const uint32_t jhi = o >> (log_l + a);
      const uint32_t jj = (jhi << log_l) | jlo;
      const uint64_t j = j0 + jj;
      const uint32_t row = a ? (__brev(k) >> (32 - a)) : 0;
      const uint64_t dst = ((j >> log_ns) << (log_ns + a)) + (j & ns_mask) + ((uint64_t)k << log_ns);
      st_fe(out, dst, tile.get((row << log_c) | jj));
    }
    __syncthreads();  // the tile is reused by the next trip
  }
}

// zk_poly_mul: dst[i] = src[i] (i < n_src), 0 up to n  (Montgomery 0 is 0)
__global__ __launch_bounds__(kBlock) void k_fft_copy_pad(const Fe* src, uint64_t n_src, Fe* dst, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  Fe z;
#pragma unroll
  for (int k = 0; k < 8; ++k) z.v[k] = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) st_fe(dst, i, i < n_src ? ld_fe(src, i) : z);
}
// a[i] *= b[i]
template <class F>
__global__ __launch_bounds__(kBlock) void k_fft_pointwise(Fe* a, const Fe* b, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const Fe x = ld_fe(a, i), y = ld_fe(b, i);
    st_fe(a, i, fe_mul<F>(x, y));
  }
}

}  // namespace zk
