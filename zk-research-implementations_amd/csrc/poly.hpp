// Univariate polynomials over arbitrary points on gfx950
// (univariate_polynomial_dense.rs evaluate :20-26, interpolate :48-74): batch
// evaluation by Horner and the three steps of the O(n^2) interpolation laid
// out in poly_plan.hpp. Tables are Montgomery images, 32 B per element; every
// global index is 64-bit; every kernel grid-strides over its tiles of kBlock
// lanes along x. No value crosses lanes and nothing is accumulated through
// atomics: what a block shares is staged in LDS and read back as a broadcast
// (the same slot in every lane) or as consecutive slots.
#pragma once
#include "field.hpp"
#include "kernels.hpp"
#include "poly_plan.hpp"

namespace zk {

static_assert(kBlock == (int)zkh::kPolyBlock, "poly_plan.hpp sizes its tiles for this block");

// N elements in LDS as two planes of 16-byte halves, one b128 access each (the
// layout fft.hpp measured faster than eight planes of limbs).
template <uint32_t N>
struct PolyLds {
  uint4 w[2][N];
  __device__ __forceinline__ Fe get(uint32_t e) const {
    const uint4 a = w[0][e], b = w[1][e];
    Fe r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
  }
  __device__ __forceinline__ void put(uint32_t e, const Fe& x) {
    w[0][e] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    w[1][e] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
  }
};

// ---------------------------------------------------------------------------
// evaluate :20-26 at m points: lane i runs Horner over the coefficients
// [y chunk_len, min(d, (y + 1) chunk_len)) of blockIdx.y = y from the top,
// kPolyEvalTile of them staged in LDS at a time, and stores cell (y, i) to
// out[y m + i]. One chunk: out is the result (no coefficients: 0).
// ---------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(kBlock) void k_poly_eval(const Fe* coeffs, uint64_t d, const Fe* xs, uint64_t m, Fe* out,
                                                      uint64_t chunk_len) {
  __shared__ PolyLds<zkh::kPolyEvalTile> cf;
  const uint32_t t = threadIdx.x;
  const uint64_t lo = (uint64_t)blockIdx.y * chunk_len;
  const uint64_t hi = d - lo < chunk_len ? d : lo + chunk_len;  // (lo <= d: the plan has ceil(d / chunk_len) chunks)
  const uint64_t tiles = (m + kBlock - 1) / kBlock;
  for (uint64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const uint64_t i = tl * kBlock + t;
    const Fe x = i < m ? ld_fe(xs, i) : fe_zero<F>();
    Fe acc = fe_zero<F>();
    for (uint64_t top = hi; top > lo;) {
      const uint64_t base = top - lo > zkh::kPolyEvalTile ? top - zkh::kPolyEvalTile : lo;
      const uint32_t cnt = (uint32_t)(top - base);
      for (uint32_t e = t; e < cnt; e += kBlock) cf.put(e, ld_fe(coeffs, base + e));
      __syncthreads();
      for (uint32_t k = cnt; k-- > 0;) acc = fe_add<F>(fe_mul<F>(acc, x), cf.get(k));
      __syncthreads();  // the stage is refilled by the next trip
      top = base;
    }
    if (i < m) st_fe(out, (uint64_t)blockIdx.y * m + i, acc);
  }
}

// out[i] = sum_c cells[c m + i] x_i^(c chunk_len): Horner in x_i^chunk_len
template <class F>
__global__ __launch_bounds__(kBlock) void k_poly_eval_combine(const Fe* cells, uint64_t m, uint32_t chunks, uint64_t chunk_len,
                                                              const Fe* xs, Fe* out) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
    const Fe x = ld_fe(xs, i);
    Fe xl = fe_one<F>();
    for (int b = 63 - __builtin_clzll(chunk_len | 1); b >= 0; --b) {  // the same exponent in every lane
      xl = fe_mul<F>(xl, xl);
      if ((chunk_len >> b) & 1) xl = fe_mul<F>(xl, x);
    }
    Fe acc = ld_fe(cells, (uint64_t)(chunks - 1) * m + i);
    for (uint32_t c = chunks - 1; c-- > 0;) acc = fe_add<F>(fe_mul<F>(acc, xl), ld_fe(cells, (uint64_t)c * m + i));
    st_fe(out, i, acc);
  }
}

// ---------------------------------------------------------------------------
// interpolate :48-74, step 1: parts[y n + i] = prod (x_i - x_j) over the j of
// blockIdx.y = y, [y part_len, min(n, (y + 1) part_len)), j != i. The x_j go
// through LDS a block at a time; every lane reads the same slot.
// ---------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(kBlock) void k_poly_weights(const Fe* xs, uint64_t n, Fe* parts, uint64_t part_len) {
  __shared__ PolyLds<kBlock> xj;
  const uint32_t t = threadIdx.x;
  const uint64_t j_lo = (uint64_t)blockIdx.y * part_len;
  const uint64_t j_hi = n - j_lo < part_len ? n : j_lo + part_len;
  const uint64_t tiles = (n + kBlock - 1) / kBlock;
  for (uint64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const uint64_t i = tl * kBlock + t;
    const Fe xi = i < n ? ld_fe(xs, i) : fe_zero<F>();
    Fe acc = fe_one<F>();
    for (uint64_t j0 = j_lo; j0 < j_hi; j0 += kBlock) {
      const uint32_t cnt = j_hi - j0 < (uint64_t)kBlock ? (uint32_t)(j_hi - j0) : (uint32_t)kBlock;
      if (t < cnt) xj.put(t, ld_fe(xs, j0 + t));
      __syncthreads();
      for (uint32_t jj = 0; jj < cnt; ++jj) {
        Fe df = fe_sub<F>(xi, xj.get(jj));
        if (j0 + jj == i) df = fe_one<F>();
        acc = fe_mul<F>(acc, df);
      }
      __syncthreads();
    }
    if (i < n) st_fe(parts, (uint64_t)blockIdx.y * n + i, acc);
  }
}

// step 2 and the leaves: d_i = prod_y parts[y n + i]; d_i = 0 (two equal x)
// raises *dup; leaf i of the tree is (M, N) = (-x_i, y_i / d_i).
template <class F>
__global__ __launch_bounds__(kBlock) void k_poly_leaves(const Fe* parts, uint32_t nparts, const Fe* xs, const Fe* ys, uint64_t n,
                                                        Fe* M, Fe* N, uint32_t* dup) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    Fe dd = ld_fe(parts, i);
    for (uint32_t q = 1; q < nparts; ++q) dd = fe_mul<F>(dd, ld_fe(parts, (uint64_t)q * n + i));
    if (fe_is_zero<F>(dd)) *dup = 1u;  // (every lane that sees it stores the same word)
    st_fe(N, i, fe_mul<F>(ld_fe(ys, i), fe_inv<F>(dd)));
    st_fe(M, i, fe_sub<F>(fe_zero<F>(), ld_fe(xs, i)));
  }
}

// ---------------------------------------------------------------------------
// step 3, one level: nodes of len = 2^log_len points pair up. For the pair at
// offset `off` with a = len and b <= len points, output k < a + b is
//   M[k] = sum_{i + j = k} Ml[i] Mr[j] + Mr[k - a] + Ml[k - b]
//   N[k] = sum_{i + j = k} (Nl[i] Mr[j] + Nr[j] Ml[i]) + Nr[k - a] + Nl[k - b]
// (i < a, j < b; the single terms are the products with the implicit leading
// 1 of Ml and Mr, present where their index is in range). One lane per output;
// the sums are accumulated unreduced and reduced once. A last node without a
// sibling is copied.
//   2 len <= kBlock: a block's outputs are whole pairs; their operands are the
//     same kBlock slots of the input level, staged once.
//   2 len >  kBlock: a block's outputs k0 .. k0 + kBlock - 1 belong to one pair;
//     it walks the left operand in steps of T = kPolyTreeTile coefficients
//     i0 .. i0 + T - 1 and stages, with them, the window of the right operand
//     they meet, j = k0 - i0 - (T - 1) .. k0 - i0 + kBlock - 1, zero where i or j
//     is out of range: lane t then reads slot t + T - 1 - e for left slot e.
//     With gridDim.y = S > 1 (poly_tree_split) the steps are dealt round robin
//     over blockIdx.y: each part stores its reduced partial sums to Mpart /
//     Npart [y n + g], and k_poly_tree_combine adds them and the single terms.
// ---------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(kBlock) void k_poly_tree_level(const Fe* Min, const Fe* Nin, Fe* Mout, Fe* Nout, uint64_t n,
                                                            uint32_t log_len, Fe* Mpart, Fe* Npart) {
  constexpr uint32_t T = zkh::kPolyTreeTile, W = T + kBlock;
  __shared__ PolyLds<T> ml, nl;
  __shared__ PolyLds<W> mr, nr;
  const uint32_t t = threadIdx.x;
  const uint64_t len = (uint64_t)1 << log_len;
  const uint64_t tiles = (n + kBlock - 1) / kBlock;
  for (uint64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const uint64_t g0 = tl * kBlock, g = g0 + t;
    if (2 * len <= (uint64_t)kBlock) {
      if (g < n) {
        mr.put(t, ld_fe(Min, g));
        nr.put(t, ld_fe(Nin, g));
      }
      __syncthreads();
      if (g < n) {
        const uint64_t off = (g >> (log_len + 1)) << (log_len + 1);  // >= g0: 2 len divides kBlock
        const uint64_t rem = n - off;
        Fe m_out, n_out;
        if (rem <= len) {  // no sibling
          m_out = mr.get(t);
          n_out = nr.get(t);
        } else {
          const uint32_t a = (uint32_t)len, b = rem - len < len ? (uint32_t)(rem - len) : (uint32_t)len;
          const uint32_t k = (uint32_t)(g - off), lb = (uint32_t)(off - g0), rb = lb + a;
          Wide wm = wide_zero<F>(), wn = wide_zero<F>();
          const uint32_t i_lo = k >= b ? k - b + 1 : 0, i_hi = k < a ? k + 1 : a;
          for (uint32_t i = i_lo; i < i_hi; ++i) {
            const Fe l_m = mr.get(lb + i), l_n = nr.get(lb + i), r_m = mr.get(rb + k - i), r_n = nr.get(rb + k - i);
            wide_mac<F>(wm, l_m, r_m);
            wide_mac<F>(wn, l_n, r_m);
            wide_mac<F>(wn, r_n, l_m);
          }
          m_out = wide_redc<F>(wm);
          n_out = wide_redc<F>(wn);
          if (k >= a) {  // (k - a < b: k < a + b)
            m_out = fe_add<F>(m_out, mr.get(rb + k - a));
            n_out = fe_add<F>(n_out, nr.get(rb + k - a));
          }
          if (k >= b && k - b < a) {
            m_out = fe_add<F>(m_out, mr.get(lb + k - b));
            n_out = fe_add<F>(n_out, nr.get(lb + k - b));
          }
        }
        st_fe(Mout, g, m_out);
        st_fe(Nout, g, n_out);
      }
      __syncthreads();
    } else {
      const uint64_t off = (g0 >> (log_len + 1)) << (log_len + 1);  // the whole tile lies in this pair: kBlock divides 2 len
      const uint64_t rem = n - off;
      const uint32_t S = gridDim.y, y = blockIdx.y;
      if (rem <= len) {  // no sibling (block-uniform)
        if (g < n && y == 0) {
          st_fe(Mout, g, ld_fe(Min, g));
          st_fe(Nout, g, ld_fe(Nin, g));
        }
        continue;
      }
      const uint64_t a = len, b = rem - len < len ? rem - len : len;
      const uint64_t k0 = g0 - off, k = k0 + t;
      const uint64_t i_min = k0 >= b ? k0 - b + 1 : 0, i_end = k0 + kBlock < a ? k0 + kBlock : a;  // [i_min, i_end)
      Wide wm = wide_zero<F>(), wn = wide_zero<F>();
      uint32_t q = 0;
      for (uint64_t i0 = i_min; i0 < i_end; i0 += T, ++q) {
        if (q % S != y) continue;  // (block-uniform) the steps are dealt round robin over blockIdx.y
        const int64_t jbase = (int64_t)k0 - (int64_t)i0 - (int64_t)(T - 1);
        if (t < T) {
          const uint64_t i = i0 + t;
          const bool in = i < a;
          ml.put(t, in ? ld_fe(Min, off + i) : fe_zero<F>());
          nl.put(t, in ? ld_fe(Nin, off + i) : fe_zero<F>());
        }
        for (uint32_t w = t; w < W; w += kBlock) {
          const int64_t j = jbase + (int64_t)w;
          const bool in = j >= 0 && (uint64_t)j < b;
          mr.put(w, in ? ld_fe(Min, off + a + (uint64_t)j) : fe_zero<F>());
          nr.put(w, in ? ld_fe(Nin, off + a + (uint64_t)j) : fe_zero<F>());
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t e = 0; e < T; ++e) {
          const Fe l_m = ml.get(e), l_n = nl.get(e), r_m = mr.get(t + T - 1 - e), r_n = nr.get(t + T - 1 - e);
          wide_mac<F>(wm, l_m, r_m);
          wide_mac<F>(wn, l_n, r_m);
          wide_mac<F>(wn, r_n, l_m);
        }
        __syncthreads();
      }
      if (S > 1) {  // partial sums: k_poly_tree_combine adds them and the single terms
        if (k < a + b) {
          st_fe(Mpart, (uint64_t)y * n + g, wide_redc<F>(wm));
          st_fe(Npart, (uint64_t)y * n + g, wide_redc<F>(wn));
        }
      } else if (k < a + b) {  // g < n
        Fe m_out = wide_redc<F>(wm), n_out = wide_redc<F>(wn);
        if (k >= a) {
          m_out = fe_add<F>(m_out, ld_fe(Min, off + a + (k - a)));
          n_out = fe_add<F>(n_out, ld_fe(Nin, off + a + (k - a)));
        }
        if (k >= b && k - b < a) {
          m_out = fe_add<F>(m_out, ld_fe(Min, off + (k - b)));
          n_out = fe_add<F>(n_out, ld_fe(Nin, off + (k - b)));
        }
        st_fe(Mout, g, m_out);
        st_fe(Nout, g, n_out);
      }
    }
  }
}

// A level run with gridDim.y = S > 1 (2 len > kBlock only): output g of a pair
// is the sum of its S partial sums (REDC is linear) and the single terms.
template <class F>
__global__ __launch_bounds__(kBlock) void k_poly_tree_combine(const Fe* Min, const Fe* Nin, const Fe* Mpart, const Fe* Npart,
                                                              uint32_t S, Fe* Mout, Fe* Nout, uint64_t n, uint32_t log_len) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock, len = (uint64_t)1 << log_len;
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
    const uint64_t off = (g >> (log_len + 1)) << (log_len + 1), rem = n - off;
    if (rem <= len) continue;  // copied by k_poly_tree_level
    const uint64_t a = len, b = rem - len < len ? rem - len : len, k = g - off;
    Fe m_out = ld_fe(Mpart, g), n_out = ld_fe(Npart, g);
    for (uint32_t y = 1; y < S; ++y) {
      m_out = fe_add<F>(m_out, ld_fe(Mpart, (uint64_t)y * n + g));
      n_out = fe_add<F>(n_out, ld_fe(Npart, (uint64_t)y * n + g));
    }
    if (k >= a) {
      m_out = fe_add<F>(m_out, ld_fe(Min, off + a + (k - a)));
      n_out = fe_add<F>(n_out, ld_fe(Nin, off + a + (k - a)));
    }
    if (k >= b && k - b < a) {
      m_out = fe_add<F>(m_out, ld_fe(Min, off + (k - b)));
      n_out = fe_add<F>(n_out, ld_fe(Nin, off + (k - b)));
    }
    st_fe(Mout, g, m_out);
    st_fe(Nout, g, n_out);
  }
}

}  // namespace zk
