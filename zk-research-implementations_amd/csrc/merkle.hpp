// Keccak Merkle tree over field elements (merkle_tree/src/merkle_tree.rs):
// one one-block Keccak-256 per lane.
//
//   compute_hash(x)  = LEint(Keccak256(LE32(x)))          mod p   (:201-206)
//   hash_pair(l, r)  = LEint(Keccak256(LE32(l) | LE32(r))) mod p   (:208-214)
//
// Both messages fit one rate block (136 B), so a hash is exactly one
// Keccak-f[1600] of the state {message words, 0x01, zeros, lane 16 = 1 << 63}
// and the digest is lanes 0-3. Leaves and nodes are stored in CANONICAL form:
// hashing consumes and produces canonical words, so nothing is converted
// between levels (only at the C-ABI boundary, by zk_repr).
//
// The 25 lanes live in registers as 32-bit halves; the 24 rounds are fully
// unrolled, every rotation is a pair of v_alignbit_b32 with an immediate and
// no state array is indexed at run time (no scratch: DESIGN.md, "Merkle").
//
// Tree memory (one allocation of 2^(depth+1) - 1 elements, N = 2^depth):
//   level -1 = the leaves      at [0, N)
//   level l  = tree[l] (:27)   at [2N - (N >> l), ...), N >> (l + 1) nodes
// so the children of node j of level l are elements 2j, 2j + 1 of level l - 1.
#pragma once
#include <utility>

#include "kernels.hpp"

namespace zk {

struct KLane {  // one 64-bit Keccak lane
  uint32_t lo, hi;
};
struct KeccakK {
  static constexpr uint64_t RC[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull,
      0x000000000000808bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
      0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
      0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull,
      0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // rho offsets of lane x + 5y
  static constexpr int ROT[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                                  25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};
};

// a ^ b ^ c: one v_bitop3_b32 (truth table 0x96) per half. Written with the
// builtin: from plain `a ^ b ^ c` the compiler emits two v_xor_b32.
__device__ __forceinline__ KLane kl_xor3(const KLane& a, const KLane& b, const KLane& c) {
  return KLane{(uint32_t)__builtin_amdgcn_bitop3_b32(a.lo, b.lo, c.lo, 0x96),
               (uint32_t)__builtin_amdgcn_bitop3_b32(a.hi, b.hi, c.hi, 0x96)};
}
// rotate left by a compile-time n: v_alignbit_b32(hi:lo >> s) on each half
__device__ __forceinline__ KLane kl_rotl(KLane a, int n) {
  if (n >= 32) {
    const uint32_t t = a.lo;
    a.lo = a.hi;
    a.hi = t;
    n -= 32;
  }
  if (n == 0) return a;
  KLane r;
  r.lo = __builtin_amdgcn_alignbit(a.lo, a.hi, 32 - n);  // (lo << n) | (hi >> (32 - n))
  r.hi = __builtin_amdgcn_alignbit(a.hi, a.lo, 32 - n);
  return r;
}
// chi: a ^ (~b & c), one v_bitop3_b32 per half. The truth table of a
// three-input function f is f(0xF0, 0xCC, 0xAA): 0xF0 ^ (~0xCC & 0xAA) = 0xD2
// (as 0xF0 ^ 0xCC ^ 0xAA = 0x96 above).
__device__ __forceinline__ uint32_t kl_chi32(uint32_t a, uint32_t b, uint32_t c) {
  return (uint32_t)__builtin_amdgcn_bitop3_b32(a, b, c, 0xD2);
}

// one round on the register state; rc is a literal in the unrolled form
__device__ __forceinline__ void keccak_round(KLane (&A)[25], uint64_t rc) {
  KLane C[5], R[5], B[25];
  // theta: column parities (two three-input xors per half), their rotations by
  // 1, and D[x] = C[x-1] ^ rotl(C[x+1], 1) folded into the lane's own xor
#pragma unroll
  for (int x = 0; x < 5; ++x) C[x] = kl_xor3(kl_xor3(A[x], A[x + 5], A[x + 10]), A[x + 15], A[x + 20]);
#pragma unroll
  for (int x = 0; x < 5; ++x) R[x] = kl_rotl(C[x], 1);
  // rho + pi: B[y][2x + 3y] = rotl(A[x][y] ^ D[x], r[x][y])
#pragma unroll
  for (int y = 0; y < 5; ++y)
#pragma unroll
    for (int x = 0; x < 5; ++x)
      B[y + 5 * ((2 * x + 3 * y) % 5)] =
          kl_rotl(kl_xor3(A[x + 5 * y], C[(x + 4) % 5], R[(x + 1) % 5]), KeccakK::ROT[x + 5 * y]);
#pragma unroll
  for (int y = 0; y < 5; ++y)
#pragma unroll
    for (int x = 0; x < 5; ++x) {
      const KLane &a = B[x + 5 * y], &b = B[(x + 1) % 5 + 5 * y], &c = B[(x + 2) % 5 + 5 * y];
      A[x + 5 * y] = KLane{kl_chi32(a.lo, b.lo, c.lo), kl_chi32(a.hi, b.hi, c.hi)};
    }
  A[0].lo ^= (uint32_t)rc;
  A[0].hi ^= (uint32_t)(rc >> 32);
}
// Rounds per trip of the round loop: 24 = no loop at all (the default; a
// `#pragma unroll` alone leaves the compiler free to keep a loop of two trips).
// A smaller divisor of 24 is for A/B builds only.
#ifndef ZK_MERKLE_UNROLL
#define ZK_MERKLE_UNROLL 24
#endif
static_assert(24 % ZK_MERKLE_UNROLL == 0, "ZK_MERKLE_UNROLL divides 24");
template <int... I>
__device__ __forceinline__ void keccak_rounds(KLane (&A)[25], int r0, std::integer_sequence<int, I...>) {
  (keccak_round(A, KeccakK::RC[r0 + I]), ...);
}
__device__ __forceinline__ void keccak_f1600_regs(KLane (&A)[25]) {
  if constexpr (ZK_MERKLE_UNROLL == 24) {
    keccak_rounds(A, 0, std::make_integer_sequence<int, 24>{});
  } else {
#pragma unroll 1
    for (int r0 = 0; r0 < 24; r0 += ZK_MERKLE_UNROLL)
      keccak_rounds(A, r0, std::make_integer_sequence<int, ZK_MERKLE_UNROLL>{});
  }
}

// K p as 8 x u32 (K p < 2^256 for the K used below)
template <class F, int K>
struct PMultiple {
  uint32_t v[8];
  constexpr PMultiple() : v{} {
    uint64_t c = 0;
    for (int i = 0; i < 8; ++i) {
      c += (uint64_t)F::P[i] * K;
      v[i] = (uint32_t)c;
      c >>= 32;
    }
  }
};
template <class F, int K>
__device__ __forceinline__ Fe fe_sub_kp_if_ge(const Fe& x) {
  constexpr PMultiple<F, K> m{};
  Fe t;
  uint32_t b = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) t.v[i] = subb32(x.v[i], m.v[i], b, &b);
  Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = b ? x.v[i] : t.v[i];
  return r;
}
// from_le_bytes_mod_order of a digest: any 256-bit integer, below 6p for the
// BN254 fields (compare-and-subtract 4p, 2p, p) and below 3p for BLS12-381 Fr
// (2p, p). No data-dependent loop.
template <class F>
__device__ __forceinline__ Fe digest_mod_p(Fe d) {
  constexpr bool kWide = (uint64_t)F::P[7] * 4 <= 0xFFFFFFFFull;  // 4p < 2^256
  static_assert(kWide ? (uint64_t)F::P[7] * 6 > 0xFFFFFFFFull : (uint64_t)F::P[7] * 3 > 0xFFFFFFFFull,
                "2^256 must be below 6p (4p, 2p, p) or 3p (2p, p)");
  if constexpr (kWide) d = fe_sub_kp_if_ge<F, 4>(d);
  d = fe_sub_kp_if_ge<F, 2>(d);
  return fe_sub_kp_if_ge<F, 1>(d);
}

// One Keccak-256 of NW canonical elements (NW = 1: compute_hash, 2: hash_pair).
template <class F, int NW>
__device__ __forceinline__ Fe merkle_hash(const Fe (&m)[NW]) {
  static_assert(NW == 1 || NW == 2, "one rate block");
  KLane A[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) A[i] = KLane{0u, 0u};
#pragma unroll
  for (int k = 0; k < NW; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) A[4 * k + i] = KLane{m[k].v[2 * i], m[k].v[2 * i + 1]};
  A[4 * NW].lo = 0x01u;        // Keccak padding 0x01 ...
  A[16].hi = 0x80000000u;      // ... 0x80 in byte 135
  keccak_f1600_regs(A);
  Fe d;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    d.v[2 * i] = A[i].lo;
    d.v[2 * i + 1] = A[i].hi;
  }
  return digest_mod_p<F>(d);
}
template <class F>
__device__ __forceinline__ Fe merkle_hash_pair(const Fe& l, const Fe& r) {
  const Fe m[2] = {l, r};
  return merkle_hash<F, 2>(m);
}
template <class F>
__device__ __forceinline__ Fe merkle_hash_leaf(const Fe& x) {
  const Fe m[1] = {x};
  return merkle_hash<F, 1>(m);
}

// first element of level l (-1: the leaves) of a tree over N leaves
__host__ __device__ inline uint64_t merkle_level_off(uint64_t N, int l) { return 2 * N - ((2 * N) >> (l + 1)); }

// new_with_inputs :60-63: leaves[i] = compute_hash(inputs[i]) for i < n_inputs,
// the field element 0 (not hashed) beyond. FromMont: inputs are Montgomery
// images (a resident device table), else canonical.
template <class F, bool FromMont>
__global__ __launch_bounds__(kBlock) void k_merkle_leaves(const Fe* __restrict__ in, uint64_t n_inputs,
                                                          Fe* __restrict__ leaves, uint64_t N) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
#pragma unroll 1
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += stride) {
    Fe h = fe_zero<F>();
    if (i < n_inputs) {
      Fe x = ld_fe(in, i);
      if (FromMont) x = fe_from_mont<F>(x);
      h = merkle_hash_leaf<F>(x);
    }
    st_fe(leaves, i, h);
  }
}

// One wide level: parent j = hash_pair(child 2j, child 2j + 1) — 64 contiguous
// bytes in, 32 out per thread.
template <class F>
__global__ __launch_bounds__(kBlock) void k_merkle_level(const Fe* __restrict__ child, Fe* __restrict__ parent,
                                                         uint64_t n_parents) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
#pragma unroll 1
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n_parents; j += stride) {
    const Fe l = ld_fe(child, 2 * j), r = ld_fe(child, 2 * j + 1);
    st_fe(parent, j, merkle_hash_pair<F>(l, r));
  }
}

// The narrow levels in one block: from level l0 (at most kBlock nodes, its
// children read from the tree) up to the root, the nodes handed from level to
// level through LDS (two buffers in turn: one barrier per level). Every level
// is also written to the tree. Launched with one block of kBlock threads.
template <class F>
__global__ __launch_bounds__(kBlock) void k_merkle_top(Fe* __restrict__ tree, uint64_t N, int l0, int depth) {
  __shared__ Fe buf[2][kBlock];
  const uint32_t t = threadIdx.x;
  int cur = 0;
#pragma unroll 1
  for (int l = l0; l < depth; ++l) {
    const uint64_t w = N >> (l + 1);  // <= kBlock
    if (t < w) {
      Fe a, b;
      if (l == l0) {
        const Fe* child = tree + merkle_level_off(N, l - 1);
        a = ld_fe(child, 2 * (uint64_t)t);
        b = ld_fe(child, 2 * (uint64_t)t + 1);
      } else {
        a = buf[cur ^ 1][2 * t];
        b = buf[cur ^ 1][2 * t + 1];
      }
      const Fe h = merkle_hash_pair<F>(a, b);
      buf[cur][t] = h;
      st_fe(tree + merkle_level_off(N, l), t, h);
    }
    __syncthreads();
    cur ^= 1;
  }
}

// update_leaf :94-100 for k distinct leaves: leaf = data (is_hash) or
// compute_hash(data). FromMont: data are Montgomery images.
template <class F, bool FromMont>
__global__ __launch_bounds__(kBlock) void k_merkle_set_leaves(Fe* __restrict__ leaves, const uint64_t* __restrict__ ids,
                                                              const Fe* __restrict__ data,
                                                              const uint8_t* __restrict__ is_hash, uint64_t k) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
#pragma unroll 1
  for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < k; q += stride) {
    Fe x = ld_fe(data, q);
    if (FromMont) x = fe_from_mont<F>(x);
    if (!is_hash[q]) x = merkle_hash_leaf<F>(x);
    st_fe(leaves, ids[q], x);
  }
}

// recompute_path :106-132, one level for k touched leaves: the parent of leaf
// ids[q] on level l from both of its children (level l - 1, already final).
// Two leaves under one parent compute and write the same value.
template <class F>
__global__ __launch_bounds__(kBlock) void k_merkle_update_level(Fe* __restrict__ tree, uint64_t N, int l,
                                                                const uint64_t* __restrict__ ids, uint64_t k) {
  const Fe* child = tree + merkle_level_off(N, l - 1);
  Fe* parent = tree + merkle_level_off(N, l);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
#pragma unroll 1
  for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < k; q += stride) {
    const uint64_t p = ids[q] >> (l + 1);
    const Fe a = ld_fe(child, 2 * p), b = ld_fe(child, 2 * p + 1);
    st_fe(parent, p, merkle_hash_pair<F>(a, b));
  }
}

// create_proof :153-177 for k leaves in one launch: out[q (depth + 1)] = leaf
// ids[q], out[q (depth + 1) + 1 + lev] = the sibling of its path on level
// lev - 1 (lev = 0: the leaf level).
__global__ __launch_bounds__(kBlock) void k_merkle_gather(const Fe* __restrict__ tree, uint64_t N, int depth,
                                                          const uint64_t* __restrict__ ids, uint64_t k,
                                                          Fe* __restrict__ out) {
  const uint64_t per = (uint64_t)depth + 1, total = k * per;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
#pragma unroll 1
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
    const uint64_t q = e / per, s = e % per;
    const uint64_t id = ids[q];
    const uint64_t src = s == 0 ? id : merkle_level_off(N, (int)s - 2) + ((id >> (s - 1)) ^ 1);
    st_fe(out, e, ld_fe(tree, src));
  }
}

}  // namespace zk
