// Sum-check over KZG-committed tables, the host-only part (no
// HIP, no zk_ctx, no curve arithmetic): the checks on the committed mask, the
// powers of rho that batch k openings into one, the byte form of a commitment
// and the two transcript steps that surround the composed sum-check. Compiled
// into the library through host.hpp and, on the CPU alone, into
// tests/native/committed_plan_check.cpp.
//
// The transcript of a committed sum-check, implemented here and nowhere else:
//   1. committed_absorb_commitments: for each committed table in index order,
//      append 96 bytes, x then y, each canonical little-endian 48 bytes (as
//      zk_g1 holds them); the point at infinity is 96 zero bytes;
//   2. the composed sum-check (composed_plan.hpp) on the same transcript;
//   3. committed_draw_rho: append(fq_vec_to_bytes(table_evals[0..ntables))),
//      then rho = get_random_challenge;
//   4. the j-th committed table (index order) is weighted by rho^j
//      (rho_powers); the opened value of the batch is rho_combine of the
//      committed tables' evaluations.
#pragma once
#include "composed_plan.hpp"

namespace zkc {
// The products of a linear combination are summed unreduced in one 544-bit
// accumulator (field.hpp Wide, 17 words) and reduced once: k products of
// values < p need k p^2 < 2^544. The largest modulus is BLS12-381 Fr,
// p < 2^255, so 16 p^2 < 2^514 and the cap is 16 with room to spare; it is
// also the composed sum-check's table cap, so a batch never needs splitting.
constexpr uint32_t kLincombMaxTables = 16;
static_assert(kLincombMaxTables == kComposedMaxTables, "a batch opens every table of a composed sum-check");

inline uint32_t mask_count(uint32_t mask) {
  uint32_t n = 0;
  for (; mask; mask &= mask - 1) ++n;
  return n;
}

// Bit i of `mask`: table i is committed. At least one table is, no bit names a
// table >= ntables, and the tables have as many variables as the setup (so
// nvars = 0 is refused: KZG needs one variable). ntables itself is the composed
// sum-check's to check.
inline int committed_validate(uint32_t ntables, uint32_t nvars, uint32_t setup_nvars, uint32_t mask, const char** err) {
  *err = nullptr;
  auto bad = [&](const char* m) {
    *err = m;
    return (int)C_EINVAL;
  };
  if (mask == 0) return bad("committed_mask is empty");
  if (ntables < 32 && (mask >> ntables) != 0) return bad("committed_mask names a table >= ntables");
  if (nvars != setup_nvars) return bad("nvars differs from the KZG setup's variable count");
  return C_OK;
}

// out[j] = rho^j for j < k (out[0] = 1 whatever rho is)
template <class F>
void rho_powers(const Fe& rho, uint32_t k, Fe* out) {
  for (uint32_t j = 0; j < k; ++j) out[j] = j ? zk::hfe_mul<F>(out[j - 1], rho) : zk::fe_one<F>();
}
// sum_j pows[j] vals[j]
template <class F>
Fe rho_combine(const Fe* pows, const Fe* vals, uint32_t k) {
  Fe s = zk::fe_zero<F>();
  for (uint32_t j = 0; j < k; ++j) s = zk::hfe_add<F>(s, zk::hfe_mul<F>(pows[j], vals[j]));
  return s;
}

// A G1 point as the transcript takes it. xy: the 12 words of a zk_g1 (x[6] then
// y[6], canonical, least significant word first).
inline void g1_bytes(const uint64_t* xy, uint8_t out[96]) {
  for (int i = 0; i < 12; ++i)
    for (int b = 0; b < 8; ++b) out[8 * i + b] = (uint8_t)(xy[i] >> (8 * b));
}
// step 1: points = 12 words per commitment, committed tables in index order
inline void committed_absorb_commitments(zk_transcript* tr, const uint64_t* points, uint32_t n) {
  uint8_t b[96];
  for (uint32_t i = 0; i < n; ++i) {
    g1_bytes(points + 12 * (size_t)i, b);
    tr->h.update(b, 96);
  }
}
// step 3: every table's evaluation (Montgomery), committed or not, then rho
template <class F>
Fe committed_draw_rho(zk_transcript* tr, const Fe* table_evals, uint32_t ntables) {
  zkh::absorb<F>(tr, table_evals, ntables);
  return zkh::challenge<F>(tr);
}

// The committed tables' entries of `all` in index order; returns their count.
template <class T>
uint32_t committed_select(uint32_t mask, uint32_t ntables, const T* all, T* out) {
  uint32_t n = 0;
  for (uint32_t i = 0; i < ntables; ++i)
    if ((mask >> i) & 1u) out[n++] = all[i];
  return n;
}
}  // namespace zkc
