// Lookups (LogUp, Haboeck 2022) over committed columns, the
// host-only part (no HIP, no zk_ctx, no curve arithmetic): caps and validation,
// the hash and the host build of the open-addressing table, the host
// multiplicity count, the padded table's evaluation, the digest, the plan
// constants of the batched inversion with its host twin, and every transcript
// step. Compiled into the library through lookup.hip and, on the CPU alone,
// into tests/native/lookup_plan_check.cpp.
//
// The statement. f: a column of 2^n elements, 1 <= n <= 24; t: a public table of
// T elements, 1 <= T <= 2^n, duplicates allowed. Claim: every f_i equals some
// t_j. t_pad[j] = t[min(j, T - 1)] for j < 2^n. m_j = #{i : f_i = t_j} at the
// FIRST index j holding that value, 0 at every later duplicate and at the
// padding. With h_f = 1 / (alpha - f) and h_t = m / (alpha - t_pad), the claim
// holds (up to the soundness error of alpha) iff sum h_f = sum h_t.
//
// The transcript, implemented here and nowhere else:
//   1. digest = Keccak-256("zk-lookup-v1" | u32le field, T | each t_j as its 32
//      canonical little-endian bytes), computed at handle creation;
//   2. append(digest); append(u32le n); the 96 bytes of the commitments of f,
//      then of m (committed_plan.hpp g1_bytes);
//   3. alpha = get_random_challenge;
//   4. h_f = 1 / (alpha - f), h_t = m / (alpha - t_pad);
//   5. the 96 bytes of the commitments of h_f, then of h_t;
//   6. tau_0 .. tau_(n-1) by n consecutive get_random_challenge, then lambda;
//   7. the committed sum-check (committed_plan.hpp) with claimed sum 0, degree 3,
//      committed mask 0b1111, over the tables
//        0 h_f   1 h_t   2 f   3 m   4 t_pad   5 ones   6 -ones
//        7 alpha lambda eq(tau,.)   8 -lambda eq(tau,.)
//        9 alpha lambda^2 eq(tau,.)   10 -lambda^2 eq(tau,.)
//      and the terms kLookupFactors: the sum is
//        sum (h_f - h_t) + lambda sum eq (h_f (alpha - f) - 1)
//                        + lambda^2 sum eq (h_t (alpha - t_pad) - m).
//      It absorbs the four commitments again, in table order.
#pragma once
#include "committed_plan.hpp"

namespace zkl {
using zk::Fe;

constexpr uint32_t kLookupMaxVars = 24;           // n <= 24: 2^24 column entries, a count fits 25 bits of a u32 counter
constexpr uint32_t kLookupEmpty = 0xFFFFFFFFu;    // an empty slot
constexpr uint32_t kLookupHashMul = 0x9E3779B1u;  // the multiplicative mix (2^32 / golden ratio, odd)

// The batched inversion (lookup.hpp k_batch_inverse). A wave of 64 lanes owns
// kBatchInvRun * 64 consecutive elements; lane l's run is the elements
// l, l + 64, l + 128 .. of that stretch (so every access of the wave is one
// contiguous 2 KiB), and one Fermat power inverts the product of a whole run:
// one fe_inv per kBatchInvRun elements. A block is kBatchInvBlock lanes.
constexpr uint32_t kBatchInvRun = 64;
constexpr uint32_t kBatchInvBlock = 256;
constexpr uint32_t kBatchInvWave = 64;
constexpr uint64_t kBatchInvWaveTile = (uint64_t)kBatchInvRun * kBatchInvWave;    // 4096 elements per wave
constexpr uint64_t kBatchInvBlockTile = (uint64_t)kBatchInvRun * kBatchInvBlock;  // 16384 elements per block
static_assert(kBatchInvRun >= 64, "at most one fe_inv per 64 elements");

constexpr uint32_t kLookupTables = 11, kLookupTerms = 8, kLookupDegree = 3, kLookupMask = 0xF;
enum { LK_HF = 0, LK_HT = 1, LK_F = 2, LK_M = 3, LK_TPAD = 4, LK_ONE = 5, LK_NEG = 6, LK_E0 = 7 };
constexpr uint8_t kLookupFactors[kLookupTerms * kLookupDegree] = {0, 5, 5, 1, 6, 5, 7, 0, 5, 8, 0, 2,
                                                                  8, 5, 5, 9, 1, 5, 10, 1, 4, 10, 3, 5};
static_assert(kLookupTables <= zkc::kComposedMaxTables && kLookupTerms <= zkc::kComposedMaxTerms &&
                  kLookupDegree <= zkc::kComposedMaxDegree,
              "the lookup's sum-check is inside the composed caps");

// the library's error codes (zk_sumcheck.h), restated so this header stands alone
enum { L_OK = 0, L_EINVAL = 1, L_EUNSUPPORTED = 5 };

// The table's shape: T >= 1 entries of a known field.
inline int lookup_validate_table(uint32_t field, const void* table, uint32_t T, const char** err) {
  *err = nullptr;
  if (!table) return *err = "null argument", L_EINVAL;
  if (field > 2) return *err = "unknown field", L_EINVAL;
  if (T == 0) return *err = "a lookup table needs at least one entry", L_EINVAL;
  if (T > (1u << kLookupMaxVars)) return *err = "more than 2^24 table entries", L_EUNSUPPORTED;
  return L_OK;
}
// A column of 2^n entries against a table of T.
inline int lookup_validate_vars(uint32_t T, uint32_t n, const char** err) {
  *err = nullptr;
  if (n == 0) return *err = "a lookup column needs at least one variable", L_EINVAL;
  if (n > kLookupMaxVars) return *err = "more than 24 variables", L_EUNSUPPORTED;
  if (T > (1u << n)) return *err = "the table is larger than the column", L_EINVAL;
  return L_OK;
}
// `count` entries counted into 2^n slots.
inline int lookup_validate_count(uint32_t T, uint64_t count, uint32_t n, const char** err) {
  const int rc = lookup_validate_vars(T, n, err);
  if (rc != L_OK) return rc;
  if (count == 0) return *err = "count must be at least 1", L_EINVAL;
  if (count > ((uint64_t)1 << kLookupMaxVars)) return *err = "more than 2^24 column entries", L_EUNSUPPORTED;
  return L_OK;
}

// The table's entries: value < p. vals: 4 words per entry, least significant
// first, canonical or (mont) Montgomery; tm: their Montgomery images.
template <class F>
int lookup_entries(const uint64_t* vals, uint32_t T, bool mont, std::vector<Fe>& tm, const char** err) {
  *err = nullptr;
  tm.resize(T);
  for (uint32_t j = 0; j < T; ++j) {
    if (!zk::h64::lt_p<F>(vals + 4 * (size_t)j)) return *err = "field element >= modulus", L_EINVAL;
    Fe x;
    memcpy(x.v, vals + 4 * (size_t)j, 32);
    tm[j] = mont ? x : zk::hfe_to_mont<F>(x);
  }
  return L_OK;
}

// The slot count: the power of two at least 2 T (so at least 2, and at least
// half the slots stay empty: every probe ends).
inline uint32_t lookup_slot_log(uint32_t T) {
  uint32_t lg = 1;
  while (((uint64_t)1 << lg) < 2 * (uint64_t)T) ++lg;
  return lg;
}
// The home slot of a value whose canonical form has the low word lo32: values
// equal mod 2^32 collide.
ZK_HD uint32_t lookup_hash(uint32_t lo32, uint32_t slot_log) { return (lo32 * kLookupHashMul) >> (32 - slot_log); }

// The open-addressing table, linear probing, built in index order: each slot
// holds the first index of its value or kLookupEmpty; a later duplicate of a
// value finds it and adds nothing.
template <class F>
std::vector<uint32_t> lookup_build_slots(const Fe* tm, uint32_t T) {
  const uint32_t lg = lookup_slot_log(T), mask = (1u << lg) - 1;
  std::vector<uint32_t> slots((size_t)1 << lg, kLookupEmpty);
  for (uint32_t j = 0; j < T; ++j) {
    uint32_t s = lookup_hash(zk::hfe_from_mont<F>(tm[j]).v[0], lg);
    for (;; s = (s + 1) & mask) {
      if (slots[s] == kLookupEmpty) {
        slots[s] = j;
        break;
      }
      if (zk::fe_eq<F>(tm[slots[s]], tm[j])) break;
    }
  }
  return slots;
}
// The first index of x (Montgomery) in the table, or kLookupEmpty.
template <class F>
uint32_t lookup_find(const Fe* tm, const uint32_t* slots, uint32_t slot_log, const Fe& x) {
  const uint32_t mask = (1u << slot_log) - 1;
  for (uint32_t s = lookup_hash(zk::hfe_from_mont<F>(x).v[0], slot_log);; s = (s + 1) & mask) {
    const uint32_t j = slots[s];
    if (j == kLookupEmpty || zk::fe_eq<F>(tm[j], x)) return j;
  }
}
// counts[j] for j < T, and the number of entries found nowhere
template <class F>
uint64_t lookup_host_counts(const Fe* tm, uint32_t T, const uint32_t* slots, const Fe* f, uint64_t count,
                            std::vector<uint32_t>& counts) {
  const uint32_t lg = lookup_slot_log(T);
  counts.assign(T, 0);
  uint64_t missing = 0;
  for (uint64_t i = 0; i < count; ++i) {
    const uint32_t j = lookup_find<F>(tm, slots, lg, f[i]);
    if (j == kLookupEmpty) ++missing;
    else ++counts[j];
  }
  return missing;
}

// t_pad~(pt), pt of n coordinates MSB first, in O(T) products after the eq
// weights of the first T indices: c + sum_(j<T) (t_j - c) eq(pt, j), c = t[T-1]
// (the eq weights of all 2^n indices sum to 1).
template <class F>
Fe lookup_table_eval(const Fe* tm, uint32_t T, const Fe* pt, uint32_t n) {
  using namespace zk;
  // eq(pt, j) for j < T, built MSB first and cut to the first T entries at every level
  std::vector<Fe> e(1, fe_one<F>());
  for (uint32_t k = 0; k < n; ++k) {
    const uint64_t need = (((uint64_t)T - 1) >> (n - 1 - k)) + 1;  // indices < T, seen through their top k + 1 bits
    std::vector<Fe> nx(need);
    for (uint64_t j = 0; j < need; ++j) {
      const Fe hi = hfe_mul<F>(e[j >> 1], pt[k]);
      nx[j] = (j & 1) ? hi : hfe_sub<F>(e[j >> 1], hi);
    }
    e.swap(nx);
  }
  const Fe c = tm[T - 1];
  Fe s = c;
  for (uint32_t j = 0; j + 1 < T; ++j) s = hfe_add<F>(s, hfe_mul<F>(hfe_sub<F>(tm[j], c), e[j]));
  return s;
}

// step 1
template <class F>
void lookup_digest(uint32_t field, const Fe* tm, uint32_t T, uint8_t out[32]) {
  zk::Keccak256 h;
  h.update(reinterpret_cast<const uint8_t*>("zk-lookup-v1"), 12);
  auto u32 = [&](uint32_t x) {
    const uint8_t b[4] = {(uint8_t)x, (uint8_t)(x >> 8), (uint8_t)(x >> 16), (uint8_t)(x >> 24)};
    h.update(b, 4);
  };
  u32(field);
  u32(T);
  for (uint32_t j = 0; j < T; ++j) {
    uint8_t b[32];
    zkh::canon_bytes<F>(tm[j], b);
    h.update(b, 32);
  }
  h.finalize_reset(out);
}

// x^-1 by Fermat on the host, 0 -> 0 (field.hpp fe_inv's twin)
template <class F>
Fe hfe_inv(const Fe& x) {
  Fe r = zk::fe_one<F>();
  for (int w = 7; w >= 0; --w)
    for (int b = 31; b >= 0; --b) {
      r = zk::hfe_mul<F>(r, r);
      if ((zk::PMinus2<F>::W[w] >> b) & 1u) r = zk::hfe_mul<F>(r, x);
    }
  return r;
}
// out[i] = in[i]^-1, 0 -> 0, by Montgomery's trick with one power for all; out may be in.
template <class F>
void host_batch_inverse(const Fe* in, size_t count, Fe* out) {
  using namespace zk;
  std::vector<Fe> pre(count);
  Fe acc = fe_one<F>();
  for (size_t i = 0; i < count; ++i) {
    pre[i] = acc;  // the product of the non-zero entries before i
    if (!fe_is_zero<F>(in[i])) acc = hfe_mul<F>(acc, in[i]);
  }
  Fe inv = hfe_inv<F>(acc);
  for (size_t i = count; i-- > 0;) {
    const Fe x = in[i];
    if (fe_is_zero<F>(x)) {
      out[i] = x;
    } else {
      out[i] = hfe_mul<F>(inv, pre[i]);
      inv = hfe_mul<F>(inv, x);
    }
  }
}

// What the prover and the verifier draw before the sum-check (Montgomery).
struct LookupChallenges {
  Fe alpha, lambda;
  std::vector<Fe> tau;
};
// steps 2 and 3. cm_f_m: the 24 words of two zk_g1, f's commitment then m's.
template <class F>
Fe lookup_begin(zk_transcript* tr, const uint8_t digest[32], uint32_t n, const uint64_t* cm_f_m) {
  tr->h.update(digest, 32);
  const uint8_t b[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
  tr->h.update(b, 4);
  zkc::committed_absorb_commitments(tr, cm_f_m, 2);
  return zkh::challenge<F>(tr);
}
// steps 5 and 6. cm_h: the 24 words of two zk_g1, h_f's commitment then h_t's.
template <class F>
void lookup_draw(zk_transcript* tr, uint32_t n, const uint64_t* cm_h, LookupChallenges& ch) {
  zkc::committed_absorb_commitments(tr, cm_h, 2);
  ch.tau.resize(n);
  for (uint32_t k = 0; k < n; ++k) ch.tau[k] = zkh::challenge<F>(tr);
  ch.lambda = zkh::challenge<F>(tr);
}
// The scalars of the four eq tables, tables 7 .. 10.
template <class F>
void lookup_eq_scalars(const Fe& alpha, const Fe& lambda, Fe (&w)[4]) {
  using namespace zk;
  const Fe zero = fe_zero<F>(), l2 = hfe_mul<F>(lambda, lambda);
  w[0] = hfe_mul<F>(alpha, lambda);
  w[1] = hfe_sub<F>(zero, lambda);
  w[2] = hfe_mul<F>(alpha, l2);
  w[3] = hfe_sub<F>(zero, l2);
}
// prod_k (a_k b_k + (1 - a_k)(1 - b_k)), zk_mle_eq_eval's body
template <class F>
Fe lookup_eq_eval(const Fe* a, const Fe* b, uint32_t n) {
  using namespace zk;
  Fe e = fe_one<F>();
  for (uint32_t i = 0; i < n; ++i) {
    const Fe xy = hfe_mul<F>(a[i], b[i]);
    e = hfe_mul<F>(e, hfe_add<F>(hfe_sub<F>(hfe_sub<F>(fe_one<F>(), a[i]), b[i]), hfe_add<F>(xy, xy)));
  }
  return e;
}
// The verifier's own check of the public entries of table_evals at the
// sum-check's point r: ones, -ones, the four scaled eq tables and t_pad.
template <class F>
bool lookup_public_ok(const LookupChallenges& ch, const Fe* r, uint32_t n, const Fe* ev, const Fe& tpad_at_r) {
  using namespace zk;
  const Fe one = fe_one<F>();
  if (!fe_eq<F>(ev[LK_ONE], one) || !fe_eq<F>(ev[LK_NEG], hfe_sub<F>(fe_zero<F>(), one))) return false;
  const Fe e = lookup_eq_eval<F>(ch.tau.data(), r, n);
  Fe w[4];
  lookup_eq_scalars<F>(ch.alpha, ch.lambda, w);
  for (int i = 0; i < 4; ++i)
    if (!fe_eq<F>(ev[LK_E0 + i], hfe_mul<F>(w[i], e))) return false;
  return fe_eq<F>(ev[LK_TPAD], tpad_at_r);
}

// The eleven tables on the host from f, the table and the challenges: small
// instances only (the transcript's reference for the device prover).
template <class F>
std::vector<std::vector<Fe>> lookup_host_tables(const Fe* tm, uint32_t T, const uint32_t* slots, const Fe* f, uint32_t n,
                                                const LookupChallenges& ch) {
  using namespace zk;
  const size_t N = (size_t)1 << n;
  const Fe zero = fe_zero<F>(), one = fe_one<F>();
  std::vector<std::vector<Fe>> tb(kLookupTables, std::vector<Fe>(N, zero));
  std::vector<uint32_t> counts;
  lookup_host_counts<F>(tm, T, slots, f, N, counts);
  for (size_t j = 0; j < N; ++j) {
    tb[LK_F][j] = f[j];
    tb[LK_TPAD][j] = tm[j < T ? j : T - 1];
    if (j < T) tb[LK_M][j] = zkc::fe_small<F>(counts[j]);
    tb[LK_ONE][j] = one;
    tb[LK_NEG][j] = hfe_sub<F>(zero, one);
    tb[LK_HF][j] = hfe_sub<F>(ch.alpha, f[j]);
    tb[LK_HT][j] = hfe_sub<F>(ch.alpha, tb[LK_TPAD][j]);
  }
  host_batch_inverse<F>(tb[LK_HF].data(), N, tb[LK_HF].data());
  host_batch_inverse<F>(tb[LK_HT].data(), N, tb[LK_HT].data());
  for (size_t j = 0; j < N; ++j) tb[LK_HT][j] = hfe_mul<F>(tb[LK_HT][j], tb[LK_M][j]);
  const std::vector<Fe> eq = zkh::host_eq_table<F>(ch.tau.data(), n);
  Fe w[4];
  lookup_eq_scalars<F>(ch.alpha, ch.lambda, w);
  for (int i = 0; i < 4; ++i)
    for (size_t j = 0; j < N; ++j) tb[LK_E0 + i][j] = hfe_mul<F>(w[i], eq[j]);
  return tb;
}
}  // namespace zkl
