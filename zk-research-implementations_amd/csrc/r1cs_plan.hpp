// R1CS satisfiability by two sum-checks over a committed witness (DESIGN.md
// 6k), the host-only part (no HIP, no zk_ctx, no curve arithmetic): shape,
// caps and validation, the instance digest, every transcript step, the host
// evaluations a verifier without a device needs, a host prover for small
// instances and the verifier up to the KZG check. Compiled into the library
// through r1cs.hip and, on the CPU alone, into tests/native/r1cs_plan_check.cpp.
//
// The statement. nrows >= 1 constraints (A z)_i (B z)_i = (C z)_i over
// z of 2^sy entries: the first half (MSB = 0) the witness w, the second half
// (1, io_0 .. io_(npub-1), 0 ..), npub + 1 <= 2^(sy-1). A, B, C are lists of
// (row, col, value) in any order; duplicates of a (row, col) add up; zero
// values are allowed. sx = max(1, ceil log2 nrows); rows are zero-padded.
//
// The transcript, implemented here and nowhere else:
//   1. digest = Keccak-256("zk-r1cs-v1" | u32le field, nrows, sx, sy, npub |
//      for A, B, C: u32le count, then per entry in the caller's order u32le
//      row, u32le col, the value's 32 canonical little-endian bytes);
//   2. append(digest); append(fq_vec_to_bytes(io)); with a KZG setup the 96
//      bytes of the commitment of w (committed_plan.hpp g1_bytes);
//   3. tau_0 .. tau_(sx-1): sx consecutive get_random_challenge;
//   4. sum-check 1 (composed_plan.hpp): tables [eq(tau,.), Az, Bz, -eq(tau,.),
//      Cz, 1], factors {0,1,2},{3,4,5}, degree 3, claimed sum 0 -> rx and
//      va, vb, vc = Az, Bz, Cz at rx;
//   5. append(fq_vec_to_bytes([va, vb, vc])); rho = get_random_challenge;
//   6. M(y) = sum_x eq(rx, x) (A + rho B + rho^2 C)(x, y);
//   7. sum-check 2: tables [M, z], factors {0,1}, degree 2, claimed sum
//      va + rho vb + rho^2 vc -> ry;
//   8. vw = w~(ry[1..]); append(fq_vec_to_bytes([vw])); committed: the opening
//      get_proof(w, vw, ry[1..]).
#pragma once
#include "committed_plan.hpp"
#include "wired_plan.hpp"

namespace zkr {
using zk::Fe;

constexpr uint32_t kR1csMaxVarsLog = zkw::kWiredMaxWidthLog;     // sx, sy <= 24
constexpr uint32_t kR1csMaxEntriesLog = zkw::kWiredMaxGatesLog;  // entries of A, B and C together <= 2^26
// A grouped entry's `other` word: its other index (< 2^24) with the matrix (0 A, 1 B, 2 C) in the top two bits.
constexpr uint32_t kR1csTagShift = 30;
constexpr uint32_t kR1csIndexMask = (1u << kR1csTagShift) - 1;
static_assert(kR1csMaxVarsLog <= kR1csTagShift, "an index and its tag share one word");

constexpr uint8_t kSc1Factors[6] = {0, 1, 2, 3, 4, 5};  // eq a b + neq c one
constexpr uint8_t kSc2Factors[2] = {0, 1};               // M z
constexpr uint32_t kSc1Degree = 3, kSc2Degree = 2;

// the library's error codes (zk_sumcheck.h), restated so this header stands alone
enum { R_OK = 0, R_EINVAL = 1, R_EUNSUPPORTED = 5 };

struct R1csShape {
  uint32_t field = 0, nrows = 0, sx = 0, sy = 0, npub = 0;
  uint32_t nnz[3] = {0, 0, 0};
  size_t off[4] = {0, 0, 0, 0};  // first entry of A, B, C in the concatenated arrays, then their total
  size_t total() const { return off[3]; }
  uint32_t matrix_of(size_t e) const { return e < off[1] ? 0u : e < off[2] ? 1u : 2u; }
};

// Shape checks and caps; fills `s`. `*err` names what failed.
inline int r1cs_shape(uint32_t field, uint32_t nrows, uint32_t sy, uint32_t npub, const uint32_t* nnz, R1csShape& s,
                      const char** err) {
  *err = nullptr;
  if (!nnz) return *err = "null argument", R_EINVAL;
  if (field > 2) return *err = "unknown field", R_EINVAL;
  if (nrows == 0) return *err = "an R1CS instance needs at least one constraint", R_EINVAL;
  if (sy == 0) return *err = "sy must be at least 1", R_EINVAL;
  if (sy > kR1csMaxVarsLog) return *err = "more than 2^24 columns", R_EUNSUPPORTED;
  if (nrows > (1u << kR1csMaxVarsLog)) return *err = "more than 2^24 constraints", R_EUNSUPPORTED;
  const uint64_t total = (uint64_t)nnz[0] + nnz[1] + nnz[2];
  if (total > ((uint64_t)1 << kR1csMaxEntriesLog)) return *err = "more than 2^26 matrix entries in all", R_EUNSUPPORTED;
  if ((uint64_t)npub + 1 > ((uint64_t)1 << (sy - 1))) return *err = "npub + 1 exceeds 2^(sy-1)", R_EINVAL;
  s = R1csShape{};
  s.field = field;
  s.nrows = nrows;
  s.sx = zkw::vars_of(nrows);
  s.sy = sy;
  s.npub = npub;
  for (int t = 0; t < 3; ++t) {
    s.nnz[t] = nnz[t];
    s.off[t + 1] = s.off[t] + nnz[t];
  }
  return R_OK;
}

// The entries: row < nrows, col < 2^sy, value < p. vals: 4 words per entry,
// least significant first, canonical or (mont) Montgomery; vm: their Montgomery images.
template <class F>
int r1cs_entries(const R1csShape& s, const uint32_t* rows, const uint32_t* cols, const uint64_t* vals, bool mont,
                 std::vector<Fe>& vm, const char** err) {
  *err = nullptr;
  const size_t n = s.total();
  if (n && (!rows || !cols || !vals)) return *err = "null argument", R_EINVAL;
  vm.resize(n);
  for (size_t e = 0; e < n; ++e) {
    if (rows[e] >= s.nrows) return *err = "a matrix entry's row is out of range", R_EINVAL;
    if (cols[e] >> s.sy) return *err = "a matrix entry's column is out of range", R_EINVAL;
    if (!zk::h64::lt_p<F>(vals + 4 * e)) return *err = "field element >= modulus", R_EINVAL;
    Fe x;
    memcpy(x.v, vals + 4 * e, 32);
    vm[e] = mont ? x : zk::hfe_to_mont<F>(x);
  }
  return R_OK;
}

// step 1
template <class F>
void r1cs_digest(const R1csShape& s, const uint32_t* rows, const uint32_t* cols, const Fe* vm, uint8_t out[32]) {
  zk::Keccak256 h;
  h.update(reinterpret_cast<const uint8_t*>("zk-r1cs-v1"), 10);
  auto u32 = [&](uint32_t x) {
    const uint8_t b[4] = {(uint8_t)x, (uint8_t)(x >> 8), (uint8_t)(x >> 16), (uint8_t)(x >> 24)};
    h.update(b, 4);
  };
  u32(s.field);
  u32(s.nrows);
  u32(s.sx);
  u32(s.sy);
  u32(s.npub);
  for (int t = 0; t < 3; ++t) {
    u32(s.nnz[t]);
    for (size_t e = s.off[t]; e < s.off[t + 1]; ++e) {
      u32(rows[e]);
      u32(cols[e]);
      uint8_t b[32];
      zkh::canon_bytes<F>(vm[e], b);
      h.update(b, 32);
    }
  }
  h.finalize_reset(out);
}

// step 2. commitment: the 12 words of a zk_g1, or null (no KZG setup).
template <class F>
void r1cs_begin(zk_transcript* tr, const uint8_t digest[32], const Fe* io, uint32_t npub, const uint64_t* commitment) {
  tr->h.update(digest, 32);
  zkh::absorb<F>(tr, io, npub);
  if (commitment) zkc::committed_absorb_commitments(tr, commitment, 1);
}
// step 3
template <class F>
void r1cs_draw_tau(zk_transcript* tr, uint32_t sx, std::vector<Fe>& tau) {
  tau.resize(sx);
  for (uint32_t k = 0; k < sx; ++k) tau[k] = zkh::challenge<F>(tr);
}
// step 5
template <class F>
Fe r1cs_draw_rho(zk_transcript* tr, const Fe& va, const Fe& vb, const Fe& vc) {
  const Fe v[3] = {va, vb, vc};
  zkh::absorb<F>(tr, v, 3);
  return zkh::challenge<F>(tr);
}
// a + rho b + rho^2 c
template <class F>
Fe r1cs_rho_combine(const Fe& rho, const Fe& a, const Fe& b, const Fe& c) {
  using namespace zk;
  return hfe_add<F>(a, hfe_mul<F>(rho, hfe_add<F>(b, hfe_mul<F>(rho, c))));
}

// Entry j of z's second half: (1, io_0 .. io_(npub-1), 0 ..).
template <class F>
Fe r1cs_public_entry(const Fe* io, uint32_t npub, uint32_t j) {
  return j == 0 ? zk::fe_one<F>() : j <= npub ? io[j - 1] : zk::fe_zero<F>();
}
// The multilinear extension of the second half at pt (n = sy - 1 coordinates,
// MSB first), summed over its npub + 1 non-zero entries only.
template <class F>
Fe r1cs_public_eval(const Fe* io, uint32_t npub, const Fe* pt, uint32_t n) {
  using namespace zk;
  Fe s = fe_zero<F>();
  for (uint32_t j = 0; j <= npub; ++j) {
    Fe e = r1cs_public_entry<F>(io, npub, j);
    for (uint32_t k = 0; k < n; ++k)
      e = hfe_mul<F>(e, ((j >> (n - 1 - k)) & 1) ? pt[k] : hfe_sub<F>(fe_one<F>(), pt[k]));
    s = hfe_add<F>(s, e);
  }
  return s;
}
// prod_k (a_k b_k + (1 - a_k)(1 - b_k)), zk_mle_eq_eval's body
template <class F>
Fe r1cs_eq_eval(const Fe* a, const Fe* b, uint32_t n) {
  using namespace zk;
  Fe e = fe_one<F>();
  for (uint32_t i = 0; i < n; ++i) {
    const Fe xy = hfe_mul<F>(a[i], b[i]);
    e = hfe_mul<F>(e, hfe_add<F>(hfe_sub<F>(hfe_sub<F>(fe_one<F>(), a[i]), b[i]), hfe_add<F>(xy, xy)));
  }
  return e;
}

// z -> Az, Bz, Cz over the 2^sx padded rows, O(entries)
template <class F>
void r1cs_host_mul(const R1csShape& s, const uint32_t* rows, const uint32_t* cols, const Fe* vm, const Fe* z,
                   std::vector<Fe> (&out)[3]) {
  for (int t = 0; t < 3; ++t) {
    out[t].assign((size_t)1 << s.sx, zk::fe_zero<F>());
    for (size_t e = s.off[t]; e < s.off[t + 1]; ++e)
      out[t][rows[e]] = zk::hfe_add<F>(out[t][rows[e]], zk::hfe_mul<F>(vm[e], z[cols[e]]));
  }
}
// The three matrices' multilinear extensions at (rx, ry), O(entries) after two eq tables
template <class F>
void r1cs_host_matrix_evals(const R1csShape& s, const uint32_t* rows, const uint32_t* cols, const Fe* vm, const Fe* rx,
                            const Fe* ry, Fe (&out)[3]) {
  const std::vector<Fe> ex = zkh::host_eq_table<F>(rx, s.sx), ey = zkh::host_eq_table<F>(ry, s.sy);
  for (int t = 0; t < 3; ++t) {
    Fe acc = zk::fe_zero<F>();
    for (size_t e = s.off[t]; e < s.off[t + 1]; ++e)
      acc = zk::hfe_add<F>(acc, zk::hfe_mul<F>(vm[e], zk::hfe_mul<F>(ex[rows[e]], ey[cols[e]])));
    out[t] = acc;
  }
}
// step 6 on the host
template <class F>
std::vector<Fe> r1cs_host_m(const R1csShape& s, const uint32_t* rows, const uint32_t* cols, const Fe* vm, const Fe* rx,
                            const Fe& rho) {
  const std::vector<Fe> ex = zkh::host_eq_table<F>(rx, s.sx);
  const Fe w[3] = {zk::fe_one<F>(), rho, zk::hfe_mul<F>(rho, rho)};
  std::vector<Fe> m((size_t)1 << s.sy, zk::fe_zero<F>());
  for (size_t e = 0; e < s.total(); ++e)
    m[cols[e]] = zk::hfe_add<F>(m[cols[e]], zk::hfe_mul<F>(w[s.matrix_of(e)], zk::hfe_mul<F>(vm[e], ex[rows[e]])));
  return m;
}

// The two groupings the gather kernel walks (wired_plan.hpp wired_csr): by
// row with the column as the other index, by column with the row. csr.gate[i]
// is the entry (index into the concatenated arrays) at position i of the
// grouping; `other` is in the same order, and the values are stored alongside
// as val[csr.gate[i]].
struct R1csGroup {
  zkw::WiredCsr csr;
  std::vector<uint32_t> other;
};
inline R1csGroup r1cs_group(const R1csShape& s, const uint32_t* rows, const uint32_t* cols, bool by_row) {
  R1csGroup g;
  const uint32_t n = (uint32_t)s.total();
  g.csr = zkw::wired_csr(by_row ? rows : cols, n, by_row ? s.nrows : 1u << s.sy);
  g.other.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t e = g.csr.gate[i];
    g.other[i] = (by_row ? cols[e] : rows[e]) | (s.matrix_of(e) << kR1csTagShift);
  }
  return g;
}

// What a proof holds besides the KZG points, as the drivers collect it (Montgomery).
template <class F>
struct R1csProof {
  zkc::ComposedOut sc1, sc2;  // sc1.challenges = rx, sc2.challenges = ry
  std::vector<Fe> tau;
  Fe va, vb, vc, rho, vw;
};

// The whole prover on the host, every round by composed_host_rounds: small
// instances only (the transcript's reference for the device prover).
// w: the 2^(sy-1) witness entries; commitment as r1cs_begin takes it.
template <class F>
void r1cs_host_prove(const R1csShape& s, const uint32_t* rows, const uint32_t* cols, const Fe* vm,
                     const uint8_t digest[32], const Fe* w, const Fe* io, const uint64_t* commitment,
                     zk_transcript* tr, R1csProof<F>& p) {
  using namespace zk;
  const size_t X = (size_t)1 << s.sx, Y = (size_t)1 << s.sy, H = Y / 2;
  std::vector<Fe> z(Y);
  for (size_t j = 0; j < H; ++j) {
    z[j] = w[j];
    z[H + j] = r1cs_public_entry<F>(io, s.npub, (uint32_t)j);
  }
  r1cs_begin<F>(tr, digest, io, s.npub, commitment);
  r1cs_draw_tau<F>(tr, s.sx, p.tau);
  std::vector<Fe> abc[3];
  r1cs_host_mul<F>(s, rows, cols, vm, z.data(), abc);
  std::vector<std::vector<Fe>> T(6);
  T[0] = zkh::host_eq_table<F>(p.tau.data(), s.sx);
  T[1] = abc[0];
  T[2] = abc[1];
  T[3].resize(X);
  for (size_t j = 0; j < X; ++j) T[3][j] = hfe_sub<F>(fe_zero<F>(), T[0][j]);
  T[4] = abc[2];
  T[5].assign(X, fe_one<F>());
  zkc::composed_out_init(p.sc1, s.sx, kSc1Degree, fe_zero<F>());
  zkc::composed_host_rounds<F>(T, kSc1Factors, 2, kSc1Degree, 0, s.sx, tr, p.sc1);
  p.va = p.sc1.table_evals[1];
  p.vb = p.sc1.table_evals[2];
  p.vc = p.sc1.table_evals[4];
  p.rho = r1cs_draw_rho<F>(tr, p.va, p.vb, p.vc);
  std::vector<std::vector<Fe>> U(2);
  U[0] = r1cs_host_m<F>(s, rows, cols, vm, p.sc1.challenges.data(), p.rho);
  U[1] = z;
  zkc::composed_out_init(p.sc2, s.sy, kSc2Degree, fe_zero<F>());
  zkc::composed_host_rounds<F>(U, kSc2Factors, 1, kSc2Degree, 0, s.sy, tr, p.sc2);
  p.vw = zkh::mle_eval_host<F>(std::vector<Fe>(w, w + H),
                               std::vector<Fe>(p.sc2.challenges.begin() + 1, p.sc2.challenges.end()));
  zkh::absorb<F>(tr, &p.vw, 1);
}

// The verifier up to the KZG check. cf1: 4 Montgomery coefficients per round
// of sum-check 1, cf2: 3 per round of sum-check 2; matrix_evals(rx, ry, out[3])
// gives the three matrices at (rx, ry) (host or device). On acceptance rx and
// ry are filled, and the claim left open is w~(ry[1..]) = vw.
template <class F, class MatrixEvals>
bool r1cs_verify(const R1csShape& s, const uint8_t digest[32], const Fe* io, const Fe* cf1, const uint8_t* nco1,
                 const Fe* cf2, const uint8_t* nco2, const Fe& va, const Fe& vb, const Fe& vc, const Fe& vw,
                 const uint64_t* commitment, zk_transcript* tr, MatrixEvals&& matrix_evals, std::vector<Fe>& rx,
                 std::vector<Fe>& ry) {
  using namespace zk;
  r1cs_begin<F>(tr, digest, io, s.npub, commitment);
  std::vector<Fe> tau;
  r1cs_draw_tau<F>(tr, s.sx, tau);
  Fe fin1, fin2;
  if (!zkc::composed_verify<F>(kSc1Degree, cf1, nco1, s.sx, fe_zero<F>(), tr, fin1, rx)) return false;
  const Fe e = r1cs_eq_eval<F>(tau.data(), rx.data(), s.sx);
  if (!fe_eq<F>(fin1, hfe_mul<F>(e, hfe_sub<F>(hfe_mul<F>(va, vb), vc)))) return false;
  const Fe rho = r1cs_draw_rho<F>(tr, va, vb, vc);
  if (!zkc::composed_verify<F>(kSc2Degree, cf2, nco2, s.sy, r1cs_rho_combine<F>(rho, va, vb, vc), tr, fin2, ry))
    return false;
  zkh::absorb<F>(tr, &vw, 1);
  Fe m[3];
  matrix_evals(rx.data(), ry.data(), m);
  const Fe pub = r1cs_public_eval<F>(io, s.npub, ry.data() + 1, s.sy - 1);
  const Fe vz = hfe_add<F>(vw, hfe_mul<F>(ry[0], hfe_sub<F>(pub, vw)));  // (1 - ry_0) vw + ry_0 pub
  return fe_eq<F>(fin2, hfe_mul<F>(r1cs_rho_combine<F>(rho, m[0], m[1], m[2]), vz));
}
}  // namespace zkr
