// From a step's sums to sum-check rounds: the transcript, the round
// polynomial, the two- and three-round formulas, the host rounds and the replay
// of device-drawn rounds. Field arithmetic only (no HIP, no zk_ctx): compiled
// into the library through host.hpp and, on the CPU alone, into
// tests/native/gkr_rounds_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hfield.hpp"
#include "keccak.hpp"

using zk::Fe;

// ===========================================================================
// transcript (fiat_shamir_transcript.rs:5-37)
// ===========================================================================
struct zk_transcript {
  zk::Keccak256 h;
};

namespace zkh {
template <class F>
void canon_bytes(const Fe& m, uint8_t out[32]) {  // into_bigint().to_bytes_le()
  const Fe c = zk::hfe_from_mont<F>(m);
  memcpy(out, c.v, 32);
}
// get_random_challenge: d = finalize_reset(); append(d); from_le_bytes_mod_order(d)
template <class F>
Fe challenge(zk_transcript* t) {
  uint8_t d[32];
  t->h.finalize_reset(d);
  t->h.update(d, 32);
  Fe x;
  memcpy(x.v, d, 32);
  return zk::hfe_to_mont<F>(x);  // LE integer mod p (2^256 < 6p), Montgomery image
}
template <class F>
void absorb(zk_transcript* t, const Fe* m, size_t n) {  // append(fq_vec_to_bytes(v))
  uint8_t b[32];
  for (size_t i = 0; i < n; ++i) {
    canon_bytes<F>(m[i], b);
    t->h.update(b, 32);
  }
}

// ---------------------------------------------------------------------------
// GKR sum-check rounds
// ---------------------------------------------------------------------------
struct GkrOut {
  std::vector<Fe> coeffs;     // 3 per round (Montgomery), trimmed count in ncoeffs
  std::vector<uint8_t> ncoeffs;
  std::vector<Fe> challenges;
};

// Absorbs round k's (trimmed) polynomial c, draws r_k and returns s_k(r_k).
template <class F>
Fe absorb_round(zk_transcript* tr, const Fe (&c)[3], int m, uint32_t k, GkrOut& out, Fe& r) {
  using namespace zk;
  absorb<F>(tr, c, (size_t)m);
  out.ncoeffs[k] = (uint8_t)m;
  for (int i = 0; i < 3; ++i) out.coeffs[3 * k + i] = i < m ? c[i] : fe_zero<F>();
  r = challenge<F>(tr);
  out.challenges[k] = r;
  // UnivariatePoly::evaluate(r) (:20-26) via Horner — same field value
  return hfe_add<F>(c[0], hfe_mul<F>(r, hfe_add<F>(c[1], hfe_mul<F>(r, c[2]))));
}
// Round polynomial through (0,e0),(1,e1),(2,e2) — the unique degree<=2
// polynomial UnivariatePoly::interpolate returns (univariate_polynomial_dense.rs:48-74),
// trailing zero coefficients trimmed (:14-18). Absorbs it, draws r_k and
// returns s_k(r_k).
template <class F>
Fe finish_round(zk_transcript* tr, const Fe& e0, const Fe& e1, const Fe& e2, uint32_t k, GkrOut& out, Fe& r) {
  using namespace zk;
  Fe c[3];
  c[0] = e0;
  c[2] = hfe_half<F>(hfe_add<F>(hfe_sub<F>(e0, hfe_add<F>(e1, e1)), e2));
  c[1] = hfe_sub<F>(hfe_sub<F>(e1, e0), c[2]);
  int m = 3;
  while (m > 0 && fe_is_zero<F>(c[m - 1])) --m;
  return absorb_round<F>(tr, c, m, k, out, r);
}

// Host rounds (ZK_HOST_ROUNDS, default 4; only where the caller does not
// need the final tables, host_ok): a double step on a few-element table is
// one wave's dependent chain of 256-bit multiplies (~7 us) plus a hand-off
// (~5 us), while the host does the same round in about a microsecond. So
// the persistent tail's last device step stores its output tables (4 x
// 2^(H+2) elements, 8 KiB at H = 4) to pinned host memory, and the host folds
// them by that step's two challenges and runs the last H rounds itself — the
// reference's own arithmetic (gkr_prove's loop, sum_check_protocol.rs:86-115,
// with get_round_partial_polynomial_proof_gkr :152-166 and partial_evaluate
// multilinear_polynomial_evaluation.rs:52-63), same field values.
template <class F>
void host_fold(std::vector<Fe> (&T)[4], const Fe& r) {
  for (auto& t : T) {
    const size_t h = t.size() / 2;
    for (size_t j = 0; j < h; ++j) t[j] = zk::hfe_add<F>(t[j], zk::hfe_mul<F>(r, zk::hfe_sub<F>(t[j + h], t[j])));
    t.resize(h);
  }
}
// e0 = sum [A S + M P](lo), e2 = sum [A S + M P](2 hi - lo) over the pairs of the current tables
// (products summed unreduced, one reduction per value); E1: also e1 = sum [A S + M P](hi)
template <class F, bool E1 = false>
void host_round_sums(const std::vector<Fe> (&T)[4], Fe& e0, Fe& e2, Fe* e1 = nullptr) {
  using namespace zk;
  const size_t h = T[0].size() / 2;
  uint64_t a0[9] = {0}, a1[9] = {0}, a2[9] = {0};
  for (size_t j = 0; j < h; ++j) {
    h64::V x2[4];
    for (int t = 0; t < 4; ++t) x2[t] = h64::of(hfe_sub<F>(hfe_add<F>(T[t][j + h], T[t][j + h]), T[t][j]));
    h64::mac_wide(a0, h64::of(T[0][j]), h64::of(T[1][j]));
    h64::mac_wide(a0, h64::of(T[2][j]), h64::of(T[3][j]));
    if constexpr (E1) {
      h64::mac_wide(a1, h64::of(T[0][j + h]), h64::of(T[1][j + h]));
      h64::mac_wide(a1, h64::of(T[2][j + h]), h64::of(T[3][j + h]));
    }
    h64::mac_wide(a2, x2[0], x2[1]);
    h64::mac_wide(a2, x2[2], x2[3]);
  }
  e0 = wide_to_fe<F>(a0);
  if constexpr (E1) *e1 = wide_to_fe<F>(a1);
  e2 = wide_to_fe<F>(a2);
}

// One phase of a circuit layer's sum-check entirely on the host (host_layer in
// gkr_layers.hpp, for the tree prover and the wired prover alike): n
// rounds over the four tables T, starting at global round k0.
template <class F>
void host_layer_phase(std::vector<Fe> (&T)[4], uint32_t n, uint32_t k0, zk_transcript* tr, GkrOut& out) {
  Fe r;
  for (uint32_t i = 0; i < n; ++i) {
    Fe e0, e1, e2;
    host_round_sums<F, true>(T, e0, e2, &e1);
    finish_round<F>(tr, e0, e1, e2, k0 + i, out, r);
    host_fold<F>(T, r);  // (after the last round: the tables at the phase's point, one entry each)
  }
}
// eq(pt, v) for every v < 2^n, bit n-1-k of v against pt[k] (MSB first):
// one product per entry (the table doubles once per coordinate)
template <class F>
std::vector<Fe> host_eq_table(const Fe* pt, uint32_t n) {
  std::vector<Fe> t(1, zk::fe_one<F>());
  for (uint32_t k = 0; k < n; ++k) {
    std::vector<Fe> u(2 * t.size());
    for (size_t j = 0; j < t.size(); ++j) {
      const Fe x = zk::hfe_mul<F>(t[j], pt[k]);
      u[2 * j] = zk::hfe_sub<F>(t[j], x);
      u[2 * j + 1] = x;
    }
    t.swap(u);
  }
  return t;
}
template <class F>
Fe mle_eval_host(std::vector<Fe> t, const std::vector<Fe>& pt) {  // MultilinearPoly::evaluate (:79-91)
  for (const Fe& r : pt) {
    const size_t h = t.size() / 2;
    for (size_t j = 0; j < h; ++j) t[j] = zk::hfe_add<F>(t[j], zk::hfe_mul<F>(r, zk::hfe_sub<F>(t[j + h], t[j])));
    t.resize(h);
  }
  return t[0];
}

// The four tables folded by every challenge of a phase (the multilinear
// extensions at the phase's point), when its last rounds ran on the host.
struct FinalVals {
  Fe v[4];
  bool ok = false;
};

// The running state of a phase's rounds. e1 of every round after the first is
// derived as s_{k-1}(r_{k-1}) - e0, exact because A*S + M*P has degree 2 per
// variable.
struct RoundState {
  zk_transcript* tr;
  GkrOut& out;
  Fe& claim;    // s_{k-1}(r_{k-1})
  Fe& r;        // the newest challenge
  uint32_t k0;  // global index of the phase's round 0
  Fe rz, ra, rb;  // the last three challenges (oldest first)
  void drew() {
    rz = ra;
    ra = rb;
    rb = r;
  }
};
template <class F>
void one_round(RoundState& s, uint32_t i, const Fe& e0, const Fe& e1, const Fe& e2) {
  s.claim = finish_round<F>(s.tr, e0, e1, e2, s.k0 + i, s.out, s.r);
  s.drew();
}
template <class F>
void later_round(RoundState& s, uint32_t i, const Fe& e0, const Fe& e2) {  // any round but a phase's first
  one_round<F>(s, i, e0, zk::hfe_sub<F>(s.claim, e0), e2);
}

// rounds i0, i0 + 1, i0 + 2 from the 27 moment sums of k_gkr_d0t / k_gkr_t33 (tile id
// 9 alpha + 3 beta + gamma per axis: 0 = X0 Y0, 1 = X1 Y1, 2 = X0 Y1 + X1 Y0);
// X(t) Y(t) = (1-t)^2 m0 + t^2 m1 + t(1-t) ms, so at t = 2 the weights are (1, 4, -2)
template <class F>
void three_rounds(RoundState& s, uint32_t i0, bool first, const Fe (&T)[27]) {
  using namespace zk;
  const Fe one = fe_one<F>();
  auto at2w = [&](const Fe& m0, const Fe& m1, const Fe& ms) {  // value at t = 2: m0 + 4 m1 - 2 ms
    const Fe m1x2 = hfe_add<F>(m1, m1);
    return hfe_sub<F>(hfe_add<F>(m0, hfe_add<F>(m1x2, m1x2)), hfe_add<F>(ms, ms));
  };
  auto wts = [&](const Fe& t, Fe (&w)[3]) {  // (1-t)^2 = (1-t) - t(1-t), t(1-t) = t - t^2
    w[1] = hfe_mul<F>(t, t);
    w[2] = hfe_sub<F>(t, w[1]);
    w[0] = hfe_sub<F>(hfe_sub<F>(one, t), w[2]);
  };
  Fe U[3];  // round i0: U[alpha] = sum over beta, gamma in {0, 1}
  for (int a = 0; a < 3; ++a)
    U[a] = hfe_add<F>(hfe_add<F>(T[9 * a], T[9 * a + 1]), hfe_add<F>(T[9 * a + 3], T[9 * a + 4]));
  one_round<F>(s, i0, U[0], first ? U[1] : hfe_sub<F>(s.claim, U[0]), at2w(U[0], U[1], U[2]));
  Fe wa[3];
  wts(s.r, wa);
  Fe V[3];  // round i0 + 1: V[beta] = sum_alpha w(ra, alpha) sum_{gamma in {0, 1}}
  for (int b = 0; b < 3; ++b) {
    V[b] = fe_zero<F>();
    for (int a = 0; a < 3; ++a)
      V[b] = hfe_add<F>(V[b], hfe_mul<F>(wa[a], hfe_add<F>(T[9 * a + 3 * b], T[9 * a + 3 * b + 1])));
  }
  later_round<F>(s, i0 + 1, V[0], at2w(V[0], V[1], V[2]));
  Fe wb[3];
  wts(s.r, wb);
  Fe Z[3];  // round i0 + 2: Z[gamma] = sum_alpha w(ra, alpha) sum_beta w(rb, beta) T
  for (int g = 0; g < 3; ++g) {
    uint64_t acc[9] = {0};
    for (int a = 0; a < 3; ++a) {
      uint64_t in[9] = {0};
      for (int b = 0; b < 3; ++b) h64::mac_wide(in, h64::of(wb[b]), h64::of(T[9 * a + 3 * b + g]));
      h64::mac_wide(acc, h64::of(wa[a]), h64::of(wide_to_fe<F>(in)));
    }
    Z[g] = wide_to_fe<F>(acc);
  }
  later_round<F>(s, i0 + 2, Z[0], at2w(Z[0], Z[1], Z[2]));
}

// rounds i0 and i0 + 1 from a double step's eight product sums (the first
// step of a phase, k_gkr_d0: nine, the ninth V11 for round 0's e1)
template <class F>
void two_rounds(RoundState& s, uint32_t i0, bool first, const Fe* d) {
  using namespace zk;
  // categories: 0 V00, 1 V22, 2 V01, 3 V02, 4 V10, 5 V20, 6 V21, 7 V12, 8 V11 (kernels.hpp)
  // round i: e0 = V00 + V01, e1 = V10 + V11 (first) or s_{i-1}(r_{i-1}) - e0, e2 = V20 + V21
  const Fe e0 = hfe_add<F>(d[0], d[2]);
  const Fe e1 = first ? hfe_add<F>(d[4], d[8]) : hfe_sub<F>(s.claim, e0);
  one_round<F>(s, i0, e0, e1, hfe_add<F>(d[5], d[6]));
  // round i + 1 at r = r_i: e0' through (V00, V10, V20), e2' through (V02, V12, V22) at r = 0, 1, 2
  const Fe &r = s.r, one = fe_one<F>(), two = hfe_add<F>(one, one);
  const Fe rm1 = hfe_sub<F>(r, one), rm2 = hfe_sub<F>(r, two);
  const Fe L0 = hfe_half<F>(hfe_mul<F>(rm1, rm2));             // (r-1)(r-2)/2
  const Fe L1 = hfe_sub<F>(fe_zero<F>(), hfe_mul<F>(r, rm2));  // -r(r-2)
  const Fe L2 = hfe_half<F>(hfe_mul<F>(r, rm1));               // r(r-1)/2
  auto lag = [&](const Fe& v0, const Fe& v1, const Fe& v2) {
    return hfe_add<F>(hfe_add<F>(hfe_mul<F>(L0, v0), hfe_mul<F>(L1, v1)), hfe_mul<F>(L2, v2));
  };
  const Fe f0 = lag(d[0], d[4], d[5]), f2 = lag(d[3], d[7], d[1]);
  later_round<F>(s, i0 + 1, f0, f2);
}

// eq((rz, ra, rb), c), c = 4a + 2b + c0 (rz, the oldest, on the top bit): the
// eight weights of a fold by three, formed on the host instead of in every
// block of the step (five products: ab = eq((rz, ra), (a, b)) from rz ra by
// differences, then e(ab, c = 1) = ab rb and e(ab, c = 0) = ab - ab rb)
template <class F>
void eq8_weights(const Fe& rz, const Fe& ra, const Fe& rb, Fe (&e)[8]) {
  using namespace zk;
  Fe ab[4];
  ab[3] = hfe_mul<F>(rz, ra);
  ab[2] = hfe_sub<F>(rz, ab[3]);                             // rz (1 - ra)
  ab[1] = hfe_sub<F>(ra, ab[3]);                             // (1 - rz) ra
  ab[0] = hfe_sub<F>(hfe_sub<F>(fe_one<F>(), rz), ab[1]);    // (1 - rz)(1 - ra)
  for (int q = 0; q < 4; ++q) {
    e[2 * q + 1] = hfe_mul<F>(ab[q], rb);
    e[2 * q] = hfe_sub<F>(ab[q], e[2 * q + 1]);
  }
}

// The tables a persistent tail handed over (4 tables of len elements,
// word-major per table, kernels.hpp st_fe_sys; level i - 2): fold by r_{i-2},
// r_{i-1}, then rounds i .. nv-1 on the host. fin: also the tables at the
// phase's point (one more fold by the last challenge).
template <class F>
void host_rounds(RoundState& s, uint32_t i, uint32_t nv, const uint64_t* raw, FinalVals* fin) {
  const size_t len = (size_t)1 << (nv - i + 2);
  std::vector<Fe> T[4];
  for (int t = 0; t < 4; ++t) {
    const uint64_t* w = raw + (size_t)t * 4 * len;
    T[t].resize(len);
    for (size_t e = 0; e < len; ++e)
      for (int k = 0; k < 4; ++k) {
        const uint64_t x = w[k * len + e];
        T[t][e].v[2 * k] = (uint32_t)x;
        T[t][e].v[2 * k + 1] = (uint32_t)(x >> 32);
      }
  }
  host_fold<F>(T, s.ra);
  host_fold<F>(T, s.rb);
  for (; i < nv; ++i) {
    Fe e0, e2;
    host_round_sums<F>(T, e0, e2);
    later_round<F>(s, i, e0, e2);
    if (i + 1 < nv || fin) host_fold<F>(T, s.r);
  }
  if (fin) {
    for (int t = 0; t < 4; ++t) fin->v[t] = T[t][0];
    fin->ok = true;
  }
}

// One round the device drew itself (ZK_DEVICE_FS; dfs.hpp FsLog: coefficients
// cf, their trimmed count m, the challenge rd, all Montgomery images),
// replayed into the host transcript: absorb the coefficients, draw the
// challenge, check it against the device's. Returns what is wrong, or null.
template <class F>
const char* replay_device_fs(RoundState& s, uint32_t i, const uint32_t (*cf)[8], uint32_t m, const uint32_t* rd) {
  using namespace zk;
  if (m > 3) return "device Fiat-Shamir record corrupt";
  Fe c[3];
  for (uint32_t q = 0; q < 3; ++q) {
    if (q < m) memcpy(c[q].v, cf[q], 32);
    else c[q] = fe_zero<F>();
  }
  // the device's interpolation, checked: s(0) + s(1) = 2 c0 + c1 + c2 must be
  // the running claim (a replayed hash alone proves only the replay)
  const Fe s01 = hfe_add<F>(hfe_add<F>(hfe_add<F>(c[0], c[0]), c[1]), c[2]);
  if (memcmp(s01.v, s.claim.v, 32) != 0) return "device Fiat-Shamir round polynomial does not match the running claim";
  s.claim = absorb_round<F>(s.tr, c, (int)m, s.k0 + i, s.out, s.r);
  if (memcmp(s.r.v, rd, 32) != 0) return "device Fiat-Shamir challenge differs from the host transcript";
  s.drew();
  return nullptr;
}
}  // namespace zkh
