// GKR over a layered circuit (gkr_protocol.rs:31-227): the parts the tree
// prover (gkr_circuit.hip) and the wired prover (wired.hip) share. A tree is a
// wired circuit with left = 2g, right = 2g + 1, so one shape (wired_plan.hpp
// WiredShape: per layer G gates, ka = the gate index's variables, kb = the
// variables of the layer's inputs) describes both, and here live, once each:
// the output stage, a layer's sum-check on the host, the skeleton of a layer's
// sum-check on the device, the prover's layer loop and the verifier's. What a
// caller supplies is its wiring (two callables) and how it fills a device
// layer's tables.
#pragma once
#include "host.hpp"

namespace zkh {
// What both provers return: the padded outputs, all layers' rounds (output
// layer first), every inner layer's two evaluations, the input layer's two.
struct LayersOut {
  std::vector<Fe> out_poly;
  GkrOut sc;
  std::vector<Fe> claims;
  Fe in_eval[2];
};

template <class F>
void gkr_out_init(GkrOut& out, uint32_t nrounds) {
  out.coeffs.assign(3 * (size_t)nrounds, zk::fe_zero<F>());
  out.ncoeffs.assign(nrounds, 0);
  out.challenges.assign(nrounds, zk::fe_zero<F>());
}

inline bool circuit_debug() {  // ZK_DEBUG_CIRCUIT: one timing line per layer on stderr (tools/circuit_phases.py)
  static const bool dbg = getenv("ZK_DEBUG_CIRCUIT") != nullptr;
  return dbg;
}
using LayerClock = std::chrono::steady_clock;
// Where a layer's time went, for the debug line: its tables ready at t1, its
// rounds done at t2. The loop stamps t1 before the layer and t2 after it; a
// layer that knows better stamps them itself.
struct LayerStamps {
  LayerClock::time_point t1, t2;
};

// The output stage: absorb the 2^v padded outputs, draw r0[0..v), absorb m0 = MLE(out)(r0)
// (v = 1: initiate_protocol, gkr_protocol.rs:229-241). Returns m0.
template <class F>
Fe gkr_output_stage(zk_transcript* tr, const std::vector<Fe>& outp, uint32_t v, std::vector<Fe>& r0) {
  absorb<F>(tr, outp.data(), outp.size());
  r0.clear();
  for (uint32_t k = 0; k < v; ++k) r0.push_back(challenge<F>(tr));
  const Fe m0 = mle_eval_host<F>(outp, r0);
  absorb<F>(tr, &m0, 1);
  return m0;
}

// A layer's gate weights on the host (k_gate_weights / k_wired_weights): the output layer
// folds its index with r0 (get_fbc_poly, :243-263), later layers
// alpha eq(r_b, g) + beta eq(r_c, g) (get_folded_fbc_poly, :265-292)
template <class F>
std::vector<Fe> host_gate_weights(const std::vector<Fe>& rb, const std::vector<Fe>& rc, const Fe& alpha, const Fe& beta,
                                  bool has_c, uint32_t ka, uint32_t G) {
  const std::vector<Fe> eb = host_eq_table<F>(rb.data(), ka);
  const std::vector<Fe> ec = has_c ? host_eq_table<F>(rc.data(), ka) : std::vector<Fe>();
  std::vector<Fe> wt(G);
  for (uint32_t g = 0; g < G; ++g) {
    wt[g] = zk::hfe_mul<F>(alpha, eb[g]);
    if (has_c) wt[g] = zk::hfe_add<F>(wt[g], zk::hfe_mul<F>(beta, ec[g]));
  }
  return wt;
}

// A small layer's sum-check entirely on the host (ZK_CIRCUIT_HOST_LGL): the
// same two phases over the same four tables of L = 2^kb entries as
// device_layer, the same field values and transcript, with no device round
// trip — on tables of a few hundred entries one host pass per round takes
// microseconds, while each device step waits for a host hand-off. The
// reference's own arithmetic: gkr_prove (sum_check_protocol.rs:86-115) with
// get_round_partial_polynomial_proof_gkr (:152-166) and partial_evaluate
// (multilinear_polynomial_evaluation.rs:52-63); each round's three values are
// summed unreduced and reduced once (host_layer_phase and host_eq_table,
// gkr_rounds.hpp).
// w = the layer's L inputs, wt = its G gate weights, ops its gate ops; gate g
// reads wires left(g) and right(g). One loop over the gates fills the tables.
// ev = {w(r_b), w(r_c)} from the folds, as in device_layer.
template <class F, class Left, class Right>
void host_layer(const Fe* w, const std::vector<Fe>& wt, const uint8_t* ops, uint32_t G, uint32_t kb, Left left,
                Right right, zk_transcript* tr, GkrOut& out, Fe (&ev)[2]) {
  using namespace zk;
  const size_t L = (size_t)1 << kb;
  gkr_out_init<F>(out, 2 * kb);
  std::vector<Fe> T[4];  // phase 1 (k_phase1_tables): W = w, U, V, 1
  for (auto& t : T) t.assign(L, fe_zero<F>());
  for (size_t b = 0; b < L; ++b) {
    T[0][b] = w[b];
    T[3][b] = fe_one<F>();
  }
  for (uint32_t g = 0; g < G; ++g) {
    const Fe x = wt[g], xw = hfe_mul<F>(x, w[right(g)]);
    Fe& u = T[1][left(g)];
    if (ops[g]) {
      u = hfe_add<F>(u, xw);
    } else {
      u = hfe_add<F>(u, x);
      T[2][left(g)] = hfe_add<F>(T[2][left(g)], xw);
    }
  }
  host_layer_phase<F>(T, kb, 0, tr, out);
  const Fe wrb = T[0][0];  // W = w folded by r_b
  for (auto& t : T) t.assign(L, fe_zero<F>());  // phase 2 (k_phase2_tables): A, S, M, P over c
  const std::vector<Fe> eqb = host_eq_table<F>(out.challenges.data(), kb);
  for (uint32_t g = 0; g < G; ++g) {
    Fe& t = (ops[g] ? T[2] : T[0])[right(g)];
    t = hfe_add<F>(t, hfe_mul<F>(wt[g], eqb[left(g)]));
  }
  for (size_t cc = 0; cc < L; ++cc) {
    T[1][cc] = hfe_add<F>(wrb, w[cc]);
    T[3][cc] = hfe_mul<F>(wrb, w[cc]);
  }
  host_layer_phase<F>(T, kb, kb, tr, out);
  ev[0] = wrb;
  ev[1] = hfe_sub<F>(T[1][0], wrb);  // S = w(r_b) + w(c) folded by r_c
}

// One layer's sum-check (2 kb rounds) on the device, in two phases over tables
// of L = 2^kb entries: the same round polynomials and challenges as gkr_prove
// over the dense L^2 tables, since every round value is the same field sum.
// Phase 1 binds b (rounds 0 .. kb-1), phase 2 binds c; both phases run the
// device sum-check of the hot path (gkr_phase) on the shared transcript, their
// last rounds on the host. The layer's two evaluations come out of the folds:
// phase 1's W = w folded by r_b is w(r_b), and phase 2's S(c) = w(r_b) + w(c)
// folded by r_c is w(r_b) + w(r_c) (a multilinear extension plus a constant),
// so ev = {w(r_b), w(r_c)} (gkr_protocol.rs:75-76) without another pass over w
// — when a phase ends on the host (FinalVals); otherwise the layer evaluates w.
// `ly` fills the tables and evaluates (ch = the challenges drawn so far):
//   ly.fill1(t)              phase 1's four tables W, U, V, 1 at t, t + L, t + 2L, t + 3L
//   ly.eval_b(ch)            w(r_b), r_b = ch[0..kb)
//   ly.fill2(ch, wrb, t)     phase 2's four tables A, S, M, P, wrb = w(r_b)
//   ly.eval_c(ch)            w(r_c), r_c = ch[kb..2 kb)
template <class F, class Layer>
void device_layer(zk_ctx* c, uint32_t kb, Layer& ly, zk_transcript* tr, GkrOut& out, Fe (&ev)[2]) {
  const uint64_t L = (uint64_t)1 << kb;
  gkr_out_init<F>(out, 2 * kb);
  ensure_partials(c, kb);
  __atomic_store_n(h_err(c), 0u, __ATOMIC_RELAXED);
  c->work[0].ensure(4 * std::max<uint64_t>(L / 2, 1) * 32);
  c->work[1].ensure(4 * std::max<uint64_t>(L / 4, 1) * 32);
  c->input.ensure(8 * L * 32);
  Fe* t1 = c->input.fe();
  Fe* t2 = t1 + 4 * L;
  ly.fill1(t1);
  const Fe* cur[4] = {t1, t1 + L, t1 + 2 * L, t1 + 3 * L};
  Fe claim = zk::fe_zero<F>(), r = zk::fe_zero<F>();
  uint32_t pend = 0;
  FinalVals f1, f2;
  gkr_phase<F>(c, cur, kb, 0, false, tr, out, claim, r, pend, true, 0, nullptr, &f1);  // rounds 0 .. kb-1 (b)
  const Fe* ch = out.challenges.data();
  ev[0] = f1.ok ? f1.v[0] : ly.eval_b(ch);
  ly.fill2(ch, ev[0], t2);
  const Fe* cur2[4] = {t2, t2 + L, t2 + 2 * L, t2 + 3 * L};
  gkr_phase<F>(c, cur2, kb, kb, false, tr, out, claim, r, pend, true, 0, nullptr, &f2);  // rounds kb .. 2 kb-1 (c)
  ev[1] = f2.ok ? zk::hfe_sub<F>(f2.v[1], ev[0]) : ly.eval_c(ch);  // S = w(r_b) + w(c) folded by r_c
  sync(c);
}

// The prover's layer loop (gkr_protocol.rs:60-91), after the output stage has
// put r0 in rb: layers from the output down, each on the host when its tables
// have at most 2^ZK_CIRCUIT_HOST_LGL entries and on the device otherwise, its
// rounds appended to o.sc, its challenges split into the next layer's
// (r_b, r_c), alpha and beta drawn from its two evaluations.
//   cir.host_layer(l, wt, tr, g, ev)     layer l by zkh::host_layer over the circuit's wiring
//   cir.device_layer(l, rb, rc, alpha, beta, has_c, tr, g, ev, st)
//                                        its gate weights and its sum-check on the device
template <class F, class Circuit>
void gkr_layers_prove(zk_ctx* c, const zkw::WiredShape& sh, Circuit& cir, zk_transcript* tr, std::vector<Fe> rb,
                      LayersOut& o) {
  using namespace zk;
  const bool dbg = circuit_debug();
  auto us = [](LayerClock::time_point a, LayerClock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
  };
  std::vector<Fe> rc;
  Fe alpha = fe_one<F>(), beta = fe_zero<F>();
  gkr_out_init<F>(o.sc, sh.total_rounds);
  uint32_t k0 = 0;
  for (uint32_t idx = 0; idx < sh.nlayers; ++idx) {
    const uint32_t l = sh.nlayers - 1 - idx, G = sh.gates[l], ka = sh.ka[l], kb = sh.kb[l], nv = 2 * kb;
    const bool has_c = idx > 0;
    require(rb.size() == ka && (!has_c || rc.size() == ka), "internal: challenge split does not match the layer");
    GkrOut g;
    Fe ev[2];
    LayerStamps st;
    const LayerClock::time_point t0 = LayerClock::now();
    st.t1 = t0;
    if (kb <= c->circuit_host_lgl) {  // gate weights, both phases and both evaluations on the host
      cir.host_layer(l, host_gate_weights<F>(rb, rc, alpha, beta, has_c, ka, G), tr, g, ev);
    } else {
      cir.device_layer(l, rb, rc, alpha, beta, has_c, tr, g, ev, st);
    }
    if (st.t2 < st.t1) st.t2 = LayerClock::now();
    for (uint32_t k = 0; k < nv; ++k) {
      for (int i = 0; i < 3; ++i) o.sc.coeffs[3 * (size_t)(k0 + k) + i] = g.coeffs[3 * (size_t)k + i];
      o.sc.ncoeffs[k0 + k] = g.ncoeffs[k];
      o.sc.challenges[k0 + k] = g.challenges[k];
    }
    k0 += nv;
    rb.assign(g.challenges.begin(), g.challenges.begin() + kb);  // (:71-73)
    rc.assign(g.challenges.begin() + kb, g.challenges.end());
    if (dbg)
      fprintf(stderr, "[circuit] layer %u nv %u: tables %.1f us, sum-check %.1f us (%.1f/round), evals %.1f us\n", idx,
              nv, us(t0, st.t1), us(st.t1, st.t2), us(st.t1, st.t2) / nv, us(st.t2, LayerClock::now()));
    if (idx + 1 < sh.nlayers) {  // (:80-89)
      absorb<F>(tr, &ev[0], 1);
      alpha = challenge<F>(tr);
      absorb<F>(tr, &ev[1], 1);
      beta = challenge<F>(tr);
      o.claims.push_back(ev[0]);
      o.claims.push_back(ev[1]);
    } else {
      o.in_eval[0] = ev[0];  // what KZG::open returns for r_b / r_c (:106-111)
      o.in_eval[1] = ev[1];
    }
  }
}

// gkr::verify (gkr_protocol.rs:128-227) after the caller's checks of the
// statement: the output stage over outp (2^v Montgomery entries), then per
// layer the round checks of gkr_verify and the wiring extension at (r_b, r_c)
// per op, sum_g wt_g eq(r_b, left(l, g)) eq(r_c, right(l, g)), from four eq
// tables — the same value as the reference's dense add_i / mul_i evaluation
// (the output layer's eq([r0] ++ chal, .) is this product too). With inputs
// given, the input layer's two evaluations are recomputed from them (standing
// in for the KZG checks). last_chal: the input layer's challenges, once its
// rounds have passed.
template <class F, class Left, class Right>
bool gkr_layers_verify(zk_repr repr, const zkw::WiredShape& sh, const uint8_t* ops, Left left, Right right,
                       const zk_fe* inputs, const std::vector<Fe>& outp, const zk_fe* coeffs, const uint8_t* ncoeffs,
                       const zk_fe* claims, const zk_fe* input_evals, std::vector<Fe>* last_chal = nullptr) {
  using namespace zk;
  const uint32_t nl = sh.nlayers;
  zk_transcript tr;
  std::vector<Fe> pb, pc;
  Fe claim = gkr_output_stage<F>(&tr, outp, sh.out_vars, pb);
  Fe alpha = fe_one<F>(), beta = fe_zero<F>();
  std::vector<Fe> in_m;
  if (inputs) {
    in_m.assign((size_t)1 << sh.kb[0], fe_zero<F>());
    for (uint32_t i = 0; i < sh.ninputs; ++i) in_m[i] = in_mont<F>(repr, inputs[i]);
  }
  size_t k0 = 0;
  for (uint32_t idx = 0; idx < nl; ++idx) {
    const uint32_t l = nl - 1 - idx, G = sh.gates[l], ka = sh.ka[l], kb = sh.kb[l], nv = 2 * kb;
    std::vector<Fe> chal;
    if (!gkr_verify_rounds<F>(repr, coeffs, ncoeffs, k0, nv, &tr, claim, chal)) return false;
    k0 += nv;
    const std::vector<Fe> rb(chal.begin(), chal.begin() + kb), rc(chal.begin() + kb, chal.end());
    Fe o1, o2;
    if (idx + 1 == nl) {
      if (last_chal) *last_chal = chal;
      o1 = in_mont<F>(repr, input_evals[0]);
      o2 = in_mont<F>(repr, input_evals[1]);
      if (inputs && (!fe_eq<F>(o1, mle_eval_host<F>(in_m, rb)) || !fe_eq<F>(o2, mle_eval_host<F>(in_m, rc)))) return false;
    } else {
      o1 = in_mont<F>(repr, claims[2 * idx]);
      o2 = in_mont<F>(repr, claims[2 * idx + 1]);
    }
    const std::vector<Fe> wt = host_gate_weights<F>(pb, pc, alpha, beta, idx > 0, ka, G);
    const std::vector<Fe> el = host_eq_table<F>(rb.data(), kb), er = host_eq_table<F>(rc.data(), kb);
    Fe a_r = fe_zero<F>(), m_r = fe_zero<F>();
    const size_t g0 = sh.goff[l];
    for (uint32_t gi = 0; gi < G; ++gi) {
      const Fe wgt = hfe_mul<F>(wt[gi], hfe_mul<F>(el[left(l, gi)], er[right(l, gi)]));
      if (ops[g0 + gi]) m_r = hfe_add<F>(m_r, wgt);
      else a_r = hfe_add<F>(a_r, wgt);
    }
    const Fe expect = fe_add<F>(fe_mul<F>(a_r, fe_add<F>(o1, o2)), fe_mul<F>(m_r, fe_mul<F>(o1, o2)));
    if (!fe_eq<F>(expect, claim)) return false;
    pb = rb;
    pc = rc;
    absorb<F>(&tr, &o1, 1);
    alpha = challenge<F>(&tr);
    absorb<F>(&tr, &o2, 1);
    beta = challenge<F>(&tr);
    claim = fe_add<F>(fe_mul<F>(alpha, o1), fe_mul<F>(beta, o2));
  }
  return true;
}
}  // namespace zkh
