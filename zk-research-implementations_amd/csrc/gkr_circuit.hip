// GKR over a layered circuit: host driver and C ABI.
#include "gkr_layers.hpp"

using namespace zkh;

namespace {
// ---------------------------------------------------------------------------
// GKR over a layered circuit: gkr_protocol.rs:31-126 with
// every table-sized step on the device — circuit evaluation, the four layer
// tables (kernels.hpp k_gate_weights / k_layer_tables, sparse wiring instead
// of the reference's dense 2^(3g+2) add_i/mul_i), the layer sum-check
// (gkr_prove_device) and w.evaluate(r_b / r_c) (mle_evaluate_device). The
// transcript and O(1) scalar steps stay on the host, as in the reference.
// Supported shape: the one for which the reference's table sizes agree — a
// binary tree of layers, ninputs = 2 G_0, G_{l+1} = G_l / 2, powers of two,
// output layer of 1 or 2 gates (initiate_protocol evaluates a 1-variable
// output poly, :229-241). The input-layer KZG opening (row f3) is replaced by
// returning the two input-MLE evaluations it opens (:106-111).
// ---------------------------------------------------------------------------
uint32_t lg2u(uint64_t x) {
  uint32_t k = 0;
  while (((uint64_t)1 << k) < x) ++k;
  return k;
}

void check_shape(uint32_t nlayers, const uint32_t* gates) {
  require(nlayers >= 1 && gates, "empty circuit");
  require(nlayers <= 24, "too many layers");
  for (uint32_t l = 0; l < nlayers; ++l) {
    require(gates[l] >= 1 && (gates[l] & (gates[l] - 1)) == 0, "layer sizes must be powers of two");
    if (l) require(2 * (uint64_t)gates[l] == gates[l - 1], "each layer must have half the gates of the one below");
  }
  require(gates[nlayers - 1] <= 2, "the output layer must have 1 or 2 gates");
  require(lg2u(2 * (uint64_t)gates[0]) <= 14, "circuit too large (input layer tables of (2 G_0)^2 entries)");
}

void check_circuit(uint32_t nlayers, const uint32_t* gates, const uint8_t* ops, uint32_t ninputs) {
  check_shape(nlayers, gates);
  require(ops != nullptr, "null argument");
  require((uint64_t)ninputs == 2 * (uint64_t)gates[0], "the first layer must have one gate per input pair");
  size_t nops = 0;
  for (uint32_t l = 0; l < nlayers; ++l) nops += gates[l];
  for (size_t i = 0; i < nops; ++i) require(ops[i] <= 1, "gate op must be 0 (add) or 1 (mul)");
}

uint32_t circuit_rounds(uint32_t nlayers, const uint32_t* gates) {
  uint32_t r = 0;
  for (uint32_t l = 0; l < nlayers; ++l) r += 2 * lg2u(2 * (uint64_t)gates[l]);
  return r;
}

// The circuit as the shared layer code sees it (gkr_layers.hpp): a wired
// shape whose gate g reads wires 2g and 2g + 1.
zkw::WiredShape tree_shape(uint32_t nlayers, const uint32_t* gates, uint32_t ninputs) {
  zkw::WiredShape sh;
  const char* err = nullptr;
  plan_check_with<zkw::W_OK, zkw::W_EUNSUPPORTED>(zkw::wired_shape(nlayers, gates, ninputs, sh, &err), err);
  return sh;
}
uint32_t tree_left(uint32_t g) { return 2 * g; }
uint32_t tree_right(uint32_t g) { return 2 * g + 1; }

// The tree's layers for gkr_layers_prove: every layer's values on the device
// (vals, layer l's inputs at off[l]), the host layers' values in hvals.
template <class F>
struct TreeLayers {
  zk_ctx* c;
  const zkw::WiredShape& sh;
  const uint8_t* ops;   // host
  const uint8_t* dop;   // device
  const Fe* vals;       // device
  Fe* dwt;              // device: a layer's gate weights
  const std::vector<size_t>& off;
  const std::vector<Fe>& hvals;
  size_t hbase;

  void host_layer(uint32_t l, const std::vector<Fe>& wt, zk_transcript* tr, GkrOut& g, Fe (&ev)[2]) {
    zkh::host_layer<F>(hvals.data() + (off[l] - hbase), wt, ops + sh.goff[l], sh.gates[l], sh.kb[l], tree_left,
                       tree_right, tr, g, ev);
  }

  // The two-phase tables of a tree layer (kernels.hpp k_phase1_tables / k_phase2_tables);
  // where a phase did not end on the host, k_mle_eval2 evaluates w at both points.
  struct TwoPhase {
    zk_ctx* c;
    const Fe *w, *wt;
    const uint8_t* ops;
    uint32_t lgL;
    zk::LayerPts ep{};
    uint64_t L() const { return (uint64_t)1 << lgL; }
    void points(const Fe* b, const Fe* cc) {
      for (uint32_t k = 0; k < lgL; ++k) {
        ep.r[k] = b[k];
        ep.r[lgL + k] = cc[k];
      }
    }
    void eval2(Fe (&v)[2]) {  // w at ep.r[0..lgL) and ep.r[lgL..2 lgL) on the device
      const zk::RoundSink sk = make_sink(c, false);
      launch(c, ZK_K_LAYER, 32.0 * L(), 4.0 * L(), zk::k_mle_eval2<F>, grid_for(c, L(), zk::k_mle_eval2<F>), w, lgL, ep,
             sk);
      collect_sums<F, 2>(c, sk, false, 17, v);
    }
    void fill1(Fe* t) {
      launch(c, ZK_K_LAYER, 160.0 * L(), 0.5 * L(), zk::k_phase1_tables<F>, blocks_for(L()), w, wt, ops, (uint32_t)L(),
             t, t + L(), t + 2 * L(), t + 3 * L());
    }
    Fe eval_b(const Fe* ch) {
      Fe v[2];
      points(ch, ch);
      eval2(v);
      return v[0];
    }
    void fill2(const Fe* ch, const Fe& wrb, Fe* t) {
      points(ch, ch);
      launch(c, ZK_K_LAYER, 160.0 * L(), (double)L() * (lgL + 2), zk::k_phase2_tables<F>, blocks_for(L()), w, wt, ops,
             lgL, ep, wrb, t, t + L(), t + 2 * L(), t + 3 * L());
    }
    Fe eval_c(const Fe* ch) {
      Fe v[2];
      points(ch, ch + lgL);
      eval2(v);
      return v[1];
    }
  };

  void device_layer(uint32_t l, const std::vector<Fe>& rb, const std::vector<Fe>& rc, const Fe& alpha, const Fe& beta,
                    bool has_c, zk_transcript* tr, GkrOut& g, Fe (&ev)[2], LayerStamps& st) {
    using namespace zk;
    const uint32_t G = sh.gates[l], W = sh.ka[l], lgL = sh.kb[l], nv = 2 * lgL;
    const Fe* w = vals + off[l];  // the layer's inputs
    LayerPts lp{};
    std::copy(rb.begin(), rb.end(), lp.r);
    std::copy(rc.begin(), rc.end(), lp.r + W);
    launch(c, ZK_K_LAYER, 32.0 * G, (double)G * (W + 2), k_gate_weights<F>, blocks_for(G), lp, W, alpha, beta,
           has_c ? 1u : 0u, G, dwt);
    if (!c->circuit_dense) {
      TwoPhase ly{c, w, dwt, dop + sh.goff[l], lgL};
      zkh::device_layer<F>(c, lgL, ly, tr, g, ev);
      return;
    }
    // ZK_CIRCUIT_DENSE=1: the four L^2 tables, then the generic sum-check and one fused
    // pass for o1 = w.evaluate(r_b), o2 = w.evaluate(r_c) (:75-76)
    const uint64_t T = (uint64_t)1 << nv;
    c->input.ensure(4 * T * 32);
    Fe* tab = c->input.fe();
    launch(c, ZK_K_LAYER, 128.0 * T, (double)T, k_layer_tables<F>, grid_for(c, T, k_layer_tables<F>), w, lgL, dwt,
           dop + sh.goff[l], tab, tab + T, tab + 2 * T, tab + 3 * T);
    const Fe* dT[4] = {tab, tab + T, tab + 2 * T, tab + 3 * T};
    if (circuit_debug()) {
      sync(c);
      st.t1 = LayerClock::now();
    }
    gkr_prove_device<F>(c, dT, nv, false, tr, g);  // gkr_prove(claimed_sum, &fbc_poly, &mut transcript) (:68)
    st.t2 = LayerClock::now();
    TwoPhase ly{c, w, dwt, dop + sh.goff[l], lgL};
    ly.points(g.challenges.data(), g.challenges.data() + lgL);
    ly.eval2(ev);
  }
};

template <class F>
void gkr_circuit_prove_device(zk_ctx* c, zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                              const zk_fe* inputs, uint32_t ninputs, LayersOut& o) {
  using namespace zk;
  const zkw::WiredShape sh = tree_shape(nlayers, gates, ninputs);
  ScopedBuf vals, dops, dwt;
  std::vector<size_t> off(nlayers + 1);  // layer l's inputs; off[nlayers]: the outputs
  off[0] = 0;
  for (uint32_t l = 0; l < nlayers; ++l) off[l + 1] = off[l] + sh.n_below[l];
  const size_t nvals = off[nlayers] + gates[nlayers - 1];
  vals.b.ensure(nvals * 32);
  dops.b.ensure(sh.goff[nlayers]);
  dwt.b.ensure((size_t)gates[0] * 32);
  const LayerClock::time_point t0 = LayerClock::now();
  upload<F>(c, repr, inputs, ninputs, vals.b.fe(0));
  HIPCK(hipMemcpyAsync(dops.b.p, ops, sh.goff[nlayers], hipMemcpyHostToDevice, c->stream));
  const uint8_t* dop = reinterpret_cast<const uint8_t*>(dops.b.p);
  for (uint32_t l = 0; l < nlayers; ++l)  // Circuit::evaluate, input -> output (gkr_circuit.rs:127-143)
    launch(c, ZK_K_LAYER, 96.0 * gates[l], 0.5 * gates[l], k_circuit_layer<F>, blocks_for(gates[l]), vals.b.fe(off[l]),
           dop + sh.goff[l], gates[l], vals.b.fe(off[l + 1]));
  o.out_poly.assign(2, fe_zero<F>());  // (a 1-gate output is padded with zero, :36-38)
  HIPCK(hipMemcpyAsync(o.out_poly.data(), vals.b.fe(off[nlayers]), 32 * gates[nlayers - 1], hipMemcpyDeviceToHost,
                       c->stream));
  sync(c);

  zk_transcript tr;  // Transcript::new() (:32)
  std::vector<Fe> r0;
  gkr_output_stage<F>(&tr, o.out_poly, 1, r0);  // initiate_protocol (:229-241)
  // layers with tables of <= 2^host_lgl entries run on the host (the top of the tree);
  // their inputs (the top of vals) come over in one copy
  std::vector<Fe> hvals;
  size_t hbase = nvals;
  for (uint32_t l = 0; l < nlayers; ++l)
    if (sh.kb[l] <= c->circuit_host_lgl) {
      hbase = off[l];
      break;
    }
  if (hbase < nvals) {
    hvals.resize(nvals - hbase);
    HIPCK(hipMemcpyAsync(hvals.data(), vals.b.fe(hbase), hvals.size() * 32, hipMemcpyDeviceToHost, c->stream));
    sync(c);
  }
  if (circuit_debug()) {
    sync(c);
    fprintf(stderr, "[circuit] evaluate+setup %.1f us\n",
            std::chrono::duration<double, std::micro>(LayerClock::now() - t0).count());
  }
  TreeLayers<F> cir{c, sh, ops, dop, vals.b.fe(0), dwt.b.fe(0), off, hvals, hbase};
  gkr_layers_prove<F>(c, sh, cir, &tr, r0, o);
}

// gkr::verify (gkr_protocol.rs:128-227): gkr_layers_verify over the tree's wiring.
template <class F>
bool gkr_circuit_verify_host(zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                             const zk_fe* inputs, uint32_t ninputs, const zk_fe* output_poly, const zk_fe* coeffs,
                             const uint8_t* ncoeffs, const zk_fe* claims, const zk_fe* input_evals,
                             std::vector<Fe>* last_chal = nullptr) {
  const std::vector<Fe> outp = {in_mont<F>(repr, output_poly[0]), in_mont<F>(repr, output_poly[1])};
  return gkr_layers_verify<F>(
      repr, tree_shape(nlayers, gates, ninputs), ops, [](uint32_t, uint32_t g) { return tree_left(g); },
      [](uint32_t, uint32_t g) { return tree_right(g); }, inputs, outp, coeffs, ncoeffs, claims, input_evals, last_chal);
}

}  // namespace

extern "C" {

// ---- GKR over a layered circuit ----
int zk_gkr_circuit_rounds(uint32_t nlayers, const uint32_t* gates, uint32_t* out_total_rounds) {
  return guarded([&] {
    require(gates && out_total_rounds, "null argument");
    check_shape(nlayers, gates);
    *out_total_rounds = circuit_rounds(nlayers, gates);
  });
}

int zk_gkr_circuit_prove(zk_ctx* c, zk_field field, zk_repr repr, uint32_t nlayers, const uint32_t* gates,
                         const uint8_t* ops, const zk_fe* inputs, uint32_t ninputs, zk_fe* out_output_poly,
                         zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_claims,
                         zk_fe* out_input_evals) {
  return guarded([&] {
    require(c && inputs && out_output_poly && out_coeffs && out_ncoeffs && out_challenges && out_input_evals,
            "null argument");
    check_repr(repr);
    check_circuit(nlayers, gates, ops, ninputs);
    require(nlayers == 1 || out_claims, "null argument");
    bind(c);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      LayersOut o;
      gkr_circuit_prove_device<F>(c, repr, nlayers, gates, ops, inputs, ninputs, o);
      for (int i = 0; i < 2; ++i) out_output_poly[i] = out_repr<F>(repr, o.out_poly[i]);
      emit_gkr<F>(repr, o.sc, (uint32_t)o.sc.ncoeffs.size(), out_coeffs, out_ncoeffs, out_challenges);
      for (size_t i = 0; i < o.claims.size(); ++i) out_claims[i] = out_repr<F>(repr, o.claims[i]);
      for (int i = 0; i < 2; ++i) out_input_evals[i] = out_repr<F>(repr, o.in_eval[i]);
    });
  });
}

int zk_gkr_circuit_verify(zk_field field, zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                          const zk_fe* inputs, uint32_t ninputs, const zk_fe* output_poly, const zk_fe* coeffs,
                          const uint8_t* ncoeffs, const zk_fe* claims, const zk_fe* input_evals, int* out_verified) {
  return guarded([&] {
    require(output_poly && coeffs && ncoeffs && input_evals && out_verified, "null argument");
    check_repr(repr);
    check_circuit(nlayers, gates, ops, ninputs);
    require(nlayers == 1 || claims, "null argument");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      *out_verified = gkr_circuit_verify_host<F>(repr, nlayers, gates, ops, inputs, ninputs, output_poly, coeffs,
                                                 ncoeffs, claims, input_evals)
                          ? 1
                          : 0;
    });
  });
}

// ---- gkr::prove / gkr::verify with the input layer's KZG step (gkr_protocol.rs:92-118, :155-175) ----
// A composition of the entry points above: the circuit proof (GPU), then
// KZG::new over the caller's taus (GPU setup), commit (GPU MSM), the two
// openings KZG::open returns (= the input evaluations the circuit prover
// computed at r_b, r_c) and their get_proofs (GPU), and the G2 taus.
int zk_gkr_circuit_prove_kzg(zk_ctx* c, zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                             const zk_fe* inputs, uint32_t ninputs, const zk_fe* taus, zk_fe* out_output_poly,
                             zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_claims,
                             zk_fe* out_input_evals, zk_g1* out_commitment, zk_g1* out_proofs, zk_g2* out_g2_taus) {
  int rc = guarded([&] {
    require(c && inputs && taus && out_commitment && out_proofs && out_g2_taus && out_challenges, "null argument");
    check_circuit(nlayers, gates, ops, ninputs);
  });
  if (rc != ZK_OK) return rc;
  rc = zk_gkr_circuit_prove(c, ZK_BLS12_381_FR, repr, nlayers, gates, ops, inputs, ninputs, out_output_poly,
                            out_coeffs, out_ncoeffs, out_challenges, out_claims, out_input_evals);
  if (rc != ZK_OK) return rc;
  const uint32_t nin = lg2u(ninputs);
  const uint32_t total = circuit_rounds(nlayers, gates);
  const zk_fe* rb = out_challenges + (total - 2 * nin);  // the input layer's sum-check: (r_b, r_c) (:71-73)
  const zk_fe* rcp = rb + nin;
  zk_kzg* k = nullptr;
  rc = zk_kzg_setup(c, repr, taus, nin, &k);  // KZG::new(&input_poly, taus) (:105)
  if (rc == ZK_OK) rc = zk_kzg_commit(c, k, repr, inputs, out_commitment);  // :106
  if (rc == ZK_OK) rc = zk_kzg_get_proof(c, k, repr, inputs, &out_input_evals[0], rb, out_proofs);  // :108-110
  if (rc == ZK_OK) rc = zk_kzg_get_proof(c, k, repr, inputs, &out_input_evals[1], rcp, out_proofs + nin);  // :112-113
  if (rc == ZK_OK) rc = zk_kzg_g2_taus(k, out_g2_taus);
  zk_kzg_free(k);
  return rc;
}

int zk_gkr_circuit_verify_kzg(zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                              const zk_fe* output_poly, const zk_fe* coeffs, const uint8_t* ncoeffs,
                              const zk_fe* claims, const zk_fe* opened_evals, const zk_g1* commitment,
                              const zk_g1* proofs, const zk_g2* g2_taus, int* out_verified) {
  std::vector<zk::Fe> chal;
  uint32_t ninputs = 0;
  int rc = guarded([&] {
    require(output_poly && coeffs && ncoeffs && opened_evals && commitment && proofs && g2_taus && out_verified,
            "null argument");
    require(nlayers >= 1 && gates, "null argument");
    ninputs = 2 * gates[0];
    check_circuit(nlayers, gates, ops, ninputs);
    require(nlayers == 1 || claims, "null argument");
    *out_verified = gkr_circuit_verify_host<zk::Bls12_381Fr>(repr, nlayers, gates, ops, nullptr, ninputs, output_poly,
                                                         coeffs, ncoeffs, claims, opened_evals, &chal)
                        ? 1
                        : 0;
  });
  if (rc != ZK_OK || !*out_verified) return rc;
  // KZG::verify of both openings at (r_b, r_c), the verifier's own challenges (:155-175)
  const uint32_t nin = lg2u(ninputs);
  if (chal.size() != 2 * (size_t)nin) {  // the sum-check failed before the input layer
    *out_verified = 0;
    return ZK_OK;
  }
  std::vector<zk_fe> pts(2 * (size_t)nin);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = out_repr<zk::Bls12_381Fr>(repr, chal[i]);
  int okb = 0, okc = 0;
  rc = zk_kzg_verify(repr, commitment, &opened_evals[0], proofs, nin, pts.data(), nin, g2_taus, &okb);
  if (rc == ZK_OK) rc = zk_kzg_verify(repr, commitment, &opened_evals[1], proofs + nin, nin, pts.data() + nin, nin,
                                      g2_taus, &okc);
  *out_verified = rc == ZK_OK && okb && okc;
  return rc;
}

}  // extern "C"
