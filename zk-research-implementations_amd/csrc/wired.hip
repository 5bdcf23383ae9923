// GKR over a circuit with explicit wiring: host driver and C ABI.
// The protocol's host side is shared with the tree prover (gkr_layers.hpp);
// what is here is how a layer is evaluated and how its phase tables are filled
// — gathers through the wiring (wired.hpp) instead of the (2g, 2g+1) pattern.
#include "gkr_layers.hpp"

using namespace zkh;

namespace {
// A layer on the device: its gates as given, and grouped by either wire (wired_plan.hpp
// WiredCsr; `other` is the gate's second wire with its op in the top bit).
struct DevLayer {
  DevBuf ops, left, right;
  DevCsr by_left, by_right;
};
}  // namespace

struct zk_wired_circuit {
  zk_ctx* c = nullptr;
  zkw::WiredShape sh;
  std::vector<uint8_t> ops;  // host copies: the layers that run on the host
  std::vector<uint32_t> left, right;
  std::vector<DevLayer> layers;
  uint32_t kmax = 1;    // the widest table (value table or gate index), log2
  uint32_t nslots = 0;  // the most partial-sum slots a pass needs
  // proof-time buffers, sized by the shape at the first proof
  DevBuf vals, wt, eq[2], eqtmp, slots, dot;
};

namespace {
void wired_release(zk_wired_circuit* w) {
  for (auto& l : w->layers) {
    for (DevBuf* b : {&l.ops, &l.left, &l.right}) b->release();
    l.by_left.release();
    l.by_right.release();
  }
  for (DevBuf* b : {&w->vals, &w->wt, &w->eq[0], &w->eq[1], &w->eqtmp, &w->slots, &w->dot}) b->release();
  delete w;
}

constexpr auto plan_check = plan_check_with<zkw::W_OK, zkw::W_EUNSUPPORTED>;

void csr_to_device(DevCsr& d, const uint32_t* key, const uint32_t* other, const uint8_t* ops, uint32_t G,
                   uint32_t nrows) {
  const zkw::WiredCsr c = zkw::wired_csr(key, G, nrows);
  std::vector<uint32_t> oth(G);
  for (uint32_t i = 0; i < G; ++i) oth[i] = other[c.gate[i]] | (ops[c.gate[i]] ? zk::kWiredOpBit : 0u);
  to_device(d.gate, c.gate);
  d.load(c, oth);
}

// One pass over a grouping: the chunks, then the split rows' slots added into the table.
template <class F, class Kern>
void gather_pass(zk_wired_circuit* wc, const DevCsr& g, uint32_t G, Kern kern, const Fe* a, const Fe* wt, Fe* X, Fe* Y) {
  zk_ctx* c = wc->c;
  Fe* px = wc->slots.fe();
  Fe* py = px + wc->nslots;
  launch(c, ZK_K_LAYER, 72.0 * G + 76.0 * g.nchunks, 2.0 * G, kern, blocks_for(g.nchunks), a, wt,
         reinterpret_cast<const uint32_t*>(g.gate.p), reinterpret_cast<const uint32_t*>(g.other.p),
         reinterpret_cast<const zk::WiredChunk*>(g.chunks.p), g.nchunks, g.nsingle, X, Y, px, py);
  if (g.nsplit)
    launch(c, ZK_K_LAYER, 64.0 * g.nslots + 64.0 * g.nsplit, 0.0, zk::k_wired_combine<F>, g.nsplit,
           reinterpret_cast<const zk::WiredChunk*>(g.split.p), (const Fe*)px, (const Fe*)py, X, Y);
}

// The wired circuit's layers for gkr_layers_prove. A device layer's tables are those of
// wired.hpp: the row kernels, then a gather through the wiring; where a phase did not end
// on the host, w(r) = w . eq(r, .) (k_wired_dot).
template <class F>
struct WiredLayers {
  zk_wired_circuit* wc;
  const std::vector<size_t>& voff;
  std::vector<Fe> hw;

  void host_layer(uint32_t l, const std::vector<Fe>& wt, zk_transcript* tr, GkrOut& g, Fe (&ev)[2]) {
    zk_ctx* c = wc->c;
    const zkw::WiredShape& sh = wc->sh;
    hw.resize((size_t)1 << sh.kb[l]);
    HIPCK(hipMemcpyAsync(hw.data(), wc->vals.fe(voff[l]), hw.size() * 32, hipMemcpyDeviceToHost, c->stream));
    sync(c);
    const uint32_t* left = wc->left.data() + sh.goff[l];
    const uint32_t* right = wc->right.data() + sh.goff[l];
    zkh::host_layer<F>(
        hw.data(), wt, wc->ops.data() + sh.goff[l], sh.gates[l], sh.kb[l], [=](uint32_t g) { return left[g]; },
        [=](uint32_t g) { return right[g]; }, tr, g, ev);
  }

  struct Gathered {
    zk_wired_circuit* wc;
    const DevLayer& dl;
    const Fe* w;
    uint32_t G, kb;
    bool have_eqb = false;
    uint64_t L() const { return (uint64_t)1 << kb; }
    const Fe* eqb(const Fe* ch) {  // eq(r_b, .): phase 2's gather reads it, and so does eval_b
      if (!have_eqb) eq_table_device<F>(wc->c, ch, kb, wc->eq[0].fe(), wc->eqtmp.fe());
      have_eqb = true;
      return wc->eq[0].fe();
    }
    void fill1(Fe* t) {
      launch(wc->c, ZK_K_LAYER, 160.0 * L(), 0.0, zk::k_wired_rows1<F>, blocks_for(L()), w, (uint32_t)L(), t, t + L(),
             t + 2 * L(), t + 3 * L());
      gather_pass<F>(wc, dl.by_left, G, zk::k_wired_phase1<F>, w, (const Fe*)wc->wt.fe(), t + L(), t + 2 * L());
    }
    Fe eval_b(const Fe* ch) { return dot_device<F>(wc->c, wc->dot, w, eqb(ch), L()); }
    void fill2(const Fe* ch, const Fe& wrb, Fe* t) {
      const Fe* e = eqb(ch);
      launch(wc->c, ZK_K_LAYER, 160.0 * L(), (double)L(), zk::k_wired_rows2<F>, blocks_for(L()), w, (uint32_t)L(), wrb, t,
             t + L(), t + 2 * L(), t + 3 * L());
      gather_pass<F>(wc, dl.by_right, G, zk::k_wired_phase2<F>, e, (const Fe*)wc->wt.fe(), t, t + 2 * L());
    }
    Fe eval_c(const Fe* ch) {
      Fe* eqc = wc->eq[1].fe();
      eq_table_device<F>(wc->c, ch + kb, kb, eqc, wc->eqtmp.fe());
      return dot_device<F>(wc->c, wc->dot, w, eqc, L());
    }
  };

  void device_layer(uint32_t l, const std::vector<Fe>& rb, const std::vector<Fe>& rc, const Fe& alpha, const Fe& beta,
                    bool has_c, zk_transcript* tr, GkrOut& g, Fe (&ev)[2], LayerStamps&) {
    zk_ctx* c = wc->c;
    const uint32_t G = wc->sh.gates[l], ka = wc->sh.ka[l], kb = wc->sh.kb[l];
    eq_table_device<F>(c, rb.data(), ka, wc->eq[0].fe(), wc->eqtmp.fe());
    if (has_c) eq_table_device<F>(c, rc.data(), ka, wc->eq[1].fe(), wc->eqtmp.fe());
    launch(c, ZK_K_LAYER, 96.0 * G, 2.0 * G, zk::k_wired_weights<F>, blocks_for(G), (const Fe*)wc->eq[0].fe(),
           (const Fe*)wc->eq[1].fe(), alpha, beta, has_c ? 1u : 0u, G, wc->wt.fe());
    Gathered ly{wc, wc->layers[l], wc->vals.fe(voff[l]), G, kb};
    zkh::device_layer<F>(c, kb, ly, tr, g, ev);
  }
};

template <class F>
void wired_prove_device(zk_wired_circuit* wc, zk_repr repr, const zk_fe* inputs, LayersOut& o) {
  using namespace zk;
  zk_ctx* c = wc->c;
  const zkw::WiredShape& sh = wc->sh;
  const uint32_t nl = sh.nlayers, v = sh.out_vars;
  std::vector<size_t> voff(nl + 2, 0);  // table l = layer l's inputs, table nl = the outputs, each padded
  for (uint32_t l = 0; l < nl; ++l) voff[l + 1] = voff[l] + ((size_t)1 << sh.kb[l]);
  voff[nl + 1] = voff[nl] + ((size_t)1 << v);
  wc->vals.ensure(voff[nl + 1] * 32);
  wc->wt.ensure(((size_t)1 << wc->kmax) * 32);
  wc->eq[0].ensure(((size_t)1 << wc->kmax) * 32);
  wc->eq[1].ensure(((size_t)1 << wc->kmax) * 32);
  wc->eqtmp.ensure((((size_t)1 << wc->kmax) / 4 + 8) * 32);
  wc->slots.ensure(std::max<size_t>(2 * (size_t)wc->nslots, 1) * 32);
  wc->dot.ensure(64 * 32);
  upload<F>(c, repr, inputs, sh.ninputs, wc->vals.fe(0));
  if (voff[1] > sh.ninputs) HIPCK(hipMemsetAsync(wc->vals.fe(sh.ninputs), 0, (voff[1] - sh.ninputs) * 32, c->stream));
  for (uint32_t l = 0; l < nl; ++l) {  // evaluate, input -> output; each table zero-padded to its power of two
    const DevLayer& dl = wc->layers[l];
    const uint32_t n2 = 1u << sh.ka[l];
    launch(c, ZK_K_LAYER, 96.0 * sh.gates[l] + 32.0 * n2, 0.5 * sh.gates[l], k_wired_layer<F>, blocks_for(n2),
           (const Fe*)wc->vals.fe(voff[l]), reinterpret_cast<const uint8_t*>(dl.ops.p),
           reinterpret_cast<const uint32_t*>(dl.left.p), reinterpret_cast<const uint32_t*>(dl.right.p), sh.gates[l], n2,
           wc->vals.fe(voff[l + 1]));
  }
  o.out_poly.resize((size_t)1 << v);
  HIPCK(hipMemcpyAsync(o.out_poly.data(), wc->vals.fe(voff[nl]), o.out_poly.size() * 32, hipMemcpyDeviceToHost, c->stream));
  sync(c);

  zk_transcript tr;
  std::vector<Fe> r0;
  gkr_output_stage<F>(&tr, o.out_poly, v, r0);  // (the prover needs no running claim: e1 comes from the tables)
  WiredLayers<F> cir{wc, voff, {}};
  gkr_layers_prove<F>(c, sh, cir, &tr, r0, o);
}

// gkr::verify (gkr_protocol.rs:128-227) for a wired circuit: the statement's padding
// checked, then gkr_layers_verify over the wiring.
template <class F>
bool wired_verify_host(zk_repr repr, const zkw::WiredShape& sh, const uint8_t* ops, const uint32_t* left,
                       const uint32_t* right, const zk_fe* inputs, const zk_fe* output_poly, const zk_fe* coeffs,
                       const uint8_t* ncoeffs, const zk_fe* claims, const zk_fe* input_evals) {
  std::vector<Fe> outp((size_t)1 << sh.out_vars);
  for (size_t i = 0; i < outp.size(); ++i) outp[i] = in_mont<F>(repr, output_poly[i]);
  for (size_t i = sh.gates[sh.nlayers - 1]; i < outp.size(); ++i)
    if (!zk::fe_is_zero<F>(outp[i])) return false;  // the padding of the output polynomial is part of the statement
  return gkr_layers_verify<F>(
      repr, sh, ops, [&](uint32_t l, uint32_t g) { return left[sh.goff[l] + g]; },
      [&](uint32_t l, uint32_t g) { return right[sh.goff[l] + g]; }, inputs, outp, coeffs, ncoeffs, claims, input_evals);
}
}  // namespace

namespace zkh {
void wired_release_all(zk_ctx* c) {
  for (zk_wired_circuit* w : c->wired) wired_release(w);
  c->wired.clear();
}
}  // namespace zkh

extern "C" {

int zk_gkr_wired_shape(uint32_t nlayers, const uint32_t* gates, uint32_t ninputs, uint32_t* out_total_rounds,
                       uint32_t* out_output_vars) {
  return guarded([&] {
    require(out_total_rounds && out_output_vars, "null argument");
    zkw::WiredShape sh;
    const char* err = nullptr;
    plan_check(zkw::wired_shape(nlayers, gates, ninputs, sh, &err), err);
    *out_total_rounds = sh.total_rounds;
    *out_output_vars = sh.out_vars;
  });
}

int zk_gkr_wired_new(zk_ctx* c, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops, const uint32_t* left,
                     const uint32_t* right, uint32_t ninputs, zk_wired_circuit** out) {
  return guarded([&] {
    require(c && out, "null argument");
    *out = nullptr;
    zkw::WiredShape sh;
    const char* err = nullptr;
    plan_check(zkw::wired_shape(nlayers, gates, ninputs, sh, &err), err);
    plan_check(zkw::wired_validate(sh, ops, left, right, &err), err);
    bind(c);
    auto* w = new zk_wired_circuit();
    try {
      w->c = c;
      w->sh = sh;
      const size_t ng = sh.goff[nlayers];
      w->ops.assign(ops, ops + ng);
      w->left.assign(left, left + ng);
      w->right.assign(right, right + ng);
      w->layers.resize(nlayers);
      for (uint32_t l = 0; l < nlayers; ++l) {
        const size_t g0 = sh.goff[l];
        const uint32_t G = sh.gates[l];
        DevLayer& dl = w->layers[l];
        to_device(dl.ops, std::vector<uint8_t>(ops + g0, ops + g0 + G));
        to_device(dl.left, std::vector<uint32_t>(left + g0, left + g0 + G));
        to_device(dl.right, std::vector<uint32_t>(right + g0, right + g0 + G));
        csr_to_device(dl.by_left, left + g0, right + g0, ops + g0, G, sh.n_below[l]);
        csr_to_device(dl.by_right, right + g0, left + g0, ops + g0, G, sh.n_below[l]);
        w->kmax = std::max({w->kmax, sh.ka[l], sh.kb[l]});
        w->nslots = std::max({w->nslots, dl.by_left.nslots, dl.by_right.nslots});
      }
    } catch (...) {
      wired_release(w);
      throw;
    }
    c->wired.push_back(w);
    *out = w;
  });
}

void zk_gkr_wired_free(zk_wired_circuit* w) {
  if (!w) return;
  zk_ctx* c = w->c;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->wired.erase(std::remove(c->wired.begin(), c->wired.end(), w), c->wired.end());
  wired_release(w);
}

int zk_gkr_wired_prove(zk_wired_circuit* w, zk_field field, zk_repr repr, const zk_fe* inputs, zk_fe* out_output_poly,
                       zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_claims,
                       zk_fe* out_input_evals) {
  return guarded([&] {
    require(w && inputs && out_output_poly && out_coeffs && out_ncoeffs && out_challenges && out_input_evals,
            "null argument");
    require(w->sh.nlayers == 1 || out_claims, "null argument");
    bind(w->c);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      LayersOut o;
      wired_prove_device<F>(w, repr, inputs, o);
      for (size_t i = 0; i < o.out_poly.size(); ++i)  // (up to 2^24 of them: the host's 64-bit arithmetic)
        out_output_poly[i] = to_zk(repr == ZK_REPR_MONTGOMERY ? o.out_poly[i] : zk::hfe_from_mont<F>(o.out_poly[i]));
      emit_gkr<F>(repr, o.sc, (uint32_t)o.sc.ncoeffs.size(), out_coeffs, out_ncoeffs, out_challenges);
      for (size_t i = 0; i < o.claims.size(); ++i) out_claims[i] = out_repr<F>(repr, o.claims[i]);
      for (int i = 0; i < 2; ++i) out_input_evals[i] = out_repr<F>(repr, o.in_eval[i]);
    });
  });
}

int zk_gkr_wired_verify(zk_field field, zk_repr repr, uint32_t nlayers, const uint32_t* gates, const uint8_t* ops,
                        const uint32_t* left, const uint32_t* right, uint32_t ninputs, const zk_fe* inputs,
                        const zk_fe* output_poly, const zk_fe* coeffs, const uint8_t* ncoeffs, const zk_fe* claims,
                        const zk_fe* input_evals, int* out_verified) {
  return guarded([&] {
    require(output_poly && coeffs && ncoeffs && input_evals && out_verified, "null argument");
    zkw::WiredShape sh;
    const char* err = nullptr;
    plan_check(zkw::wired_shape(nlayers, gates, ninputs, sh, &err), err);
    plan_check(zkw::wired_validate(sh, ops, left, right, &err), err);
    require(nlayers == 1 || claims, "null argument");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      *out_verified =
          wired_verify_host<F>(repr, sh, ops, left, right, inputs, output_poly, coeffs, ncoeffs, claims, input_evals) ? 1 : 0;
    });
  });
}

}  // extern "C"
