// GKR over a circuit with explicit wiring: host driver and C ABI.
// The protocol and the driver's structure are the tree prover's
// (gkr_circuit.hip gkr_circuit_prove_device); what differs is how a layer is
// evaluated and how its phase tables are filled — gathers through the wiring
// (wired.hpp) instead of the (2g, 2g+1) pattern — and that every width comes
// from wired_plan.hpp instead of a halving power of two.
#include "host.hpp"
#include "wired.hpp"

using namespace zkh;

namespace {
// One grouping of a layer's gates on the device (wired_plan.hpp WiredCsr):
// `other` is the gate's second wire with its op in the top bit.
struct DevCsr {
  DevBuf gate, other, chunks, split;
  uint32_t nchunks = 0, nsingle = 0, nsplit = 0, nslots = 0;
  void release() {
    gate.release();
    other.release();
    chunks.release();
    split.release();
  }
};
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
    l.ops.release();
    l.left.release();
    l.right.release();
    l.by_left.release();
    l.by_right.release();
  }
  for (DevBuf* b : {&w->vals, &w->wt, &w->eq[0], &w->eq[1], &w->eqtmp, &w->slots, &w->dot}) b->release();
  delete w;
}

void plan_check(int rc, const char* err) {
  if (rc != zkw::W_OK) fail(rc == zkw::W_EUNSUPPORTED ? ZK_EUNSUPPORTED : ZK_EINVAL, err);
}

template <class T>
void to_device(DevBuf& b, const std::vector<T>& v) {
  b.ensure(std::max<size_t>(v.size() * sizeof(T), 16));
  if (!v.empty()) HIPCK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}
void csr_to_device(DevCsr& d, const uint32_t* key, const uint32_t* other, const uint8_t* ops, uint32_t G,
                   uint32_t nrows) {
  const zkw::WiredCsr c = zkw::wired_csr(key, G, nrows);
  std::vector<uint32_t> oth(G);
  for (uint32_t i = 0; i < G; ++i) oth[i] = other[c.gate[i]] | (ops[c.gate[i]] ? zk::kWiredOpBit : 0u);
  to_device(d.gate, c.gate);
  to_device(d.other, oth);
  to_device(d.chunks, c.chunks);
  to_device(d.split, c.split);
  d.nchunks = (uint32_t)c.chunks.size();
  d.nsingle = c.nsingle;
  d.nsplit = (uint32_t)c.split.size();
  d.nslots = d.nchunks - d.nsingle;
}

struct WiredOut {
  std::vector<Fe> out_poly;
  GkrOut sc;  // all layers' rounds, output layer first
  std::vector<Fe> claims;
  Fe in_eval[2];
};

uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + zk::kBlock - 1) / zk::kBlock); }

}  // namespace

// eq(pt[0..n), .) into dst (2^n entries), by doubling in passes of <= 3 coordinates (k_eq_table);
// the tables between passes live in tmp (< 2^(n-2) + 8 entries in all). n >= 1.
// Declared in host.hpp: zk_dev_mle_eq_table (committed.hip) builds its table here too.
template <class F>
void zkh::eq_table_device(zk_ctx* c, const Fe* pt, uint32_t n, Fe* dst, Fe* tmp) {
  const Fe* src = nullptr;
  uint32_t have = 0;
  size_t off = 0;
  while (have < n) {
    const uint32_t S = have == 0 && n % 3 ? n % 3 : 3;
    Fe* out = have + S == n ? dst : tmp + off;
    const uint32_t nsrc = 1u << have;
    zk::EqPts p{};
    for (uint32_t k = 0; k < S; ++k) p.r[k] = pt[have + k];
    const double made = (double)nsrc * (1u << S);
    auto go = [&](auto kern) { launch(c, ZK_K_LAYER, 32.0 * (nsrc + made), made, kern, blocks_for(nsrc), src, nsrc, p, out); };
    if (S == 1) go(zk::k_eq_table<F, 1>);
    else if (S == 2) go(zk::k_eq_table<F, 2>);
    else go(zk::k_eq_table<F, 3>);
    if (out != dst) off += (size_t)1 << (have + S);
    src = out;
    have += S;
  }
}
template void zkh::eq_table_device<zk::Bn254Fr>(zk_ctx*, const Fe*, uint32_t, Fe*, Fe*);
template void zkh::eq_table_device<zk::Bn254Fq>(zk_ctx*, const Fe*, uint32_t, Fe*, Fe*);
template void zkh::eq_table_device<zk::Bls12_381Fr>(zk_ctx*, const Fe*, uint32_t, Fe*, Fe*);

namespace {

// sum_j w[j] e[j] over n entries on the device (k_wired_dot), the blocks' parts added here
template <class F>
Fe dot_device(zk_wired_circuit* wc, const Fe* w, const Fe* e, uint64_t n) {
  zk_ctx* c = wc->c;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(blocks_for(n), 64);
  launch(c, ZK_K_LAYER, 64.0 * n, (double)n, zk::k_wired_dot<F>, grid, w, e, n, wc->dot.fe());
  Fe part[64];
  HIPCK(hipMemcpyAsync(part, wc->dot.fe(), grid * sizeof(Fe), hipMemcpyDeviceToHost, c->stream));
  sync(c);
  Fe s = zk::fe_zero<F>();
  for (uint32_t i = 0; i < grid; ++i) s = zk::hfe_add<F>(s, part[i]);
  return s;
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

// One layer's sum-check on the device: gkr_circuit.hip gkr_layer_two_phase with the
// tables of wired.hpp. w: the layer's 2^kb inputs, wt: its gate weights (both on the
// device). ev = {w(r_b), w(r_c)}: from the folds where a phase ended in host rounds
// (FinalVals), otherwise w . eq(r, .) (k_wired_dot).
template <class F>
void wired_layer_device(zk_wired_circuit* wc, uint32_t l, const Fe* w, zk_transcript* tr, GkrOut& out, Fe (&ev)[2]) {
  zk_ctx* c = wc->c;
  const DevLayer& dl = wc->layers[l];
  const uint32_t kb = wc->sh.kb[l], nv = 2 * kb, G = wc->sh.gates[l];
  const uint64_t L = (uint64_t)1 << kb;
  const Fe* wt = wc->wt.fe();
  out.coeffs.assign(3 * (size_t)nv, zk::fe_zero<F>());
  out.ncoeffs.assign(nv, 0);
  out.challenges.assign(nv, zk::fe_zero<F>());
  ensure_partials(c, kb);
  __atomic_store_n(h_err(c), 0u, __ATOMIC_RELAXED);
  c->work[0].ensure(4 * std::max<uint64_t>(L / 2, 1) * 32);
  c->work[1].ensure(4 * std::max<uint64_t>(L / 4, 1) * 32);
  c->input.ensure(8 * L * 32);
  Fe* t1 = c->input.fe();
  Fe* t2 = t1 + 4 * L;
  launch(c, ZK_K_LAYER, 160.0 * L, 0.0, zk::k_wired_rows1<F>, blocks_for(L), w, (uint32_t)L, t1, t1 + L, t1 + 2 * L,
         t1 + 3 * L);
  gather_pass<F>(wc, dl.by_left, G, zk::k_wired_phase1<F>, w, wt, t1 + L, t1 + 2 * L);
  const Fe* cur[4] = {t1, t1 + L, t1 + 2 * L, t1 + 3 * L};
  Fe claim = zk::fe_zero<F>(), r = zk::fe_zero<F>();
  uint32_t pend = 0;
  FinalVals f1, f2;
  gkr_phase<F>(c, cur, kb, 0, false, tr, out, claim, r, pend, true, 0, nullptr, &f1);  // rounds 0 .. kb-1 (b)
  Fe* eqb = wc->eq[0].fe();
  eq_table_device<F>(c, out.challenges.data(), kb, eqb, wc->eqtmp.fe());
  ev[0] = f1.ok ? f1.v[0] : dot_device<F>(wc, w, eqb, L);
  launch(c, ZK_K_LAYER, 160.0 * L, (double)L, zk::k_wired_rows2<F>, blocks_for(L), w, (uint32_t)L, ev[0], t2, t2 + L,
         t2 + 2 * L, t2 + 3 * L);
  gather_pass<F>(wc, dl.by_right, G, zk::k_wired_phase2<F>, (const Fe*)eqb, wt, t2, t2 + 2 * L);
  const Fe* cur2[4] = {t2, t2 + L, t2 + 2 * L, t2 + 3 * L};
  gkr_phase<F>(c, cur2, kb, kb, false, tr, out, claim, r, pend, true, 0, nullptr, &f2);  // rounds kb .. 2 kb-1 (c)
  if (f2.ok) {
    ev[1] = zk::hfe_sub<F>(f2.v[1], ev[0]);  // S = w(r_b) + w(c) folded by r_c
  } else {
    Fe* eqc = wc->eq[1].fe();
    eq_table_device<F>(c, out.challenges.data() + kb, kb, eqc, wc->eqtmp.fe());
    ev[1] = dot_device<F>(wc, w, eqc, L);
  }
  sync(c);
}

// A small layer entirely on the host (ZK_CIRCUIT_HOST_LGL): gkr_circuit.hip
// host_layer for any wiring — one loop over the gates fills the same tables.
template <class F>
void wired_layer_host(const Fe* w, const std::vector<Fe>& wt, const uint8_t* ops, const uint32_t* left,
                      const uint32_t* right, uint32_t G, uint32_t kb, zk_transcript* tr, GkrOut& out, Fe (&ev)[2]) {
  using namespace zk;
  const uint32_t nv = 2 * kb;
  const size_t L = (size_t)1 << kb;
  out.coeffs.assign(3 * (size_t)nv, fe_zero<F>());
  out.ncoeffs.assign(nv, 0);
  out.challenges.assign(nv, fe_zero<F>());
  std::vector<Fe> T[4];  // phase 1: W = w, U, V, 1
  for (auto& t : T) t.assign(L, fe_zero<F>());
  for (size_t b = 0; b < L; ++b) {
    T[0][b] = w[b];
    T[3][b] = fe_one<F>();
  }
  for (uint32_t g = 0; g < G; ++g) {
    const Fe x = wt[g], xw = hfe_mul<F>(x, w[right[g]]);
    Fe& u = T[1][left[g]];
    if (ops[g]) {
      u = hfe_add<F>(u, xw);
    } else {
      u = hfe_add<F>(u, x);
      T[2][left[g]] = hfe_add<F>(T[2][left[g]], xw);
    }
  }
  host_layer_phase<F>(T, kb, 0, tr, out);
  const Fe wrb = T[0][0];  // W = w folded by r_b
  for (auto& t : T) t.assign(L, fe_zero<F>());  // phase 2: A, S, M, P over c
  const std::vector<Fe> eqb = host_eq_table<F>(out.challenges.data(), kb);
  for (uint32_t g = 0; g < G; ++g) {
    Fe& t = (ops[g] ? T[2] : T[0])[right[g]];
    t = hfe_add<F>(t, hfe_mul<F>(wt[g], eqb[left[g]]));
  }
  for (size_t cc = 0; cc < L; ++cc) {
    T[1][cc] = hfe_add<F>(wrb, w[cc]);
    T[3][cc] = hfe_mul<F>(wrb, w[cc]);
  }
  host_layer_phase<F>(T, kb, kb, tr, out);
  ev[0] = wrb;
  ev[1] = hfe_sub<F>(T[1][0], wrb);  // S = w(r_b) + w(c) folded by r_c
}

// The output stage: absorb the 2^v padded outputs, draw r0[0..v), absorb m0 = MLE(out)(r0)
// (v = 1: initiate_protocol, gkr_protocol.rs:229-241). Returns m0.
template <class F>
Fe wired_output_stage(zk_transcript* tr, const std::vector<Fe>& outp, uint32_t v, std::vector<Fe>& r0) {
  absorb<F>(tr, outp.data(), outp.size());
  r0.clear();
  for (uint32_t k = 0; k < v; ++k) r0.push_back(challenge<F>(tr));
  const Fe m0 = mle_eval_host<F>(outp, r0);
  absorb<F>(tr, &m0, 1);
  return m0;
}

template <class F>
void wired_prove_device(zk_wired_circuit* wc, zk_repr repr, const zk_fe* inputs, WiredOut& o) {
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
  std::vector<Fe> rb, rc;  // the weights' points: r0, then the previous layer's (r_b, r_c)
  wired_output_stage<F>(&tr, o.out_poly, v, rb);  // (the prover needs no running claim: e1 comes from the tables)
  Fe alpha = fe_one<F>(), beta = fe_zero<F>();
  o.sc.coeffs.assign(3 * (size_t)sh.total_rounds, fe_zero<F>());
  o.sc.ncoeffs.assign(sh.total_rounds, 0);
  o.sc.challenges.assign(sh.total_rounds, fe_zero<F>());
  uint32_t k0 = 0;
  std::vector<Fe> hw;
  for (uint32_t idx = 0; idx < nl; ++idx) {
    const uint32_t l = nl - 1 - idx, G = sh.gates[l], ka = sh.ka[l], kb = sh.kb[l], nv = 2 * kb;
    const bool has_c = idx > 0;
    require(rb.size() == ka && (!has_c || rc.size() == ka), "internal: challenge split does not match the layer");
    const Fe* w = wc->vals.fe(voff[l]);
    GkrOut g;
    Fe ev[2];
    if (kb <= c->circuit_host_lgl) {  // gate weights, both phases and both evaluations on the host
      hw.resize((size_t)1 << kb);
      HIPCK(hipMemcpyAsync(hw.data(), w, hw.size() * 32, hipMemcpyDeviceToHost, c->stream));
      sync(c);
      const std::vector<Fe> eb = host_eq_table<F>(rb.data(), ka);
      const std::vector<Fe> ec = has_c ? host_eq_table<F>(rc.data(), ka) : std::vector<Fe>();
      std::vector<Fe> wt(G);
      for (uint32_t gi = 0; gi < G; ++gi) {
        wt[gi] = hfe_mul<F>(alpha, eb[gi]);
        if (has_c) wt[gi] = hfe_add<F>(wt[gi], hfe_mul<F>(beta, ec[gi]));
      }
      const size_t g0 = sh.goff[l];
      wired_layer_host<F>(hw.data(), wt, wc->ops.data() + g0, wc->left.data() + g0, wc->right.data() + g0, G, kb, &tr,
                          g, ev);
    } else {
      eq_table_device<F>(c, rb.data(), ka, wc->eq[0].fe(), wc->eqtmp.fe());
      if (has_c) eq_table_device<F>(c, rc.data(), ka, wc->eq[1].fe(), wc->eqtmp.fe());
      launch(c, ZK_K_LAYER, 96.0 * G, 2.0 * G, k_wired_weights<F>, blocks_for(G), (const Fe*)wc->eq[0].fe(),
             (const Fe*)wc->eq[1].fe(), alpha, beta, has_c ? 1u : 0u, G, wc->wt.fe());
      wired_layer_device<F>(wc, l, w, &tr, g, ev);
    }
    for (uint32_t k = 0; k < nv; ++k) {
      for (int i = 0; i < 3; ++i) o.sc.coeffs[3 * (size_t)(k0 + k) + i] = g.coeffs[3 * (size_t)k + i];
      o.sc.ncoeffs[k0 + k] = g.ncoeffs[k];
      o.sc.challenges[k0 + k] = g.challenges[k];
    }
    k0 += nv;
    rb.assign(g.challenges.begin(), g.challenges.begin() + kb);  // (gkr_protocol.rs:71-73)
    rc.assign(g.challenges.begin() + kb, g.challenges.end());
    if (idx + 1 < nl) {  // (:80-89)
      absorb<F>(&tr, &ev[0], 1);
      alpha = challenge<F>(&tr);
      absorb<F>(&tr, &ev[1], 1);
      beta = challenge<F>(&tr);
      o.claims.push_back(ev[0]);
      o.claims.push_back(ev[1]);
    } else {
      o.in_eval[0] = ev[0];  // what KZG::open returns for r_b / r_c (:106-111)
      o.in_eval[1] = ev[1];
    }
  }
}

// gkr::verify (gkr_protocol.rs:128-227) for a wired circuit: per layer the
// round checks of gkr_verify, then the wiring extension at (r_b, r_c) per op,
// sum_g wt_g eq(r_b, left_g) eq(r_c, right_g), from four eq tables.
template <class F>
bool wired_verify_host(zk_repr repr, const zkw::WiredShape& sh, const uint8_t* ops, const uint32_t* left,
                       const uint32_t* right, const zk_fe* inputs, const zk_fe* output_poly, const zk_fe* coeffs,
                       const uint8_t* ncoeffs, const zk_fe* claims, const zk_fe* input_evals) {
  using namespace zk;
  const uint32_t nl = sh.nlayers, v = sh.out_vars;
  std::vector<Fe> outp((size_t)1 << v);
  for (size_t i = 0; i < outp.size(); ++i) outp[i] = in_mont<F>(repr, output_poly[i]);
  for (size_t i = sh.gates[nl - 1]; i < outp.size(); ++i)
    if (!fe_is_zero<F>(outp[i])) return false;  // the padding of the output polynomial is part of the statement
  zk_transcript tr;
  std::vector<Fe> pb, pc;
  Fe claim = wired_output_stage<F>(&tr, outp, v, pb);
  Fe alpha = fe_one<F>(), beta = fe_zero<F>();
  std::vector<Fe> in_m;
  if (inputs) {
    in_m.assign((size_t)1 << sh.kb[0], fe_zero<F>());
    for (uint32_t i = 0; i < sh.ninputs; ++i) in_m[i] = in_mont<F>(repr, inputs[i]);
  }
  size_t k0 = 0;
  const Fe zero = fe_zero<F>(), one = fe_one<F>();
  for (uint32_t idx = 0; idx < nl; ++idx) {
    const uint32_t l = nl - 1 - idx, G = sh.gates[l], ka = sh.ka[l], kb = sh.kb[l], nv = 2 * kb;
    std::vector<Fe> chal;
    for (uint32_t k = 0; k < nv; ++k) {  // gkr_verify (sum_check_protocol.rs:117-150)
      const int m = ncoeffs[k0 + k];
      require(m <= 3, "round polynomial has more than 3 coefficients");
      Fe cf[3];
      for (int i = 0; i < m; ++i) cf[i] = in_mont<F>(repr, coeffs[3 * (k0 + k) + i]);
      auto at = [&](const Fe& x) {
        Fe s = zero, xp = one;
        for (int i = 0; i < m; ++i) {
          s = fe_add<F>(s, fe_mul<F>(cf[i], xp));
          xp = fe_mul<F>(xp, x);
        }
        return s;
      };
      if (!fe_eq<F>(fe_add<F>(at(zero), at(one)), claim)) return false;
      absorb<F>(&tr, cf, (size_t)m);
      const Fe r = challenge<F>(&tr);
      chal.push_back(r);
      claim = at(r);
    }
    k0 += nv;
    const std::vector<Fe> rb(chal.begin(), chal.begin() + kb), rc(chal.begin() + kb, chal.end());
    Fe o1, o2;
    if (idx + 1 == nl) {
      o1 = in_mont<F>(repr, input_evals[0]);
      o2 = in_mont<F>(repr, input_evals[1]);
      if (inputs && (!fe_eq<F>(o1, mle_eval_host<F>(in_m, rb)) || !fe_eq<F>(o2, mle_eval_host<F>(in_m, rc)))) return false;
    } else {
      o1 = in_mont<F>(repr, claims[2 * idx]);
      o2 = in_mont<F>(repr, claims[2 * idx + 1]);
    }
    const std::vector<Fe> eb = host_eq_table<F>(pb.data(), ka);
    const std::vector<Fe> ec = idx ? host_eq_table<F>(pc.data(), ka) : std::vector<Fe>();
    const std::vector<Fe> el = host_eq_table<F>(rb.data(), kb), er = host_eq_table<F>(rc.data(), kb);
    Fe a_r = zero, m_r = zero;
    const size_t g0 = sh.goff[l];
    for (uint32_t gi = 0; gi < G; ++gi) {
      Fe wgt = hfe_mul<F>(alpha, eb[gi]);
      if (idx) wgt = hfe_add<F>(wgt, hfe_mul<F>(beta, ec[gi]));
      wgt = hfe_mul<F>(wgt, hfe_mul<F>(el[left[g0 + gi]], er[right[g0 + gi]]));
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
      WiredOut o;
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
