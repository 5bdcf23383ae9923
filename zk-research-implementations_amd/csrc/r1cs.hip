// R1CS satisfiability by two sum-checks over a committed witness (DESIGN.md
// 6k): host driver and C ABI. The prover is calls on one transcript, in the
// order r1cs_plan.hpp fixes: the row pass (r1cs.hpp) fills Az, Bz, Cz, the
// composed sum-check (composed.hip, called, not copied) proves the zero-check,
// the column pass builds M, the composed sum-check again reduces it to one
// evaluation of z, and KZG (kzg.hip) closes on the witness.
#include "host.hpp"
#include "r1cs.hpp"

using namespace zkh;

namespace {
// One grouping of the entries on the device (r1cs_plan.hpp R1csGroup): the
// shared layout and the entries' values in its order.
struct DevGroup {
  DevCsr csr;
  DevBuf vals;
};
}  // namespace

struct zk_r1cs {
  zk_ctx* c = nullptr;  // null: host-only
  int device = -1;      // c's device, kept so that freeing the handle never reads the context
  zk_field field = ZK_BN254_FR;
  zkr::R1csShape sh;
  std::vector<uint32_t> rows, cols;  // host copies: the digest's order
  std::vector<Fe> vm;                // the values, Montgomery
  uint8_t digest[32] = {0};
  DevGroup by_row, by_col;
  uint32_t nslots = 0;  // the most partial-sum slots a pass needs
  // proof-time buffers, sized by the shape at first use
  DevBuf tabs, slots, dot;
};

namespace {
constexpr auto plan_check = plan_check_with<zkr::R_OK, zkr::R_EUNSUPPORTED>;

void r1cs_release(zk_r1cs* r) {
  for (DevGroup* g : {&r->by_row, &r->by_col}) {
    g->csr.release();
    g->vals.release();
  }
  for (DevBuf* b : {&r->tabs, &r->slots, &r->dot}) b->release();
  delete r;
}

void group_to_device(DevGroup& d, const zk_r1cs* r, bool by_row) {
  const zkr::R1csGroup g = zkr::r1cs_group(r->sh, r->rows.data(), r->cols.data(), by_row);
  std::vector<Fe> vals(g.other.size());
  for (size_t i = 0; i < vals.size(); ++i) vals[i] = r->vm[g.csr.gate[i]];
  d.csr.load(g.csr, g.other);
  to_device(d.vals, vals);
}

// The handle's tables, in elements: six of 2^sx for sum-check 1, then of 2^sy
// each: M, z, an eq table, and three columns for the matrices kept apart.
struct Tabs {
  uint64_t X, Y;
  Fe* base;
  Fe* t1(int i) const { return base + (uint64_t)i * X; }
  Fe* m() const { return base + 6 * X; }
  Fe* z() const { return base + 6 * X + Y; }
  Fe* e() const { return base + 6 * X + 2 * Y; }
  Fe* col(int i) const { return base + 6 * X + (3 + (uint64_t)i) * Y; }
};
Tabs tabs_of(zk_r1cs* r) {
  const uint64_t X = (uint64_t)1 << r->sh.sx, Y = (uint64_t)1 << r->sh.sy;
  r->tabs.ensure((6 * X + 6 * Y) * 32);
  r->slots.ensure(std::max<size_t>(3 * (size_t)r->nslots, 1) * 32);
  r->dot.ensure(64 * 32);
  return Tabs{X, Y, r->tabs.fe()};
}

// One pass over a grouping into `nout` rows of NC columns: zero, the chunks,
// then the split rows' slots added in.
template <class F, int NC>
void gather_pass(zk_r1cs* r, const DevGroup& dg, const Fe* x, uint32_t nout, const Fe& rho, const Fe& rho2, Fe* o0,
                 Fe* o1, Fe* o2) {
  zk_ctx* c = r->c;
  const DevCsr& g = dg.csr;
  const double n = (double)r->sh.total();
  Fe* p0 = r->slots.fe();
  Fe* p1 = p0 + r->nslots;
  Fe* p2 = p1 + r->nslots;
  launch(c, ZK_K_LAYER, 32.0 * NC * nout, 0.0, zk::k_r1cs_zero<F, NC>, blocks_for(nout), nout, o0, o1, o2);
  if (g.nchunks)
    launch(c, ZK_K_LAYER, 68.0 * n + (12.0 + 32.0 * NC) * g.nchunks, n, zk::k_r1cs_gather<F, NC>, blocks_for(g.nchunks),
           x, (const Fe*)dg.vals.fe(), reinterpret_cast<const uint32_t*>(g.other.p),
           reinterpret_cast<const zk::WiredChunk*>(g.chunks.p), g.nchunks, g.nsingle, rho, rho2, o0, o1, o2, p0, p1,
           p2);
  if (g.nsplit)
    launch(c, ZK_K_LAYER, 32.0 * NC * (g.nslots + g.nsplit), 0.0, zk::k_r1cs_combine<F, NC>, g.nsplit,
           reinterpret_cast<const zk::WiredChunk*>(g.split.p), (const Fe*)p0, (const Fe*)p1, (const Fe*)p2, o0, o1,
           o2);
}

// eq(pt[0..n), .) into d_out through the public builder (Montgomery scalars)
template <class F>
void eq_table(zk_r1cs* r, const Fe* pt, uint32_t n, Fe* d_out) {
  std::vector<zk_fe> p(std::max<uint32_t>(n, 1));
  for (uint32_t i = 0; i < n; ++i) p[i] = to_zk(pt[i]);
  pass_on(zk_dev_mle_eq_table(r->c, r->field, ZK_REPR_MONTGOMERY, p.data(), n, d_out));
}

template <class F>
void matrix_evals_device(zk_r1cs* r, const Fe* rx, const Fe* ry, Fe (&out)[3]) {
  const Tabs t = tabs_of(r);
  eq_table<F>(r, rx, r->sh.sx, t.t1(0));
  const Fe zero = zk::fe_zero<F>();
  gather_pass<F, 3>(r, r->by_col, t.t1(0), (uint32_t)t.Y, zero, zero, t.col(0), t.col(1), t.col(2));
  eq_table<F>(r, ry, r->sh.sy, t.e());
  for (int k = 0; k < 3; ++k) out[k] = dot_device<F>(r->c, r->dot, t.col(k), t.e(), t.Y);
}

struct ProveArgs {
  const zk_fe* io;
  const zk_kzg* kzg;
  const zk_g1* commitment_in;
  zk_transcript* transcript;
  zk_fe *out_coeffs1, *out_coeffs2, *out_evals, *out_rx, *out_ry;
  uint8_t *out_ncoeffs1, *out_ncoeffs2;
  zk_g1 *out_commitment, *out_opening;
};

void check_prove_args(const zk_r1cs* r, zk_repr repr, const void* witness, const ProveArgs& a) {
  require(r && witness && a.transcript && a.out_coeffs1 && a.out_ncoeffs1 && a.out_coeffs2 && a.out_ncoeffs2 &&
              a.out_evals && a.out_rx && a.out_ry,
          "null argument");
  require(a.io || r->sh.npub == 0, "null argument");
  check_repr(repr);
  if (a.kzg) {
    require(a.out_commitment && a.out_opening, "null argument");
    require(r->field == ZK_BLS12_381_FR, "the KZG closing is over BLS12-381 Fr");
    require(r->sh.sy >= 2 && kzg_nvars(a.kzg) == r->sh.sy - 1, "the KZG setup must have sy - 1 variables");
  }
  if (!r->c) fail(ZK_EDEVICE, "a host-only R1CS handle cannot prove");
}

// The proof over a Montgomery witness on the device. Everything is collected
// in locals, the transcript included, and handed out only at the end: nothing
// is written on failure.
template <class F>
void prove_device(zk_r1cs* r, zk_repr repr, const Fe* d_w, const ProveArgs& a) {
  using namespace zk;
  zk_ctx* c = r->c;
  const zkr::R1csShape& sh = r->sh;
  const uint32_t sx = sh.sx, sy = sh.sy, npub = sh.npub;
  std::vector<Fe> io(npub);
  for (uint32_t k = 0; k < npub; ++k) io[k] = in_mont<F>(repr, a.io[k]);
  const Tabs t = tabs_of(r);
  const uint64_t H = t.Y / 2;

  zk_g1 cm{};
  if (a.kzg) {
    if (a.commitment_in) {  // absorbed and returned as given (its encoding checked, not recomputed)
      cm = *a.commitment_in;
      check_g1_points(&cm, 1);
    } else {
      pass_on(zk_dev_kzg_commit(c, a.kzg, d_w, &cm));
    }
  }
  // z = (w | 1, io, 0 ..)
  std::vector<Fe> pub(npub + 1);
  for (uint32_t j = 0; j <= npub; ++j) pub[j] = zkr::r1cs_public_entry<F>(io.data(), npub, j);
  HIPCK(hipMemcpyAsync(t.z(), d_w, H * 32, hipMemcpyDeviceToDevice, c->stream));
  HIPCK(hipMemcpyAsync(t.z() + H, pub.data(), pub.size() * 32, hipMemcpyHostToDevice, c->stream));
  if (H > pub.size()) HIPCK(hipMemsetAsync(t.z() + H + pub.size(), 0, (H - pub.size()) * 32, c->stream));
  sync(c);  // (pub is read by the copy)

  zk_transcript tr = *a.transcript;
  zkr::R1csProof<F> p;
  zkr::r1cs_begin<F>(&tr, r->digest, io.data(), npub, a.kzg ? reinterpret_cast<const uint64_t*>(&cm) : nullptr);
  zkr::r1cs_draw_tau<F>(&tr, sx, p.tau);

  // sum-check 1 over [eq, Az, Bz, -eq, Cz, 1]
  const Fe zero = fe_zero<F>(), one = fe_one<F>();
  eq_table<F>(r, p.tau.data(), sx, t.t1(0));
  gather_pass<F, 3>(r, r->by_row, t.z(), (uint32_t)t.X, zero, zero, t.t1(1), t.t1(2), t.t1(4));
  {
    const void* src[1] = {t.t1(0)};
    const zk_fe minus1 = to_zk(hfe_sub<F>(zero, one)), k0 = to_zk(zero), k1 = to_zk(one);
    pass_on(zk_dev_mle_lincomb(c, r->field, ZK_REPR_MONTGOMERY, src, 1, &minus1, nullptr, t.X, t.t1(3)));
    pass_on(zk_dev_mle_lincomb(c, r->field, ZK_REPR_MONTGOMERY, src, 1, &k0, &k1, t.X, t.t1(5)));
  }
  const zk_fe zzero = to_zk(zero);
  zk_fe cs;
  {
    const void* dT[6];
    for (int i = 0; i < 6; ++i) dT[i] = t.t1(i);
    std::vector<zk_fe> cf((size_t)4 * sx), ch(sx);
    std::vector<uint8_t> nco(sx);
    zk_fe ev[6];
    pass_on(zk_dev_composed_sumcheck_prove(c, r->field, ZK_REPR_MONTGOMERY, dT, 6, sx, zkr::kSc1Factors, 2,
                                           zkr::kSc1Degree, &zzero, &tr, cf.data(), nco.data(), ch.data(), ev, &cs));
    p.sc1.ncoeffs = nco;
    for (const zk_fe& x : cf) p.sc1.coeffs.push_back(from_zk(x));
    for (const zk_fe& x : ch) p.sc1.challenges.push_back(from_zk(x));
    p.va = from_zk(ev[1]);
    p.vb = from_zk(ev[2]);
    p.vc = from_zk(ev[4]);
  }
  p.rho = zkr::r1cs_draw_rho<F>(&tr, p.va, p.vb, p.vc);

  // sum-check 2 over [M, z]
  eq_table<F>(r, p.sc1.challenges.data(), sx, t.t1(0));
  gather_pass<F, 1>(r, r->by_col, t.t1(0), (uint32_t)t.Y, p.rho, hfe_mul<F>(p.rho, p.rho), t.m(), nullptr, nullptr);
  {
    const void* dT[2] = {t.m(), t.z()};
    const zk_fe claim = to_zk(zkr::r1cs_rho_combine<F>(p.rho, p.va, p.vb, p.vc));
    std::vector<zk_fe> cf((size_t)3 * sy), ch(sy);
    std::vector<uint8_t> nco(sy);
    zk_fe ev[2];
    pass_on(zk_dev_composed_sumcheck_prove(c, r->field, ZK_REPR_MONTGOMERY, dT, 2, sy, zkr::kSc2Factors, 1,
                                           zkr::kSc2Degree, &claim, &tr, cf.data(), nco.data(), ch.data(), ev, &cs));
    p.sc2.ncoeffs = nco;
    for (const zk_fe& x : cf) p.sc2.coeffs.push_back(from_zk(x));
    for (const zk_fe& x : ch) p.sc2.challenges.push_back(from_zk(x));
  }
  const Fe* ry = p.sc2.challenges.data();
  if (sy == 1) {  // w is one value
    HIPCK(hipMemcpyAsync(&p.vw, d_w, 32, hipMemcpyDeviceToHost, c->stream));
    sync(c);
  } else {
    eq_table<F>(r, ry + 1, sy - 1, t.e());
    p.vw = dot_device<F>(r->c, r->dot, d_w, t.e(), H);
  }
  absorb<F>(&tr, &p.vw, 1);
  std::vector<zk_g1> opening;
  if (a.kzg) {
    opening.resize(sy - 1);
    std::vector<zk_fe> pt(sy - 1);
    for (uint32_t k = 0; k + 1 < sy; ++k) pt[k] = to_zk(ry[k + 1]);
    const zk_fe vw = to_zk(p.vw);
    pass_on(zk_dev_kzg_get_proof(c, a.kzg, ZK_REPR_MONTGOMERY, d_w, &vw, pt.data(), opening.data()));
  }

  for (size_t i = 0; i < p.sc1.coeffs.size(); ++i) a.out_coeffs1[i] = out_repr<F>(repr, p.sc1.coeffs[i]);
  for (size_t i = 0; i < p.sc2.coeffs.size(); ++i) a.out_coeffs2[i] = out_repr<F>(repr, p.sc2.coeffs[i]);
  std::copy(p.sc1.ncoeffs.begin(), p.sc1.ncoeffs.end(), a.out_ncoeffs1);
  std::copy(p.sc2.ncoeffs.begin(), p.sc2.ncoeffs.end(), a.out_ncoeffs2);
  const Fe ev[4] = {p.va, p.vb, p.vc, p.vw};
  for (int i = 0; i < 4; ++i) a.out_evals[i] = out_repr<F>(repr, ev[i]);
  for (uint32_t k = 0; k < sx; ++k) a.out_rx[k] = out_repr<F>(repr, p.sc1.challenges[k]);
  for (uint32_t k = 0; k < sy; ++k) a.out_ry[k] = out_repr<F>(repr, p.sc2.challenges[k]);
  if (a.kzg) {
    *a.out_commitment = cm;
    std::copy(opening.begin(), opening.end(), a.out_opening);
  }
  *a.transcript = tr;
}
}  // namespace

extern "C" {

int zk_r1cs_new(zk_ctx* c, zk_field field, zk_repr repr, uint32_t nrows, uint32_t sy, uint32_t npub,
                const uint32_t nnz[3], const uint32_t* rows, const uint32_t* cols, const zk_fe* vals, zk_r1cs** out) {
  return guarded([&] {
    require(out && nnz, "null argument");
    check_repr(repr);
    zkr::R1csShape sh;
    const char* err = nullptr;
    plan_check(zkr::r1cs_shape((uint32_t)field, nrows, sy, npub, nnz, sh, &err), err);
    std::unique_ptr<zk_r1cs> h(new zk_r1cs());
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      plan_check(zkr::r1cs_entries<F>(sh, rows, cols, reinterpret_cast<const uint64_t*>(vals),
                                      repr == ZK_REPR_MONTGOMERY, h->vm, &err),
                 err);
      zkr::r1cs_digest<F>(sh, rows, cols, h->vm.data(), h->digest);
    });
    h->c = c;
    h->device = c ? c->device : -1;
    h->field = field;
    h->sh = sh;
    h->rows.assign(rows, rows + sh.total());
    h->cols.assign(cols, cols + sh.total());
    zk_r1cs* r = h.release();
    if (c) {
      try {
        bind(c);
        group_to_device(r->by_row, r, true);
        group_to_device(r->by_col, r, false);
        r->nslots = std::max(r->by_row.csr.nslots, r->by_col.csr.nslots);
      } catch (...) {
        r1cs_release(r);
        throw;
      }
    }
    *out = r;
  });
}

void zk_r1cs_free(zk_r1cs* r) {
  if (!r) return;
  if (r->device >= 0) {  // (the context may be gone already: only the device is named)
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
  }
  r1cs_release(r);
}

int zk_r1cs_shape(const zk_r1cs* r, uint32_t* out_sx, uint32_t* out_sy, uint32_t* out_rounds1, uint32_t* out_rounds2,
                  uint8_t out_digest[32]) {
  return guarded([&] {
    require(r != nullptr, "null argument");
    if (out_sx) *out_sx = r->sh.sx;
    if (out_sy) *out_sy = r->sh.sy;
    if (out_rounds1) *out_rounds1 = r->sh.sx;
    if (out_rounds2) *out_rounds2 = r->sh.sy;
    if (out_digest) memcpy(out_digest, r->digest, 32);
  });
}

int zk_r1cs_mul(zk_r1cs* r, zk_repr repr, const zk_fe* z, zk_fe* out_az, zk_fe* out_bz, zk_fe* out_cz) {
  return guarded([&] {
    require(r && z && out_az && out_bz && out_cz, "null argument");
    check_repr(repr);
    dispatch(r->field, [&](auto f) {
      using F = decltype(f);
      const uint64_t X = (uint64_t)1 << r->sh.sx, Y = (uint64_t)1 << r->sh.sy;
      zk_fe* const outs[3] = {out_az, out_bz, out_cz};
      if (!r->c) {  // host-only handle: O(entries) on the host
        std::vector<Fe> zm(Y), abc[3];
        for (uint64_t j = 0; j < Y; ++j) zm[j] = in_mont<F>(repr, z[j]);
        zkr::r1cs_host_mul<F>(r->sh, r->rows.data(), r->cols.data(), r->vm.data(), zm.data(), abc);
        for (int k = 0; k < 3; ++k)
          for (uint64_t i = 0; i < X; ++i) outs[k][i] = out_repr<F>(repr, abc[k][i]);
        return;
      }
      for (uint64_t j = 0; j < Y; ++j) (void)in_mont<F>(repr, z[j]);  // < p, before anything is written
      bind(r->c);
      const Tabs t = tabs_of(r);
      upload<F>(r->c, repr, z, Y, t.z());
      const Fe zero = zk::fe_zero<F>();
      gather_pass<F, 3>(r, r->by_row, t.z(), (uint32_t)X, zero, zero, t.t1(1), t.t1(2), t.t1(4));
      const int src[3] = {1, 2, 4};
      std::vector<zk_fe> tmp(3 * X);
      for (int k = 0; k < 3; ++k) download<F>(r->c, repr, t.t1(src[k]), X, tmp.data() + k * X);
      for (int k = 0; k < 3; ++k) std::copy(tmp.begin() + k * X, tmp.begin() + (k + 1) * X, outs[k]);
    });
  });
}

int zk_dev_r1cs_mul(zk_r1cs* r, const void* d_z, void* d_az, void* d_bz, void* d_cz) {
  return guarded([&] {
    require(r && d_z && d_az && d_bz && d_cz, "null argument");
    if (!r->c) fail(ZK_EDEVICE, "a host-only R1CS handle has no device");
    dispatch(r->field, [&](auto f) {
      using F = decltype(f);
      bind(r->c);
      (void)tabs_of(r);  // (the slots)
      const Fe zero = zk::fe_zero<F>();
      gather_pass<F, 3>(r, r->by_row, reinterpret_cast<const Fe*>(d_z), 1u << r->sh.sx, zero, zero,
                        reinterpret_cast<Fe*>(d_az), reinterpret_cast<Fe*>(d_bz), reinterpret_cast<Fe*>(d_cz));
      sync(r->c);
    });
  });
}

int zk_dev_r1cs_mul_t(zk_r1cs* r, const void* d_x, void* d_atx, void* d_btx, void* d_ctx) {
  return guarded([&] {
    require(r && d_x && d_atx && d_btx && d_ctx, "null argument");
    if (!r->c) fail(ZK_EDEVICE, "a host-only R1CS handle has no device");
    dispatch(r->field, [&](auto f) {
      using F = decltype(f);
      bind(r->c);
      (void)tabs_of(r);  // (the slots)
      const Fe zero = zk::fe_zero<F>();
      gather_pass<F, 3>(r, r->by_col, reinterpret_cast<const Fe*>(d_x), 1u << r->sh.sy, zero, zero,
                        reinterpret_cast<Fe*>(d_atx), reinterpret_cast<Fe*>(d_btx), reinterpret_cast<Fe*>(d_ctx));
      sync(r->c);
    });
  });
}

int zk_r1cs_matrix_evals(zk_r1cs* r, zk_repr repr, const zk_fe* rx, const zk_fe* ry, zk_fe out[3]) {
  return guarded([&] {
    require(r && rx && ry && out, "null argument");
    check_repr(repr);
    dispatch(r->field, [&](auto f) {
      using F = decltype(f);
      std::vector<Fe> px(r->sh.sx), py(r->sh.sy);
      for (uint32_t k = 0; k < r->sh.sx; ++k) px[k] = in_mont<F>(repr, rx[k]);
      for (uint32_t k = 0; k < r->sh.sy; ++k) py[k] = in_mont<F>(repr, ry[k]);
      Fe m[3];
      if (r->c) {
        bind(r->c);
        matrix_evals_device<F>(r, px.data(), py.data(), m);
      } else {
        zkr::r1cs_host_matrix_evals<F>(r->sh, r->rows.data(), r->cols.data(), r->vm.data(), px.data(), py.data(), m);
      }
      for (int k = 0; k < 3; ++k) out[k] = out_repr<F>(repr, m[k]);
    });
  });
}

int zk_dev_r1cs_prove(zk_r1cs* r, zk_repr repr, const void* d_witness, const zk_fe* io, const zk_kzg* kzg,
                      const zk_g1* commitment_in, zk_transcript* transcript, zk_fe* out_coeffs1,
                      uint8_t* out_ncoeffs1, zk_fe* out_coeffs2, uint8_t* out_ncoeffs2, zk_fe out_evals[4],
                      zk_fe* out_rx, zk_fe* out_ry, zk_g1* out_commitment, zk_g1* out_opening) {
  return guarded([&] {
    const ProveArgs a{io, kzg, commitment_in, transcript, out_coeffs1, out_coeffs2, out_evals, out_rx, out_ry,
                      out_ncoeffs1, out_ncoeffs2, out_commitment, out_opening};
    check_prove_args(r, repr, d_witness, a);
    bind(r->c);
    dispatch(r->field, [&](auto f) { prove_device<decltype(f)>(r, repr, reinterpret_cast<const Fe*>(d_witness), a); });
  });
}

int zk_r1cs_prove(zk_r1cs* r, zk_repr repr, const zk_fe* witness, const zk_fe* io, const zk_kzg* kzg,
                  const zk_g1* commitment_in, zk_transcript* transcript, zk_fe* out_coeffs1, uint8_t* out_ncoeffs1,
                  zk_fe* out_coeffs2, uint8_t* out_ncoeffs2, zk_fe out_evals[4], zk_fe* out_rx, zk_fe* out_ry,
                  zk_g1* out_commitment, zk_g1* out_opening) {
  return guarded([&] {
    const ProveArgs a{io, kzg, commitment_in, transcript, out_coeffs1, out_coeffs2, out_evals, out_rx, out_ry,
                      out_ncoeffs1, out_ncoeffs2, out_commitment, out_opening};
    check_prove_args(r, repr, witness, a);
    bind(r->c);
    dispatch(r->field, [&](auto f) {
      using F = decltype(f);
      const uint64_t H = (uint64_t)1 << (r->sh.sy - 1);
      ScopedBuf up;  // the witness goes up once, for both sum-checks, the commitment and the opening
      up.b.ensure(H * 32);
      upload<F>(r->c, repr, witness, H, up.b.fe());
      prove_device<F>(r, repr, up.b.fe(), a);
      sync(r->c);  // (nothing of the stream still reads `up`)
    });
  });
}

int zk_r1cs_verify(zk_r1cs* r, zk_repr repr, const zk_fe* io, const zk_fe* coeffs1, const uint8_t* ncoeffs1,
                   const zk_fe* coeffs2, const uint8_t* ncoeffs2, const zk_fe evals[4], const zk_g1* commitment,
                   const zk_g1* opening, const zk_g2* g2_taus, zk_transcript* transcript, int* out_verified,
                   zk_fe* out_rx, zk_fe* out_ry) {
  return guarded([&] {
    require(r && coeffs1 && ncoeffs1 && coeffs2 && ncoeffs2 && evals && transcript && out_verified && out_rx && out_ry,
            "null argument");
    require(io || r->sh.npub == 0, "null argument");
    check_repr(repr);
    const bool committed = commitment != nullptr;
    require(committed ? (opening && g2_taus) : (!opening && !g2_taus),
            "commitment, opening and g2_taus are given together or not at all");
    const uint32_t sx = r->sh.sx, sy = r->sh.sy, npub = r->sh.npub;
    if (committed) {
      require(r->field == ZK_BLS12_381_FR, "the KZG closing is over BLS12-381 Fr");
      require(sy >= 2, "a committed witness needs sy >= 2");
      check_g1_points(commitment, 1);
      check_g1_points(opening, sy - 1);
    }
    dispatch(r->field, [&](auto f) {
      using F = decltype(f);
      std::vector<Fe> iom(npub), cf1((size_t)4 * sx, zk::fe_zero<F>()), cf2((size_t)3 * sy, zk::fe_zero<F>());
      for (uint32_t k = 0; k < npub; ++k) iom[k] = in_mont<F>(repr, io[k]);
      for (uint32_t k = 0; k < sx; ++k)
        for (uint32_t i = 0; i < std::min<uint32_t>(ncoeffs1[k], 4); ++i) cf1[4 * k + i] = in_mont<F>(repr, coeffs1[4 * k + i]);
      for (uint32_t k = 0; k < sy; ++k)
        for (uint32_t i = 0; i < std::min<uint32_t>(ncoeffs2[k], 3); ++i) cf2[3 * k + i] = in_mont<F>(repr, coeffs2[3 * k + i]);
      Fe ev[4];
      for (int i = 0; i < 4; ++i) ev[i] = in_mont<F>(repr, evals[i]);
      if (r->c) bind(r->c);
      zk_transcript tr = *transcript;
      std::vector<Fe> rx, ry;
      auto matrix_evals = [&](const Fe* px, const Fe* py, Fe (&m)[3]) {
        if (r->c) matrix_evals_device<F>(r, px, py, m);
        else zkr::r1cs_host_matrix_evals<F>(r->sh, r->rows.data(), r->cols.data(), r->vm.data(), px, py, m);
      };
      bool ok = zkr::r1cs_verify<F>(r->sh, r->digest, iom.data(), cf1.data(), ncoeffs1, cf2.data(), ncoeffs2, ev[0],
                                    ev[1], ev[2], ev[3], reinterpret_cast<const uint64_t*>(commitment), &tr,
                                    matrix_evals, rx, ry);
      if (ok && committed) {
        std::vector<zk_fe> pt(sy - 1);
        for (uint32_t k = 0; k + 1 < sy; ++k) pt[k] = to_zk(ry[k + 1]);
        const zk_fe vw = to_zk(ev[3]);
        int kz = 0;
        pass_on(zk_kzg_verify(ZK_REPR_MONTGOMERY, commitment, &vw, opening, sy - 1, pt.data(), sy - 1, g2_taus, &kz));
        ok = kz != 0;
      }
      *out_verified = ok ? 1 : 0;
      if (!ok) return;  // a rejection writes nothing else
      for (uint32_t k = 0; k < sx; ++k) out_rx[k] = out_repr<F>(repr, rx[k]);
      for (uint32_t k = 0; k < sy; ++k) out_ry[k] = out_repr<F>(repr, ry[k]);
      *transcript = tr;
    });
  });
}

}  // extern "C"
