// Lookups (LogUp) over committed columns: host driver and C ABI.
// The prover is calls on one transcript, in the order lookup_plan.hpp fixes:
// the multiplicity count and the batched inversion (lookup.hpp) build m, h_f
// and h_t, KZG (kzg.hip) commits the four columns, and the committed sum-check
// (committed.hip, called, not copied) proves the three identities at once and
// opens the four columns at one point.
#include "host.hpp"
#include "lookup.hpp"

using namespace zkh;

struct zk_lookup {
  zk_ctx* c = nullptr;  // null: host-only
  int device = -1;      // c's device, kept so that freeing the handle never reads the context
  zk_field field = ZK_BN254_FR;
  uint32_t T = 0, slot_log = 0;
  std::vector<Fe> tm;           // the table, Montgomery
  std::vector<uint32_t> slots;  // 2^slot_log: the first index of a value, or kLookupEmpty
  uint8_t digest[32] = {0};
  DevBuf d_tm, d_slots, d_counts;  // d_counts: T counters, then the missing counter
  DevBuf tabs;                     // proof-time tables, sized at first use
};

namespace {
using Fr381 = zk::Bls12_381Fr;

constexpr auto plan_check = plan_check_with<zkl::L_OK, zkl::L_EUNSUPPORTED>;

void lookup_release(zk_lookup* lk) {
  for (DevBuf* b : {&lk->d_tm, &lk->d_slots, &lk->d_counts, &lk->tabs}) b->release();
  delete lk;
}

// counts zeroed, one probe per entry, the counters written out as elements
// over all 2^n slots; returns the number of entries found nowhere
template <class F>
uint64_t multiplicities_device(zk_lookup* lk, const Fe* d_f, uint64_t count, Fe* d_m, uint32_t n) {
  zk_ctx* c = lk->c;
  const uint64_t N = (uint64_t)1 << n;
  uint32_t* counts = reinterpret_cast<uint32_t*>(lk->d_counts.p);
  HIPCK(hipMemsetAsync(counts, 0, ((size_t)lk->T + 1) * 4, c->stream));
  launch(c, ZK_K_LAYER, 72.0 * count, (double)count, zk::k_lookup_probe<F>, grid_for(c, count, zk::k_lookup_probe<F>),
         d_f, count, (const Fe*)lk->d_tm.fe(), reinterpret_cast<const uint32_t*>(lk->d_slots.p), lk->slot_log, counts,
         counts + lk->T);
  launch(c, ZK_K_LAYER, 36.0 * N, (double)lk->T, zk::k_lookup_counts_to_fe<F>,
         grid_for(c, N, zk::k_lookup_counts_to_fe<F>), (const uint32_t*)counts, lk->T, d_m, N);
  uint32_t missing = 0;
  HIPCK(hipMemcpyAsync(&missing, counts + lk->T, 4, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  return missing;
}

struct ProveArgs {
  uint32_t n;
  const zk_kzg* kzg;
  const zk_g1* commitment_in;
  zk_transcript* transcript;
  zk_fe *out_coeffs, *out_table_evals, *out_point;
  uint8_t* out_ncoeffs;
  zk_g1 *out_commitments, *out_opening;
  uint64_t* out_missing;
};

void check_prove_args(const zk_lookup* lk, zk_repr repr, const void* f, const ProveArgs& a) {
  require(lk && f && a.kzg && a.transcript && a.out_coeffs && a.out_ncoeffs && a.out_table_evals && a.out_point &&
              a.out_commitments && a.out_opening && a.out_missing,
          "null argument");
  check_repr(repr);
  require(lk->field == ZK_BLS12_381_FR, "lookups are proved over BLS12-381 Fr");
  const char* err = nullptr;
  plan_check(zkl::lookup_validate_vars(lk->T, a.n, &err), err);
  if (!lk->c) fail(ZK_EDEVICE, "a host-only lookup handle cannot prove");  // (before the setup is read)
  require(kzg_nvars(a.kzg) == a.n, "the KZG setup must have n variables");
}

// The proof over a Montgomery column on the device. Everything is collected in
// locals, the transcript included, and handed out only at the end: nothing is
// written on failure.
void prove_device(zk_lookup* lk, zk_repr repr, const Fe* d_f, const ProveArgs& a) {
  using F = Fr381;
  using namespace zk;
  zk_ctx* c = lk->c;
  const uint32_t n = a.n;
  const uint64_t N = (uint64_t)1 << n;
  lk->tabs.ensure((uint64_t)zkl::kLookupTables * N * 32);
  auto tab = [&](uint32_t i) { return lk->tabs.fe((uint64_t)i * N); };
  const void* dT[zkl::kLookupTables];
  for (uint32_t i = 0; i < zkl::kLookupTables; ++i) dT[i] = tab(i);
  dT[zkl::LK_F] = d_f;  // (read in place)
  const zk_field fld = ZK_BLS12_381_FR;
  const Fe zero = fe_zero<F>(), one = fe_one<F>(), neg1 = hfe_sub<F>(zero, one);
  const zk_fe zzero = to_zk(zero), zone = to_zk(one), zneg1 = to_zk(neg1);

  // m, and the commitments of f and m
  const uint64_t missing = multiplicities_device<F>(lk, d_f, N, tab(zkl::LK_M), n);
  zk_g1 cm[4];  // table order: h_f, h_t, f, m
  if (a.commitment_in) {  // absorbed and returned as given (its encoding checked, not recomputed)
    cm[zkl::LK_F] = *a.commitment_in;
    check_g1_points(&cm[zkl::LK_F], 1);
    pass_on(zk_dev_kzg_commit_batch(c, a.kzg, &dT[zkl::LK_M], 1, &cm[zkl::LK_M]));
  } else {
    pass_on(zk_dev_kzg_commit_batch(c, a.kzg, &dT[zkl::LK_F], 2, &cm[zkl::LK_F]));
  }
  zk_transcript tr = *a.transcript;
  zkl::LookupChallenges ch;
  ch.alpha = zkl::lookup_begin<F>(&tr, lk->digest, n, reinterpret_cast<const uint64_t*>(&cm[zkl::LK_F]));

  // h_f = 1 / (alpha - f), h_t = m / (alpha - t_pad); table 10 holds alpha - . meanwhile
  launch(c, ZK_K_LAYER, 64.0 * N, 0.0, k_lookup_pad, grid_for(c, N, k_lookup_pad), (const Fe*)lk->d_tm.fe(), lk->T,
         tab(zkl::LK_TPAD), N);
  const zk_fe zalpha = to_zk(ch.alpha);
  Fe* tmp = tab(10);
  pass_on(zk_dev_mle_lincomb(c, fld, ZK_REPR_MONTGOMERY, &dT[zkl::LK_F], 1, &zneg1, &zalpha, N, tmp));
  launch_batch_inverse<F>(c, tmp, tab(zkl::LK_HF), tab(zkl::LK_HF), N);
  pass_on(zk_dev_mle_lincomb(c, fld, ZK_REPR_MONTGOMERY, &dT[zkl::LK_TPAD], 1, &zneg1, &zalpha, N, tmp));
  launch_batch_inverse<F>(c, tmp, tab(zkl::LK_HT), tab(zkl::LK_HT), N);
  launch(c, ZK_K_LAYER, 96.0 * N, (double)N, k_lookup_mul<F>, grid_for(c, N, k_lookup_mul<F>),
         (const Fe*)tab(zkl::LK_HT), (const Fe*)tab(zkl::LK_M), tab(zkl::LK_HT), N);
  sync(c);
  pass_on(zk_dev_kzg_commit_batch(c, a.kzg, &dT[zkl::LK_HF], 2, &cm[zkl::LK_HF]));
  zkl::lookup_draw<F>(&tr, n, reinterpret_cast<const uint64_t*>(&cm[zkl::LK_HF]), ch);

  // the public tables: eq(tau, .) into table 5 first, its four multiples, then the constants
  {
    std::vector<zk_fe> tau(n);
    for (uint32_t k = 0; k < n; ++k) tau[k] = to_zk(ch.tau[k]);
    Fe* eq = tab(zkl::LK_ONE);
    const void* eq_src[1] = {eq};
    pass_on(zk_dev_mle_eq_table(c, fld, ZK_REPR_MONTGOMERY, tau.data(), n, eq));
    Fe w[4];
    zkl::lookup_eq_scalars<F>(ch.alpha, ch.lambda, w);
    for (int i = 0; i < 4; ++i) {
      const zk_fe wi = to_zk(w[i]);
      pass_on(zk_dev_mle_lincomb(c, fld, ZK_REPR_MONTGOMERY, eq_src, 1, &wi, nullptr, N, tab(zkl::LK_E0 + i)));
    }
    pass_on(zk_dev_mle_lincomb(c, fld, ZK_REPR_MONTGOMERY, &dT[zkl::LK_F], 1, &zzero, &zone, N, tab(zkl::LK_ONE)));
    pass_on(zk_dev_mle_lincomb(c, fld, ZK_REPR_MONTGOMERY, &dT[zkl::LK_F], 1, &zzero, &zneg1, N, tab(zkl::LK_NEG)));
  }

  std::vector<zk_fe> coeffs((size_t)4 * n), point(n);
  std::vector<uint8_t> nco(n);
  std::vector<zk_g1> opening(n);
  zk_fe ev[zkl::kLookupTables], cs;
  zk_g1 cm_out[4];
  pass_on(zk_dev_committed_sumcheck_prove(c, a.kzg, repr, dT, zkl::kLookupTables, n, zkl::kLookupFactors,
                                          zkl::kLookupTerms, zkl::kLookupDegree, zkl::kLookupMask, cm,
                                          &zzero, &tr, coeffs.data(), nco.data(),
                                          point.data(), ev, &cs, cm_out, opening.data()));

  std::copy(coeffs.begin(), coeffs.end(), a.out_coeffs);
  std::copy(nco.begin(), nco.end(), a.out_ncoeffs);
  std::copy(ev, ev + zkl::kLookupTables, a.out_table_evals);
  std::copy(point.begin(), point.end(), a.out_point);
  std::copy(cm_out, cm_out + 4, a.out_commitments);
  std::copy(opening.begin(), opening.end(), a.out_opening);
  *a.out_missing = missing;
  *a.transcript = tr;
}
}  // namespace

extern "C" {

int zk_fe_batch_inverse(zk_field field, zk_repr repr, const zk_fe* in, uint64_t count, zk_fe* out) {
  return guarded([&] {
    require(in && out, "null argument");
    require(count >= 1, "count must be at least 1");
    check_repr(repr);
    require(in == out || !overlap(in, out, count * 32), "out overlaps in partly");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      std::vector<Fe> v(count);
      for (uint64_t i = 0; i < count; ++i) v[i] = in_mont<F>(repr, in[i]);
      zkl::host_batch_inverse<F>(v.data(), count, v.data());
      for (uint64_t i = 0; i < count; ++i) out[i] = out_repr<F>(repr, v[i]);
    });
  });
}

int zk_dev_fe_batch_inverse(zk_ctx* c, zk_field field, const void* d_in, uint64_t count, void* d_out) {
  return guarded([&] {
    require(c && d_in && d_out, "null argument");
    require(count >= 1, "count must be at least 1");
    if (count > ((uint64_t)1 << 32)) fail(ZK_EUNSUPPORTED, "more than 2^32 elements");
    require(d_in == d_out || !overlap(d_in, d_out, count * 32), "d_out overlaps d_in partly");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      bind(c);
      ScopedBuf pre;  // in place: the running products need a table of their own
      Fe* out = reinterpret_cast<Fe*>(d_out);
      if (d_in == d_out) pre.b.ensure(count * 32);
      launch_batch_inverse<F>(c, reinterpret_cast<const Fe*>(d_in), d_in == d_out ? pre.b.fe() : out, out, count);
      sync(c);
    });
  });
}

int zk_lookup_new(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* table, uint32_t T, zk_lookup** out) {
  return guarded([&] {
    require(out != nullptr, "null argument");
    check_repr(repr);
    const char* err = nullptr;
    plan_check(zkl::lookup_validate_table((uint32_t)field, table, T, &err), err);
    std::unique_ptr<zk_lookup> h(new zk_lookup());
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      plan_check(zkl::lookup_entries<F>(reinterpret_cast<const uint64_t*>(table), T, repr == ZK_REPR_MONTGOMERY, h->tm,
                                        &err),
                 err);
      h->slots = zkl::lookup_build_slots<F>(h->tm.data(), T);
      zkl::lookup_digest<F>((uint32_t)field, h->tm.data(), T, h->digest);
    });
    h->c = c;
    h->device = c ? c->device : -1;
    h->field = field;
    h->T = T;
    h->slot_log = zkl::lookup_slot_log(T);
    zk_lookup* lk = h.release();
    if (c) {
      try {
        bind(c);
        lk->d_tm.ensure((size_t)T * 32);
        lk->d_slots.ensure(lk->slots.size() * 4);
        lk->d_counts.ensure(((size_t)T + 1) * 4);
        HIPCK(hipMemcpy(lk->d_tm.p, lk->tm.data(), (size_t)T * 32, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(lk->d_slots.p, lk->slots.data(), lk->slots.size() * 4, hipMemcpyHostToDevice));
      } catch (...) {
        lookup_release(lk);
        throw;
      }
    }
    *out = lk;
  });
}

void zk_lookup_free(zk_lookup* lk) {
  if (!lk) return;
  if (lk->device >= 0) {  // (the context may be gone already: only the device is named)
    (void)hipSetDevice(lk->device);
    (void)hipDeviceSynchronize();
  }
  lookup_release(lk);
}

int zk_lookup_info(const zk_lookup* lk, uint32_t* out_T, uint32_t* out_nslots, uint8_t out_digest[32],
                   uint32_t* out_slots) {
  return guarded([&] {
    require(lk != nullptr, "null argument");
    if (out_T) *out_T = lk->T;
    if (out_nslots) *out_nslots = (uint32_t)lk->slots.size();
    if (out_digest) memcpy(out_digest, lk->digest, 32);
    if (out_slots) std::copy(lk->slots.begin(), lk->slots.end(), out_slots);
  });
}

int zk_lookup_multiplicities(zk_lookup* lk, zk_repr repr, const zk_fe* f, uint64_t count, uint32_t n, zk_fe* out_m,
                             uint64_t* out_missing) {
  return guarded([&] {
    require(lk && f && out_m && out_missing, "null argument");
    check_repr(repr);
    const char* err = nullptr;
    plan_check(zkl::lookup_validate_count(lk->T, count, n, &err), err);
    dispatch(lk->field, [&](auto ff) {
      using F = decltype(ff);
      const uint64_t N = (uint64_t)1 << n;
      if (!lk->c) {  // host-only handle: one probe per entry on the host
        std::vector<Fe> fm(count);
        for (uint64_t i = 0; i < count; ++i) fm[i] = in_mont<F>(repr, f[i]);
        std::vector<uint32_t> counts;
        const uint64_t missing = zkl::lookup_host_counts<F>(lk->tm.data(), lk->T, lk->slots.data(), fm.data(), count, counts);
        for (uint64_t j = 0; j < N; ++j)
          out_m[j] = out_repr<F>(repr, j < lk->T ? zkc::fe_small<F>(counts[j]) : zk::fe_zero<F>());
        *out_missing = missing;
        return;
      }
      for (uint64_t i = 0; i < count; ++i) (void)in_mont<F>(repr, f[i]);  // < p, before anything is written
      bind(lk->c);
      ScopedBuf buf;
      buf.b.ensure((count + N) * 32);
      upload<F>(lk->c, repr, f, count, buf.b.fe());
      const uint64_t missing = multiplicities_device<F>(lk, buf.b.fe(), count, buf.b.fe(count), n);
      std::vector<zk_fe> tmp(N);
      download<F>(lk->c, repr, buf.b.fe(count), N, tmp.data());
      std::copy(tmp.begin(), tmp.end(), out_m);
      *out_missing = missing;
    });
  });
}

int zk_dev_lookup_multiplicities(zk_lookup* lk, const void* d_f, uint64_t count, void* d_m, uint32_t n,
                                 uint64_t* out_missing) {
  return guarded([&] {
    require(lk && d_f && d_m && out_missing, "null argument");
    const char* err = nullptr;
    plan_check(zkl::lookup_validate_count(lk->T, count, n, &err), err);
    if (!lk->c) fail(ZK_EDEVICE, "a host-only lookup handle has no device");
    require(!overlap(d_f, d_m, std::min<uint64_t>(count, (uint64_t)1 << n) * 32), "d_m overlaps d_f");
    dispatch(lk->field, [&](auto ff) {
      using F = decltype(ff);
      bind(lk->c);
      *out_missing =
          multiplicities_device<F>(lk, reinterpret_cast<const Fe*>(d_f), count, reinterpret_cast<Fe*>(d_m), n);
    });
  });
}

int zk_lookup_table_eval(zk_lookup* lk, zk_repr repr, const zk_fe* point, uint32_t n, zk_fe* out) {
  return guarded([&] {
    require(lk && point && out, "null argument");
    check_repr(repr);
    const char* err = nullptr;
    plan_check(zkl::lookup_validate_vars(lk->T, n, &err), err);
    dispatch(lk->field, [&](auto ff) {
      using F = decltype(ff);
      std::vector<Fe> pt(n);
      for (uint32_t k = 0; k < n; ++k) pt[k] = in_mont<F>(repr, point[k]);
      *out = out_repr<F>(repr, zkl::lookup_table_eval<F>(lk->tm.data(), lk->T, pt.data(), n));
    });
  });
}

int zk_dev_lookup_prove(zk_lookup* lk, zk_repr repr, const void* d_f, uint32_t n, const zk_kzg* kzg,
                        const zk_g1* commitment_in, zk_transcript* transcript, zk_fe* out_coeffs, uint8_t* out_ncoeffs,
                        zk_fe* out_table_evals, zk_fe* out_point, zk_g1* out_commitments, zk_g1* out_opening,
                        uint64_t* out_missing) {
  return guarded([&] {
    const ProveArgs a{n, kzg, commitment_in, transcript, out_coeffs, out_table_evals, out_point, out_ncoeffs,
                      out_commitments, out_opening, out_missing};
    check_prove_args(lk, repr, d_f, a);
    bind(lk->c);
    prove_device(lk, repr, reinterpret_cast<const Fe*>(d_f), a);
  });
}

int zk_lookup_prove(zk_lookup* lk, zk_repr repr, const zk_fe* f, uint32_t n, const zk_kzg* kzg,
                    const zk_g1* commitment_in, zk_transcript* transcript, zk_fe* out_coeffs, uint8_t* out_ncoeffs,
                    zk_fe* out_table_evals, zk_fe* out_point, zk_g1* out_commitments, zk_g1* out_opening,
                    uint64_t* out_missing) {
  return guarded([&] {
    const ProveArgs a{n, kzg, commitment_in, transcript, out_coeffs, out_table_evals, out_point, out_ncoeffs,
                      out_commitments, out_opening, out_missing};
    check_prove_args(lk, repr, f, a);
    bind(lk->c);
    const uint64_t N = (uint64_t)1 << n;
    ScopedBuf up;  // the column goes up once, for the count, the commitment, the sum-check and the opening
    up.b.ensure(N * 32);
    upload<Fr381>(lk->c, repr, f, N, up.b.fe());
    prove_device(lk, repr, up.b.fe(), a);
    sync(lk->c);  // (nothing of the stream still reads `up`)
  });
}

int zk_lookup_verify(zk_lookup* lk, zk_repr repr, uint32_t n, const zk_fe* coeffs, const uint8_t* ncoeffs,
                     const zk_fe* table_evals, const zk_g1* commitments, const zk_g1* opening, const zk_g2* g2_taus,
                     zk_transcript* transcript, int* out_verified, zk_fe* out_point) {
  return guarded([&] {
    using F = Fr381;
    require(lk && coeffs && ncoeffs && table_evals && commitments && opening && g2_taus && transcript && out_verified &&
                out_point,
            "null argument");
    check_repr(repr);
    require(lk->field == ZK_BLS12_381_FR, "lookups are proved over BLS12-381 Fr");
    const char* err = nullptr;
    plan_check(zkl::lookup_validate_vars(lk->T, n, &err), err);
    check_g1_points(commitments, 4);
    check_g1_points(opening, n);
    Fe ev[zkl::kLookupTables];
    for (uint32_t i = 0; i < zkl::kLookupTables; ++i) ev[i] = in_mont<F>(repr, table_evals[i]);
    for (uint32_t k = 0; k < n; ++k)
      for (uint32_t i = 0; i < std::min<uint32_t>(ncoeffs[k], 4); ++i) (void)in_mont<F>(repr, coeffs[4 * k + i]);
    zk_transcript tr = *transcript;
    zkl::LookupChallenges ch;
    const uint64_t* cmw = reinterpret_cast<const uint64_t*>(commitments);
    ch.alpha = zkl::lookup_begin<F>(&tr, lk->digest, n, cmw + 12 * zkl::LK_F);
    zkl::lookup_draw<F>(&tr, n, cmw + 12 * zkl::LK_HF, ch);
    const zk_fe zzero = to_zk(zk::fe_zero<F>());
    std::vector<zk_fe> point(n);
    int ok = 0;
    pass_on(zk_committed_sumcheck_verify(repr, zkl::kLookupDegree, coeffs, ncoeffs, n, &zzero, zkl::kLookupFactors,
                                         zkl::kLookupTerms, zkl::kLookupTables, table_evals, zkl::kLookupMask,
                                         commitments, opening, g2_taus, &tr, &ok, point.data()));
    if (ok) {
      std::vector<Fe> r(n);
      for (uint32_t k = 0; k < n; ++k) r[k] = in_mont<F>(repr, point[k]);
      const Fe tp = zkl::lookup_table_eval<F>(lk->tm.data(), lk->T, r.data(), n);
      ok = zkl::lookup_public_ok<F>(ch, r.data(), n, ev, tp) ? 1 : 0;
    }
    *out_verified = ok;
    if (!ok) return;  // a rejection writes nothing else
    std::copy(point.begin(), point.end(), out_point);
    *transcript = tr;
  });
}

}  // extern "C"
