// Sum-check over KZG-committed tables with one batched opening:
// host driver and C ABI. The prover is three calls on one transcript — the
// commitments absorbed, the composed sum-check (composed.hip, called, not
// copied), rho drawn after the tables' evaluations, one batched opening
// (kzg.hip) — in the order committed_plan.hpp fixes. Also the two table builders
// a zero-check needs in public: the linear combination (committed.hpp) and the
// eq table (host.hpp eq_table_device).
#include "host.hpp"
#include "committed.hpp"

using namespace zkh;

namespace {
using Fr381 = zk::Bls12_381Fr;
constexpr zk_field kField = ZK_BLS12_381_FR;  // all KZG here is over BLS12-381

constexpr auto plan_check = plan_check_with<zkc::C_OK, zkc::C_EUNSUPPORTED>;

struct ProveArgs {
  uint32_t ntables, nvars, nterms, degree, mask;
  const uint8_t* factors;
  const zk_g1* commitments_in;
  const zk_fe* claimed_sum;
  zk_transcript* transcript;
  zk_fe *out_coeffs, *out_claimed_sum, *out_challenges, *out_table_evals;
  uint8_t* out_ncoeffs;
  zk_g1 *out_commitments, *out_opening;
};

void check_prove_args(const zk_ctx* c, const zk_kzg* k, const void* const* tables, zk_repr repr, const ProveArgs& a) {
  require(c && k && tables && a.claimed_sum && a.transcript && a.out_coeffs && a.out_ncoeffs && a.out_challenges &&
              a.out_table_evals && a.out_claimed_sum && a.out_commitments && a.out_opening,
          "null argument");
  check_repr(repr);
  const char* err = nullptr;
  plan_check(zkc::composed_validate(a.ntables, a.nvars, a.factors, a.nterms, a.degree, &err), err);
  plan_check(zkc::committed_validate(a.ntables, a.nvars, kzg_nvars(k), a.mask, &err), err);
  for (uint32_t i = 0; i < a.ntables; ++i) require(tables[i] != nullptr, "null table");
  (void)in_mont<Fr381>(repr, *a.claimed_sum);  // < p
}

// The proof over Montgomery tables on the device. Everything is collected in
// locals, the transcript included, and handed out only once the opening has
// succeeded: nothing is written on failure.
void prove_device(zk_ctx* c, const zk_kzg* k, zk_repr repr, const void* const* dT, const ProveArgs& a) {
  const uint32_t nt = a.ntables, n = a.nvars, nc = zkc::mask_count(a.mask);
  const void* dC[zkc::kLincombMaxTables];
  zkc::committed_select(a.mask, nt, dT, dC);
  std::vector<zk_g1> cm(nc);
  if (a.commitments_in) {  // absorbed and returned as given (their encoding checked, not recomputed)
    for (uint32_t j = 0; j < nc; ++j) cm[j] = a.commitments_in[j];
    check_g1_points(cm.data(), nc);  // (what the verifier will require of them)
  } else {
    pass_on(zk_dev_kzg_commit_batch(c, k, dC, nc, cm.data()));
  }
  zk_transcript tr = *a.transcript;
  zkc::committed_absorb_commitments(&tr, reinterpret_cast<const uint64_t*>(cm.data()), nc);
  std::vector<zk_fe> coeffs((size_t)(a.degree + 1) * n), chal(n), ev(nt);
  std::vector<uint8_t> nco(n);
  zk_fe cs;
  pass_on(zk_dev_composed_sumcheck_prove(c, kField, repr, dT, nt, n, a.factors, a.nterms, a.degree, a.claimed_sum, &tr,
                                         coeffs.data(), nco.data(), chal.data(), ev.data(), &cs));
  Fe evm[zkc::kComposedMaxTables];
  for (uint32_t i = 0; i < nt; ++i) evm[i] = in_mont<Fr381>(repr, ev[i]);
  const zk_fe rho = out_repr<Fr381>(repr, zkc::committed_draw_rho<Fr381>(&tr, evm, nt));
  zk_fe evc[zkc::kLincombMaxTables];
  zkc::committed_select(a.mask, nt, ev.data(), evc);
  std::vector<zk_g1> opening(n);
  pass_on(zk_dev_kzg_batch_open(c, k, repr, dC, nc, &rho, evc, chal.data(), opening.data()));
  std::copy(coeffs.begin(), coeffs.end(), a.out_coeffs);
  std::copy(nco.begin(), nco.end(), a.out_ncoeffs);
  std::copy(chal.begin(), chal.end(), a.out_challenges);
  std::copy(ev.begin(), ev.end(), a.out_table_evals);
  *a.out_claimed_sum = cs;
  std::copy(cm.begin(), cm.end(), a.out_commitments);
  std::copy(opening.begin(), opening.end(), a.out_opening);
  *a.transcript = tr;
}
}  // namespace

extern "C" {

int zk_dev_mle_lincomb(zk_ctx* c, zk_field field, zk_repr repr, const void* const* d_tables, uint32_t ntables,
                       const zk_fe* coeffs, const zk_fe* constant, uint64_t count, void* d_out) {
  return guarded([&] {
    require(c && d_tables && coeffs && d_out, "null argument");
    require(ntables >= 1 && count >= 1, "ntables and count must be at least 1");
    if (ntables > zkc::kLincombMaxTables) fail(ZK_EUNSUPPORTED, "more than 16 tables");
    check_repr(repr);
    for (uint32_t i = 0; i < ntables; ++i) {
      require(d_tables[i] != nullptr, "null table");
      require(d_tables[i] != d_out, "d_out aliases an input table");
    }
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      Fe cf[zkc::kLincombMaxTables];
      for (uint32_t i = 0; i < ntables; ++i) cf[i] = in_mont<F>(repr, coeffs[i]);
      const Fe k0 = constant ? in_mont<F>(repr, *constant) : zk::fe_zero<F>();
      bind(c);
      launch_lincomb<F>(c, reinterpret_cast<const Fe* const*>(d_tables), ntables, cf, k0, count,
                        reinterpret_cast<Fe*>(d_out));
      sync(c);
    });
  });
}

int zk_dev_mle_eq_table(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* point, uint32_t n, void* d_out) {
  return guarded([&] {
    require(c && d_out && (point || n == 0), "null argument");
    if (n > zkc::kComposedMaxVars) fail(ZK_EUNSUPPORTED, "more than 26 variables");
    check_repr(repr);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      std::vector<Fe> pt(n);
      for (uint32_t i = 0; i < n; ++i) pt[i] = in_mont<F>(repr, point[i]);
      bind(c);
      const Fe one = zk::fe_one<F>();
      if (n == 0) {  // the empty product
        HIPCK(hipMemcpyAsync(d_out, &one, 32, hipMemcpyHostToDevice, c->stream));
      } else {
        c->work[1].ensure((((uint64_t)1 << n) / 4 + 8) * 32);
        eq_table_device<F>(c, pt.data(), n, reinterpret_cast<Fe*>(d_out), c->work[1].fe());
      }
      sync(c);
    });
  });
}

int zk_mle_eq_table(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* point, uint32_t n, zk_fe* out) {
  return guarded([&] {
    require(c && out && (point || n == 0), "null argument");
    if (n > zkc::kComposedMaxVars) fail(ZK_EUNSUPPORTED, "more than 26 variables");
    check_repr(repr);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      for (uint32_t i = 0; i < n; ++i) (void)in_mont<F>(repr, point[i]);
      bind(c);
      const uint64_t N = (uint64_t)1 << n;
      c->input.ensure(N * 32);
      pass_on(zk_dev_mle_eq_table(c, field, repr, point, n, c->input.p));
      download<F>(c, repr, c->input.fe(), N, out);
    });
  });
}

int zk_mle_eq_eval(zk_field field, zk_repr repr, const zk_fe* a, const zk_fe* b, uint32_t n, zk_fe* out) {
  return guarded([&] {
    require(out && ((a && b) || n == 0), "null argument");
    check_repr(repr);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      using namespace zk;
      Fe e = fe_one<F>();
      for (uint32_t i = 0; i < n; ++i) {  // a b + (1 - a)(1 - b) = 1 - a - b + 2 a b
        const Fe x = in_mont<F>(repr, a[i]), y = in_mont<F>(repr, b[i]), xy = hfe_mul<F>(x, y);
        const Fe t = hfe_add<F>(hfe_sub<F>(hfe_sub<F>(fe_one<F>(), x), y), hfe_add<F>(xy, xy));
        e = hfe_mul<F>(e, t);
      }
      *out = out_repr<F>(repr, e);
    });
  });
}

int zk_dev_committed_sumcheck_prove(zk_ctx* c, const zk_kzg* kzg, zk_repr repr, const void* const* d_tables,
                                    uint32_t ntables, uint32_t nvars, const uint8_t* factors, uint32_t nterms,
                                    uint32_t degree, uint32_t committed_mask, const zk_g1* commitments_in,
                                    const zk_fe* claimed_sum, zk_transcript* transcript, zk_fe* out_coeffs,
                                    uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_table_evals,
                                    zk_fe* out_claimed_sum, zk_g1* out_commitments, zk_g1* out_opening) {
  return guarded([&] {
    const ProveArgs a{ntables, nvars, nterms, degree, committed_mask, factors, commitments_in, claimed_sum, transcript,
                      out_coeffs, out_claimed_sum, out_challenges, out_table_evals, out_ncoeffs, out_commitments,
                      out_opening};
    check_prove_args(c, kzg, d_tables, repr, a);
    bind(c);
    prove_device(c, kzg, repr, d_tables, a);
  });
}

int zk_committed_sumcheck_prove(zk_ctx* c, const zk_kzg* kzg, zk_repr repr, const zk_fe* const* tables,
                                uint32_t ntables, uint32_t nvars, const uint8_t* factors, uint32_t nterms,
                                uint32_t degree, uint32_t committed_mask, const zk_g1* commitments_in,
                                const zk_fe* claimed_sum, zk_transcript* transcript, zk_fe* out_coeffs,
                                uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_table_evals,
                                zk_fe* out_claimed_sum, zk_g1* out_commitments, zk_g1* out_opening) {
  return guarded([&] {
    const ProveArgs a{ntables, nvars, nterms, degree, committed_mask, factors, commitments_in, claimed_sum, transcript,
                      out_coeffs, out_claimed_sum, out_challenges, out_table_evals, out_ncoeffs, out_commitments,
                      out_opening};
    check_prove_args(c, kzg, reinterpret_cast<const void* const*>(tables), repr, a);
    bind(c);
    // the tables go up once, into a buffer of their own (the commitments convert
    // through the context's staging area), and serve the sum-check and the opening
    const uint64_t N = (uint64_t)1 << nvars;
    ScopedBuf up;
    up.b.ensure((uint64_t)ntables * N * 32);
    const void* dT[zkc::kComposedMaxTables];
    for (uint32_t i = 0; i < ntables; ++i) {
      upload<Fr381>(c, repr, tables[i], N, up.b.fe(i * N));
      dT[i] = up.b.fe(i * N);
    }
    prove_device(c, kzg, repr, dT, a);
    sync(c);  // (nothing of the stream still reads `up`)
  });
}

int zk_committed_sumcheck_verify(zk_repr repr, uint32_t degree, const zk_fe* coeffs, const uint8_t* ncoeffs,
                                 uint32_t nrounds, const zk_fe* claimed_sum, const uint8_t* factors, uint32_t nterms,
                                 uint32_t ntables, const zk_fe* table_evals, uint32_t committed_mask,
                                 const zk_g1* commitments, const zk_g1* opening, const zk_g2* g2_taus,
                                 zk_transcript* transcript, int* out_verified, zk_fe* out_challenges) {
  return guarded([&] {
    require(coeffs && ncoeffs && claimed_sum && table_evals && commitments && opening && g2_taus && transcript &&
                out_verified && out_challenges,
            "null argument");
    check_repr(repr);
    const char* err = nullptr;
    plan_check(zkc::composed_validate(ntables, nrounds, factors, nterms, degree, &err), err);
    plan_check(zkc::committed_validate(ntables, nrounds, nrounds, committed_mask, &err), err);
    require(nrounds >= 1, "KZG needs at least one variable");
    const uint32_t nc = zkc::mask_count(committed_mask);
    Fe evm[zkc::kComposedMaxTables];
    for (uint32_t i = 0; i < ntables; ++i) evm[i] = in_mont<Fr381>(repr, table_evals[i]);
    check_g1_points(commitments, nc);  // canonical coordinates, on the curve; (0, 0) is infinity (an all-zero table)
    check_g1_points(opening, nrounds);
    zk_transcript tr = *transcript;
    zkc::committed_absorb_commitments(&tr, reinterpret_cast<const uint64_t*>(commitments), nc);
    int ok = 0;
    zk_fe fin;
    std::vector<zk_fe> chal(nrounds);
    pass_on(zk_composed_sumcheck_verify(kField, repr, degree, coeffs, ncoeffs, nrounds, claimed_sum, &tr, &ok, &fin,
                                        chal.data()));
    if (ok) {
      const Fe want = zkc::composed_combine<Fr381>(evm, factors, nterms, degree);
      ok = zk::fe_eq<Fr381>(in_mont<Fr381>(repr, fin), want) ? 1 : 0;
    }
    if (ok) {
      const zk_fe rho = out_repr<Fr381>(repr, zkc::committed_draw_rho<Fr381>(&tr, evm, ntables));
      zk_fe evc[zkc::kLincombMaxTables];
      zkc::committed_select(committed_mask, ntables, table_evals, evc);
      pass_on(zk_kzg_batch_verify(repr, commitments, nc, &rho, evc, opening, nrounds, chal.data(), nrounds, g2_taus,
                                  &ok));
    }
    *transcript = tr;
    *out_verified = ok;
    if (ok) {
      std::copy(chal.begin(), chal.end(), out_challenges);
    } else {  // as zk_composed_sumcheck_verify reports a failed round: one zero challenge
      out_challenges[0] = out_repr<Fr381>(repr, zk::fe_zero<Fr381>());
    }
  });
}

}  // extern "C"
