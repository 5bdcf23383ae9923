// Sum-check over any sum of products of multilinear tables:
// host driver and C ABI. The plain loop: launch a round kernel (composed.hpp),
// wait for its sums through the pinned RoundSink flag, interpolate and run the
// transcript on the host (composed_plan.hpp), launch the next round with the
// challenge as an argument. Rounds whose tables have at most
// 2^ZK_COMPOSED_HOST_LG entries run on the host, on the same composed_plan.hpp
// code the CPU tests drive.
#include "host.hpp"
#include "composed.hpp"

using namespace zkh;

static_assert(ZK_COMPOSED_MAX_DEGREE == zkc::kComposedMaxDegree, "the header states the cap");

namespace {
constexpr auto plan_check = plan_check_with<zkc::C_OK, zkc::C_EUNSUPPORTED>;

struct Shape {
  uint32_t ntables, nvars, nterms, degree;
  const uint8_t* factors;
};

zk::ComposedArgs make_args(const Shape& sh) {
  zk::ComposedArgs a{};
  const zkc::ComposedMasks m = zkc::composed_masks(sh.ntables, sh.factors, sh.nterms, sh.degree);
  memcpy(a.factors, sh.factors, (size_t)sh.nterms * sh.degree);
  memcpy(a.store, m.store, sizeof a.store);
  memcpy(a.unused, m.unused, sizeof a.unused);
  a.nterms = sh.nterms;
  a.nunused = m.nunused;
  return a;
}

// The device rounds (tables of more than 2^host_lg entries), then the hand-over:
// the newest tables come to the host still unfolded by the last challenge, the
// host folds them and runs what is left (composed_host_rounds).
template <class F, int D>
void composed_prove_device(zk_ctx* c, const Fe* const* dT, const Shape& sh, zk_transcript* tr, zkc::ComposedOut& o) {
  using namespace zk;
  const uint32_t n = sh.nvars, nt = sh.ntables;
  zkc::composed_out_init(o, n, D, fe_zero<F>());
  ComposedArgs a = make_args(sh);
  for (uint32_t i = 0; i < nt; ++i) a.in[i] = dT[i];
  uint64_t size = (uint64_t)1 << n;  // entries per table of a.in
  uint32_t k = 0;
  Fe r = fe_zero<F>();
  if (n > c->composed_host_lg) {
    ensure_partials(c, n);
    __atomic_store_n(h_err(c), 0u, __ATOMIC_RELAXED);
    c->work[0].ensure((uint64_t)nt * (size / 2) * 32);
    if (n >= 2) c->work[1].ensure((uint64_t)nt * (size / 4) * 32);
  }
  int ob = 0;
  const double prods = (double)sh.nterms * (D + 1) * (D - 1);  // per pair
  for (; n - k > c->composed_host_lg; ++k) {
    const uint64_t h = (uint64_t)1 << (n - k - 1);
    const RoundSink sk = make_sink(c, false);
    if (k == 0) {
      const uint32_t grid = step_grid(c, grid_for(c, h, k_composed_round0<F, D>), 1);
      launch(c, ZK_K_GKR_ROUND0, 64.0 * nt * h, prods * h, k_composed_round0<F, D>, grid, a, h, sk);
    } else {
      Fe* w = c->work[ob].fe();
      for (uint32_t i = 0; i < nt; ++i) a.out[i] = w + (uint64_t)i * 2 * h;
      RoundIn rin{};
      rin.r = r;
      const uint32_t grid = step_grid(c, grid_for(c, h, k_composed_round<F, D>), 1);
      launch(c, ZK_K_GKR_ROUND, 192.0 * nt * h, (2.0 * nt + prods) * h, k_composed_round<F, D>, grid, a, h, rin, sk);
      for (uint32_t i = 0; i < nt; ++i) a.in[i] = a.out[i];
      size = 2 * h;
      ob ^= 1;
    }
    Fe y[D + 1];
    collect_sums<F, D + 1>(c, sk, false, 17, y);
    r = zkc::composed_finish_round<F>(tr, D, y, k, o);  // (round 0 folds nothing: the inputs wait for r_0)
  }
  // a.in: tables of `size` entries; after a device round they still want the fold by r
  std::vector<std::vector<Fe>> T(nt, std::vector<Fe>(size));
  for (uint32_t i = 0; i < nt; ++i)
    HIPCK(hipMemcpyAsync(T[i].data(), a.in[i], size * 32, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  if (k > 0) zkc::composed_host_fold<F>(T, r);
  zkc::composed_host_rounds<F>(T, sh.factors, sh.nterms, D, k, n, tr, o);
}

template <class F>
void composed_prove_any(zk_ctx* c, const Fe* const* dT, const Shape& sh, zk_transcript* tr, zkc::ComposedOut& o) {
  static_assert(zkc::kComposedMaxDegree == 4, "one instantiation per degree");
  switch (sh.degree) {
    case 1: composed_prove_device<F, 1>(c, dT, sh, tr, o); break;
    case 2: composed_prove_device<F, 2>(c, dT, sh, tr, o); break;
    case 3: composed_prove_device<F, 3>(c, dT, sh, tr, o); break;
    default: composed_prove_device<F, 4>(c, dT, sh, tr, o); break;
  }
}

template <class F>
void emit_composed(zk_repr repr, const zkc::ComposedOut& o, const Shape& sh, const Fe& cs, zk_fe* out_coeffs,
                   uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_table_evals, zk_fe* out_claimed_sum) {
  for (size_t i = 0; i < o.coeffs.size(); ++i) out_coeffs[i] = out_repr<F>(repr, o.coeffs[i]);
  for (uint32_t k = 0; k < sh.nvars; ++k) {
    out_ncoeffs[k] = o.ncoeffs[k];
    out_challenges[k] = out_repr<F>(repr, o.challenges[k]);
  }
  for (uint32_t i = 0; i < sh.ntables; ++i) out_table_evals[i] = out_repr<F>(repr, o.table_evals[i]);
  *out_claimed_sum = out_repr<F>(repr, cs);  // carried through (sum_check_protocol.rs:110-114)
}

void check_prove_args(const void* c, const void* const* tables, const Shape& sh, const void* claimed_sum,
                      const void* transcript, const void* out_coeffs, const void* out_ncoeffs,
                      const void* out_challenges, const void* out_table_evals, const void* out_claimed_sum) {
  require(c && tables && claimed_sum && transcript && out_table_evals && out_claimed_sum, "null argument");
  require(sh.nvars == 0 || (out_coeffs && out_ncoeffs && out_challenges), "null output");
  const char* err = nullptr;
  plan_check(zkc::composed_validate(sh.ntables, sh.nvars, sh.factors, sh.nterms, sh.degree, &err), err);
  for (uint32_t i = 0; i < sh.ntables; ++i) require(tables[i] != nullptr, "null table");
}
}  // namespace

extern "C" {

int zk_composed_sumcheck_prove(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* const* tables, uint32_t ntables,
                               uint32_t nvars, const uint8_t* factors, uint32_t nterms, uint32_t degree,
                               const zk_fe* claimed_sum, zk_transcript* transcript, zk_fe* out_coeffs,
                               uint8_t* out_ncoeffs, zk_fe* out_challenges, zk_fe* out_table_evals,
                               zk_fe* out_claimed_sum) {
  return guarded([&] {
    const Shape sh{ntables, nvars, nterms, degree, factors};
    check_prove_args(c, reinterpret_cast<const void* const*>(tables), sh, claimed_sum, transcript, out_coeffs,
                     out_ncoeffs, out_challenges, out_table_evals, out_claimed_sum);
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown repr");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const Fe cs = in_mont<F>(repr, *claimed_sum);
      bind(c);
      const uint64_t N = (uint64_t)1 << nvars;
      c->input.ensure((uint64_t)ntables * N * 32);
      const Fe* dT[zkc::kComposedMaxTables];
      for (uint32_t i = 0; i < ntables; ++i) {
        upload<F>(c, repr, tables[i], N, c->input.fe(i * N));
        dT[i] = c->input.fe(i * N);
      }
      zkc::ComposedOut o;
      composed_prove_any<F>(c, dT, sh, transcript, o);
      emit_composed<F>(repr, o, sh, cs, out_coeffs, out_ncoeffs, out_challenges, out_table_evals, out_claimed_sum);
    });
  });
}

int zk_dev_composed_sumcheck_prove(zk_ctx* c, zk_field field, zk_repr repr, const void* const* d_tables,
                                   uint32_t ntables, uint32_t nvars, const uint8_t* factors, uint32_t nterms,
                                   uint32_t degree, const zk_fe* claimed_sum, zk_transcript* transcript,
                                   zk_fe* out_coeffs, uint8_t* out_ncoeffs, zk_fe* out_challenges,
                                   zk_fe* out_table_evals, zk_fe* out_claimed_sum) {
  return guarded([&] {
    const Shape sh{ntables, nvars, nterms, degree, factors};
    check_prove_args(c, d_tables, sh, claimed_sum, transcript, out_coeffs, out_ncoeffs, out_challenges,
                     out_table_evals, out_claimed_sum);
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown repr");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const Fe cs = in_mont<F>(repr, *claimed_sum);
      bind(c);
      const Fe* dT[zkc::kComposedMaxTables];
      for (uint32_t i = 0; i < ntables; ++i) dT[i] = reinterpret_cast<const Fe*>(d_tables[i]);
      zkc::ComposedOut o;
      composed_prove_any<F>(c, dT, sh, transcript, o);
      emit_composed<F>(repr, o, sh, cs, out_coeffs, out_ncoeffs, out_challenges, out_table_evals, out_claimed_sum);
    });
  });
}

int zk_composed_sumcheck_verify(zk_field field, zk_repr repr, uint32_t degree, const zk_fe* coeffs,
                                const uint8_t* ncoeffs, uint32_t nrounds, const zk_fe* claimed_sum,
                                zk_transcript* transcript, int* out_verified, zk_fe* out_final_claim,
                                zk_fe* out_challenges) {
  return guarded([&] {
    require(claimed_sum && transcript && out_verified && out_final_claim && out_challenges, "null argument");
    require(nrounds == 0 || (coeffs && ncoeffs), "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown repr");
    require(degree >= 1, "degree must be at least 1");
    if (degree > zkc::kComposedMaxDegree) fail(ZK_EUNSUPPORTED, "degree above the cap (ZK_COMPOSED_MAX_DEGREE)");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const Fe claim = in_mont<F>(repr, *claimed_sum);
      std::vector<Fe> cf((size_t)(degree + 1) * nrounds, zk::fe_zero<F>());
      for (uint32_t k = 0; k < nrounds; ++k)
        for (uint32_t i = 0; i < std::min<uint32_t>(ncoeffs[k], degree + 1); ++i)
          cf[(size_t)(degree + 1) * k + i] = in_mont<F>(repr, coeffs[(size_t)(degree + 1) * k + i]);
      Fe fin;
      std::vector<Fe> chal;
      if (!zkc::composed_verify<F>(degree, cf.data(), ncoeffs, nrounds, claim, transcript, fin, chal)) {
        *out_verified = 0;
        *out_final_claim = out_repr<F>(repr, zk::fe_zero<F>());
        out_challenges[0] = out_repr<F>(repr, zk::fe_zero<F>());
        return;
      }
      for (uint32_t k = 0; k < nrounds; ++k) out_challenges[k] = out_repr<F>(repr, chal[k]);
      *out_verified = 1;
      *out_final_claim = out_repr<F>(repr, fin);
    });
  });
}

int zk_composed_combine(zk_field field, zk_repr repr, const zk_fe* table_evals, uint32_t ntables,
                        const uint8_t* factors, uint32_t nterms, uint32_t degree, zk_fe* out) {
  return guarded([&] {
    require(table_evals && out, "null argument");
    require(repr == ZK_REPR_CANONICAL || repr == ZK_REPR_MONTGOMERY, "unknown repr");
    const char* err = nullptr;
    plan_check(zkc::composed_validate(ntables, 0, factors, nterms, degree, &err), err);
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      Fe ev[zkc::kComposedMaxTables];
      for (uint32_t i = 0; i < ntables; ++i) ev[i] = in_mont<F>(repr, table_evals[i]);
      *out = out_repr<F>(repr, zkc::composed_combine<F>(ev, factors, nterms, degree));
    });
  });
}

}  // extern "C"
