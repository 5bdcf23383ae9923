// Radix-2 NTT over the scalar fields (fft/src/fft.rs) and the polynomial
// product built on it (univariate_polynomial_dense.rs impl Mul), C ABI: the
// roots and twiddle tables come from the host (hfield.hpp), every butterfly
// runs on the GPU (fft.hpp) as the passes fft_plan.hpp lays out.
#include "host.hpp"
#include "hfield.hpp"
#include "fft.hpp"

using namespace zkh;

namespace {
// F::TWO_ADICITY and F::TWO_ADIC_ROOT_OF_UNITY = g^((p - 1) / 2^s), canonical
// (ark-bn254 / ark-bls12-381 0.5.0: g = 5, 7; Fq has s = 1 and the root p - 1)
template <class F>
struct FftField;
template <>
struct FftField<zk::Bn254Fr> {
  static constexpr uint32_t S = 28;
  static constexpr uint64_t ROOT[4] = {0x9bd61b6e725b19f0ull, 0x402d111e41112ed4ull, 0x00e0a7eb8ef62abcull,
                                       0x2a3c09f0a58a7e85ull};
};
template <>
struct FftField<zk::Bn254Fq> {
  static constexpr uint32_t S = 1;
  static constexpr uint64_t ROOT[4] = {0x3c208c16d87cfd46ull, 0x97816a916871ca8dull, 0xb85045b68181585dull,
                                       0x30644e72e131a029ull};
};
template <>
struct FftField<zk::Bls12_381Fr> {
  static constexpr uint32_t S = 32;
  static constexpr uint64_t ROOT[4] = {0x3829971f439f0d2bull, 0xb63683508c2280b9ull, 0xd09b681922c813b4ull,
                                       0x16a2a19edfe81f20ull};
};

inline bool is_pow2(uint64_t n) { return n != 0 && (n & (n - 1)) == 0; }
inline uint32_t log2u(uint64_t n) { return 63u - (uint32_t)__builtin_clzll(n); }

// log2 n of a transform length the reference accepts (fft.rs :34-38) and this build runs
template <class F>
uint32_t transform_log(uint64_t n) {
  require(is_pow2(n), "Length must be a power of 2");
  const uint32_t m = log2u(n);
  require(m <= FftField<F>::S, "the field has no root of unity of this order (get_root_of_unity is None)");
  if (m > kFftMaxLog) fail(ZK_EUNSUPPORTED, "transforms above 2^28 elements are not supported");
  return m;
}

// ---- host field helpers (Montgomery images) ----
template <class F>
Fe h_pow(Fe x, uint64_t e) {
  Fe r = zk::fe_one<F>();
  for (; e; e >>= 1) {
    if (e & 1) r = zk::hfe_mul<F>(r, x);
    x = zk::hfe_mul<F>(x, x);
  }
  return r;
}
template <class F>
Fe h_root(uint32_t m) {  // F::get_root_of_unity(2^m), m <= S
  Fe c;
  memcpy(c.v, FftField<F>::ROOT, 32);
  Fe w = zk::hfe_to_mont<F>(c);
  for (uint32_t k = m; k < FftField<F>::S; ++k) w = zk::hfe_mul<F>(w, w);
  return w;
}
template <class F>
Fe h_inv_pow2(uint32_t m) {  // (2^m)^-1
  return h_pow<F>(zk::fe_inv2<F>(), m);
}
// dev[i] = first * step^i, i < count. The copy is the blocking hipMemcpy (null
// stream) although the kernels run on c->stream: it has finished for the host
// on return, and the host enqueues the first kernel that reads `dev` only after
// that; the table is new, so nothing in flight on c->stream touches it.
template <class F>
void fill_powers(DevBuf& dev, const Fe& first, const Fe& step, uint64_t count) {
  std::vector<Fe> v(count);
  Fe cur = first;
  for (uint64_t i = 0; i < count; ++i) {
    v[i] = cur;
    cur = zk::hfe_mul<F>(cur, step);
  }
  dev.ensure(count * sizeof(Fe));
  HIPCK(hipMemcpy(dev.p, v.data(), count * sizeof(Fe), hipMemcpyHostToDevice));
}

// The tables of a (field, log2 n, direction); the stage cap is fixed for the context's life.
// Built at the first transform of that shape and kept until zk_ctx_destroy,
// never evicted: a cost of zk_dev_fft the caller does not see, at most about
// 1.5 MB per shape (128 stage roots, Hi, Lo and the inverse's scaled Lo of <=
// 2^14 entries each) and 3 fields x 29 sizes x 2 directions shapes in all.
template <class F>
const FftTables& tables_for(zk_ctx* c, uint32_t m, bool inverse, const std::vector<FftPassPlan>& plan) {
  for (auto& t : c->fft_tables)
    if (t->field == F::id && t->m == m && t->inverse == inverse) return *t;
  auto t = std::make_unique<FftTables>();
  t->field = F::id;
  t->m = m;
  t->inverse = inverse;
  try {
    const uint64_t n = (uint64_t)1 << m;
    Fe w = h_root<F>(m);
    if (inverse) w = h_pow<F>(w, n - 1);  // w^-1
    t->n_inv = inverse ? h_inv_pow2<F>(m) : zk::fe_one<F>();
    for (auto& q : plan) t->log_w = std::max(t->log_w, q.a);
    // in-tile stage roots: w_(2^log_w)^i, i < 2^(log_w - 1)
    fill_powers<F>(t->stage_roots, zk::fe_one<F>(), h_pow<F>(w, n >> t->log_w), (uint64_t)1 << (t->log_w - 1));
    if (plan.size() > 1) {  // inter-pass twiddles: w^e = hi[e >> h] lo[e & (2^h - 1)], both <= 2^14 entries
      t->h = (m + 1) / 2;
      fill_powers<F>(t->lo, zk::fe_one<F>(), w, (uint64_t)1 << t->h);
      fill_powers<F>(t->hi, zk::fe_one<F>(), h_pow<F>(w, (uint64_t)1 << t->h), (uint64_t)1 << (m - t->h));
      if (inverse) fill_powers<F>(t->lo_scaled, t->n_inv, w, (uint64_t)1 << t->h);  // n^-1 rides on the last pass
    }
  } catch (...) {
    t->stage_roots.release();
    t->hi.release();
    t->lo.release();
    t->lo_scaled.release();
    throw;
  }
  c->fft_tables.push_back(std::move(t));
  return *c->fft_tables.back();
}

template <class K>
uint32_t fft_grid(zk_ctx* c, uint64_t blocks, K kernel) {
  uint32_t g = grid_for(c, blocks * zk::kBlock, kernel);
  if (c->grid_cap > 0 && g > c->grid_cap) g = c->grid_cap;
  return g;
}
#define FFT_LAUNCH(c, kernel, grid, ...)                                   \
  do {                                                                     \
    kernel<<<dim3(grid), dim3(zk::kBlock), 0, (c)->stream>>>(__VA_ARGS__); \
    HIPCK(hipGetLastError());                                              \
  } while (0)

// d_out = DFT of d_in (2^m Montgomery elements, natural order both sides) on
// the context's stream; d_out == d_in or disjoint. Not synchronised.
template <class F>
void run_fft(zk_ctx* c, const Fe* d_in, uint32_t m, bool inverse, Fe* d_out) {
  const uint64_t n = (uint64_t)1 << m;
  if (m == 0) {  // dft :9-11; n^-1 = 1
    if (d_out != d_in) HIPCK(hipMemcpyAsync(d_out, d_in, sizeof(Fe), hipMemcpyDeviceToDevice, c->stream));
    return;
  }
  const std::vector<FftPassPlan> plan = fft_plan(m, c->fft_stages);
  const FftTables& tb = tables_for<F>(c, m, inverse, plan);
  const size_t P = plan.size();
  // the chain in -> ... -> A -> out: the passes alternate between A and Y
  // (out itself when it is not the input, else a second scratch table)
  Fe *A = nullptr, *Y = d_out;
  if (P >= 2) {
    c->fft_scratch[0].ensure(n * sizeof(Fe));
    A = c->fft_scratch[0].fe();
  }
  if (P >= 3 && d_out == d_in) {
    c->fft_scratch[1].ensure(n * sizeof(Fe));
    Y = c->fft_scratch[1].fe();
  }
  const Fe* src = d_in;
  for (size_t p = 0; p < P; ++p) {
    const FftPassPlan& q = plan[p];
    Fe* dst = p + 1 == P ? d_out : ((P - 1 - p) % 2 == 0 ? Y : A);
    zk::FftPass fp;
    fp.n = n;
    fp.m = m;
    fp.a = q.a;
    fp.log_ns = q.log_ns;
    fp.log_c = q.log_c;
    fp.log_w = tb.log_w;
    fp.h = tb.h;
    fp.scale = inverse && P == 1;
    fp.stage_roots = tb.stage_roots.fe();
    fp.hi = tb.hi.fe();
    fp.lo = inverse && P > 1 && p + 1 == P ? tb.lo_scaled.fe() : tb.lo.fe();
    fp.n_inv = tb.n_inv;
    const uint64_t tiles = n >> (q.a + q.log_c);
    if (src == dst && tiles != 1) fail(ZK_EINVAL, "internal: an in-place pass of more than one tile");
    if (inverse) {
      const auto kern = zk::k_fft_pass<F, true>;
      FFT_LAUNCH(c, kern, fft_grid(c, tiles, kern), src, dst, fp);
    } else {
      const auto kern = zk::k_fft_pass<F, false>;
      FFT_LAUNCH(c, kern, fft_grid(c, tiles, kern), src, dst, fp);
    }
    src = dst;
  }
}

// fft_evaluate :31-41 / fft_interpolate :43-60 over host values
int host_transform(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* in, uint64_t n, zk_fe* out, bool inverse) {
  return guarded([&] {
    require(c && in && out, "null argument");
    check_repr(repr, "unknown representation");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const uint32_t m = transform_log<F>(n);
      bind(c);
      c->input.ensure(n * sizeof(Fe));
      upload<F>(c, repr, in, n, c->input.fe());
      run_fft<F>(c, c->input.fe(), m, inverse, c->input.fe());
      download<F>(c, repr, c->input.fe(), n, out);
    });
  });
}

bool fe_all_zero(const zk_fe& x) { return (x.limb[0] | x.limb[1] | x.limb[2] | x.limb[3]) == 0; }
}  // namespace

extern "C" {

int zk_fft_root_of_unity(zk_field field, zk_repr repr, uint64_t n, zk_fe* out) {
  return guarded([&] {
    require(out != nullptr, "null argument");
    check_repr(repr, "unknown representation");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      *out = out_repr<F>(repr, h_root<F>(transform_log<F>(n)));
    });
  });
}

int zk_fft_interpolation_roots(zk_field field, zk_repr repr, uint64_t n, zk_fe* out) {
  return guarded([&] {
    require(out != nullptr, "null argument");
    check_repr(repr, "unknown representation");
    require(n >= 1 && n <= ((uint64_t)1 << kFftMaxLog), "no evaluation domain of this size");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const uint32_t M = log2u(n) + (is_pow2(n) ? 0 : 1);  // GeneralEvaluationDomain::new rounds up
      require(M <= FftField<F>::S && M <= kFftMaxLog, "no evaluation domain of this size");
      const Fe w_inv = h_pow<F>(h_root<F>(M), ((uint64_t)1 << M) - 1);
      Fe cur = h_inv_pow2<F>(M);
      for (uint64_t k = 0; k < n; ++k) {  // :77
        out[k] = out_repr<F>(repr, cur);
        cur = zk::hfe_mul<F>(cur, w_inv);
      }
    });
  });
}

int zk_fft_evaluate(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* coeffs, uint64_t n, zk_fe* out) {
  return host_transform(c, field, repr, coeffs, n, out, false);
}

int zk_fft_interpolate(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* evals, uint64_t n, zk_fe* out) {
  return host_transform(c, field, repr, evals, n, out, true);
}

int zk_dev_fft(zk_ctx* c, zk_field field, const void* d_in, uint64_t n, int inverse, void* d_out) {
  return guarded([&] {
    require(c && d_in && d_out, "null argument");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const uint32_t m = transform_log<F>(n);
      const char *a = reinterpret_cast<const char*>(d_in), *b = reinterpret_cast<const char*>(d_out);
      require(a == b || a + n * sizeof(Fe) <= b || b + n * sizeof(Fe) <= a, "the output overlaps the input");
      bind(c);
      run_fft<F>(c, reinterpret_cast<const Fe*>(d_in), m, inverse != 0, reinterpret_cast<Fe*>(d_out));
      sync(c);
    });
  });
}

int zk_poly_mul(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* a, uint64_t na, const zk_fe* b, uint64_t nb,
                zk_fe* out, uint64_t cap, uint64_t* out_len) {
  return guarded([&] {
    require(c && a && b && out_len, "null argument");
    check_repr(repr, "unknown representation");
    if (na > ((uint64_t)1 << kFftMaxLog) || nb > ((uint64_t)1 << kFftMaxLog))
      fail(ZK_EUNSUPPORTED, "products above 2^28 terms are not supported");
    while (na > 0 && fe_all_zero(a[na - 1])) --na;  // degree() :28-32
    while (nb > 0 && fe_all_zero(b[nb - 1])) --nb;
    require(na > 0 && nb > 0, "attempt to subtract with overflow (the zero polynomial has no degree)");
    const uint64_t len = na + nb - 1;
    *out_len = len;
    require(cap >= len && out != nullptr, "the output buffer is shorter than the product");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const uint32_t M = log2u(len) + (is_pow2(len) ? 0 : 1);
      if (M > FftField<F>::S || M > kFftMaxLog)
        fail(ZK_EUNSUPPORTED, "the product is longer than the field's largest power-of-two domain (or 2^28)");
      const uint64_t N = (uint64_t)1 << M;
      bind(c);
      c->input.ensure(2 * N * sizeof(Fe));
      c->work[0].ensure(std::max(na, nb) * sizeof(Fe));
      Fe *X = c->input.fe(), *Y = c->input.fe(N), *stage = c->work[0].fe();
      upload<F>(c, repr, a, na, stage);
      FFT_LAUNCH(c, zk::k_fft_copy_pad, fft_grid(c, (N + zk::kBlock - 1) / zk::kBlock, zk::k_fft_copy_pad), stage, na, X, N);
      upload<F>(c, repr, b, nb, stage);  // (after the pad on the same stream)
      FFT_LAUNCH(c, zk::k_fft_copy_pad, fft_grid(c, (N + zk::kBlock - 1) / zk::kBlock, zk::k_fft_copy_pad), stage, nb, Y, N);
      run_fft<F>(c, X, M, false, X);
      run_fft<F>(c, Y, M, false, Y);
      FFT_LAUNCH(c, zk::k_fft_pointwise<F>, fft_grid(c, (N + zk::kBlock - 1) / zk::kBlock, zk::k_fft_pointwise<F>), X, Y, N);
      run_fft<F>(c, X, M, true, X);
      download<F>(c, repr, X, len, out);
    });
  });
}

}  // extern "C"
