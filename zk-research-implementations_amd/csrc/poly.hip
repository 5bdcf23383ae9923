// Univariate polynomials over arbitrary points
// (univariate_polynomial_dense.rs evaluate :20-26, interpolate :48-74; all of
// the shamir_secret_sharing crate is these two), C ABI: the launches
// poly_plan.hpp lays out over the kernels of poly.hpp, and below
// ZK_POLY_HOST_MAX the same arithmetic on the host (poly_host.hpp).
#include "host.hpp"
#include "hfield.hpp"
#include "poly.hpp"
#include "poly_host.hpp"

using namespace zkh;

namespace {
void check_field(zk_field field) {
  require(field == ZK_BN254_FR || field == ZK_BN254_FQ || field == ZK_BLS12_381_FR, "unknown field");
}
// the caps of one evaluation (poly_plan.hpp), before anything is read
void check_eval_size(uint64_t d, uint64_t m) {
  const uint64_t cap = (uint64_t)1 << kPolyTableMaxLog;
  if (d > cap || m > cap) fail(ZK_EUNSUPPORTED, "more than 2^28 coefficients or points are not supported");
  if (d != 0 && m > kPolyEvalMaxProducts / d)
    fail(ZK_EUNSUPPORTED, "npoints x ncoeffs above 2^40 is not supported in one call");
}

template <class K>
uint32_t poly_grid(zk_ctx* c, uint64_t lanes, K kernel) {
  uint32_t g = grid_for(c, lanes, kernel);
  if (c->grid_cap > 0 && g > c->grid_cap) g = c->grid_cap;
  return g;
}
#define POLY_LAUNCH(c, kernel, gx, gy, ...)                                     \
  do {                                                                          \
    kernel<<<dim3(gx, gy), dim3(zk::kBlock), 0, (c)->stream>>>(__VA_ARGS__);    \
    HIPCK(hipGetLastError());                                                   \
  } while (0)

// d_out[i] = sum_k d_coeffs[k] d_xs[i]^k on the context's stream (Montgomery
// tables; d_out may be d_xs). Not synchronised.
template <class F>
void run_eval(zk_ctx* c, const Fe* d_coeffs, uint64_t d, const Fe* d_xs, uint64_t m, Fe* d_out) {
  if (m == 0) return;
  const PolyEvalPlan pl = poly_eval_plan(m, d, (uint32_t)c->num_cus);
  const uint32_t gx = poly_grid(c, m, zk::k_poly_eval<F>);
  if (pl.chunks == 1) {
    POLY_LAUNCH(c, zk::k_poly_eval<F>, gx, 1, d_coeffs, d, d_xs, m, d_out, pl.chunk_len);
    return;
  }
  c->poly_scratch[2].ensure((size_t)pl.chunks * m * sizeof(Fe));
  Fe* cells = c->poly_scratch[2].fe();
  POLY_LAUNCH(c, zk::k_poly_eval<F>, gx, pl.chunks, d_coeffs, d, d_xs, m, cells, pl.chunk_len);
  POLY_LAUNCH(c, zk::k_poly_eval_combine<F>, poly_grid(c, m, zk::k_poly_eval_combine<F>), 1, cells, m, pl.chunks,
              pl.chunk_len, d_xs, d_out);
}

// The interpolant of (d_xs[i], d_ys[i]), i < n (n >= 1): its n coefficients,
// untrimmed, in a context scratch table (returned). Synchronises once, to
// read the duplicate flag before the tree.
template <class F>
const Fe* run_interpolate(zk_ctx* c, const Fe* d_xs, const Fe* d_ys, uint64_t n) {
  const PolyWeightsPlan wp = poly_weights_plan(n, (uint32_t)c->num_cus);
  for (int k = 0; k < 2; ++k) c->poly_scratch[k].ensure(2 * n * sizeof(Fe));
  uint32_t max_split = 1;
  for (const PolyLevel& lv : poly_tree_plan(n)) max_split = std::max(max_split, poly_tree_split(lv.log_len));
  // the weight parts, later the tree's partial sums (M and N per part)
  c->poly_scratch[2].ensure(std::max<size_t>(wp.parts, max_split > 1 ? 2 * (size_t)max_split : 0) * n * sizeof(Fe));
  Fe* parts = c->poly_scratch[2].fe();
  Fe *M = c->poly_scratch[0].fe(), *N = c->poly_scratch[0].fe(n);
  Fe *M2 = c->poly_scratch[1].fe(), *N2 = c->poly_scratch[1].fe(n);
  HIPCK(hipMemsetAsync(d_flag(c), 0, 4, c->stream));
  POLY_LAUNCH(c, zk::k_poly_weights<F>, poly_grid(c, n, zk::k_poly_weights<F>), wp.parts, d_xs, n, parts, wp.part_len);
  POLY_LAUNCH(c, zk::k_poly_leaves<F>, poly_grid(c, n, zk::k_poly_leaves<F>), 1, parts, wp.parts, d_xs, d_ys, n, M, N,
              d_flag(c));
  uint32_t dup = 0;
  HIPCK(hipMemcpyAsync(&dup, d_flag(c), 4, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  require(dup == 0, "attempt to divide by zero (two points with the same x)");  // :62-64
  for (const PolyLevel& lv : poly_tree_plan(n)) {
    const uint32_t S = poly_tree_split(lv.log_len);
    Fe *Mp = c->poly_scratch[2].fe(), *Np = c->poly_scratch[2].fe((size_t)S * n);
    POLY_LAUNCH(c, zk::k_poly_tree_level<F>, poly_grid(c, n, zk::k_poly_tree_level<F>), S, M, N, M2, N2, n, lv.log_len, Mp, Np);
    if (S > 1)
      POLY_LAUNCH(c, zk::k_poly_tree_combine<F>, poly_grid(c, n, zk::k_poly_tree_combine<F>), 1, M, N, Mp, Np, S, M2, N2, n,
                  lv.log_len);
    std::swap(M, M2);
    std::swap(N, N2);
  }
  return N;
}

bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const char *x = reinterpret_cast<const char*>(a), *y = reinterpret_cast<const char*>(b);
  return x < y + nb * sizeof(Fe) && y < x + na * sizeof(Fe);
}
}  // namespace

extern "C" {

int zk_poly_evaluate(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* coeffs, uint64_t ncoeffs, const zk_fe* xs,
                     uint64_t npoints, zk_fe* out) {
  return guarded([&] {
    require((coeffs || ncoeffs == 0) && (npoints == 0 || (xs && out)), "null argument");
    check_repr(repr, "unknown representation");
    check_field(field);
    check_eval_size(ncoeffs, npoints);
    require(c != nullptr, "null context");
    if (npoints == 0) return;
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      const uint64_t h = c->poly_host_max;
      if (h > 0 && (ncoeffs == 0 || npoints <= h * h / ncoeffs)) {  // (h <= 2^16)
        std::vector<Fe> cf(ncoeffs), x(npoints), y(npoints);
        for (uint64_t k = 0; k < ncoeffs; ++k) cf[k] = in_mont<F>(repr, coeffs[k]);
        for (uint64_t i = 0; i < npoints; ++i) x[i] = in_mont<F>(repr, xs[i]);
        host_poly_evaluate<F>(cf.data(), ncoeffs, x.data(), npoints, y.data());
        for (uint64_t i = 0; i < npoints; ++i) out[i] = out_repr<F>(repr, y[i]);
        return;
      }
      bind(c);
      c->input.ensure((ncoeffs + npoints) * sizeof(Fe));
      Fe *d_cf = c->input.fe(), *d_x = c->input.fe(ncoeffs);
      upload<F>(c, repr, coeffs, ncoeffs, d_cf);
      upload<F>(c, repr, xs, npoints, d_x);
      run_eval<F>(c, d_cf, ncoeffs, d_x, npoints, d_x);
      download<F>(c, repr, d_x, npoints, out);
    });
  });
}

int zk_dev_poly_evaluate(zk_ctx* c, zk_field field, const void* coeffs_tbl, uint64_t ncoeffs, const void* xs_tbl,
                         uint64_t npoints, void* out_tbl) {
  return guarded([&] {
    require((coeffs_tbl || ncoeffs == 0) && (npoints == 0 || (xs_tbl && out_tbl)), "null argument");
    check_field(field);
    check_eval_size(ncoeffs, npoints);
    require(c != nullptr, "null context");
    if (npoints == 0) return;
    require(ncoeffs == 0 || !overlap(coeffs_tbl, ncoeffs, out_tbl, npoints), "the output overlaps the coefficients");
    require(xs_tbl == out_tbl || !overlap(xs_tbl, npoints, out_tbl, npoints), "the output overlaps the points");
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      bind(c);
      run_eval<F>(c, reinterpret_cast<const Fe*>(coeffs_tbl), ncoeffs, reinterpret_cast<const Fe*>(xs_tbl), npoints,
                  reinterpret_cast<Fe*>(out_tbl));
      sync(c);
    });
  });
}

int zk_poly_eval_plan(const zk_ctx* c, uint64_t ncoeffs, uint64_t npoints, uint32_t* out_chunks, uint64_t* out_chunk_len) {
  return guarded([&] {
    require(c && out_chunks && out_chunk_len, "null argument");
    check_eval_size(ncoeffs, npoints);
    const PolyEvalPlan pl = poly_eval_plan(npoints, ncoeffs, (uint32_t)c->num_cus);
    *out_chunks = pl.chunks;
    *out_chunk_len = pl.chunk_len;
  });
}

int zk_poly_interpolate(zk_ctx* c, zk_field field, zk_repr repr, const zk_fe* xs, const zk_fe* ys, uint64_t n,
                        zk_fe* out_coeffs, uint64_t cap, uint64_t* out_ncoeffs) {
  return guarded([&] {
    require(out_ncoeffs != nullptr && (n == 0 || (xs && ys && out_coeffs)), "null argument");
    check_repr(repr, "unknown representation");
    check_field(field);
    if (n > kPolyInterpMax) fail(ZK_EUNSUPPORTED, "interpolation of more than 2^16 points is not supported");
    require(cap >= n, "the output buffer is shorter than the number of points");
    require(c != nullptr, "null context");
    if (n == 0) {
      *out_ncoeffs = 0;
      return;
    }
    dispatch(field, [&](auto f) {
      using F = decltype(f);
      std::vector<zk_fe> res(n);
      if (n <= c->poly_host_max) {
        std::vector<Fe> x(n), y(n), r(n);
        for (uint64_t i = 0; i < n; ++i) {
          x[i] = in_mont<F>(repr, xs[i]);
          y[i] = in_mont<F>(repr, ys[i]);
        }
        require(host_poly_interpolate<F>(x.data(), y.data(), n, r.data()),
                "attempt to divide by zero (two points with the same x)");  // :62-64
        for (uint64_t k = 0; k < n; ++k) res[k] = out_repr<F>(repr, r[k]);
      } else {
        bind(c);
        c->input.ensure(2 * n * sizeof(Fe));
        Fe *d_x = c->input.fe(), *d_y = c->input.fe(n);
        upload<F>(c, repr, xs, n, d_x);
        upload<F>(c, repr, ys, n, d_y);
        download<F>(c, repr, run_interpolate<F>(c, d_x, d_y, n), n, res.data());
      }
      uint64_t len = n;  // trim :14-18, :71 (0 is 0 in both representations)
      while (len > 0 && (res[len - 1].limb[0] | res[len - 1].limb[1] | res[len - 1].limb[2] | res[len - 1].limb[3]) == 0) --len;
      memcpy(out_coeffs, res.data(), len * sizeof(zk_fe));
      *out_ncoeffs = len;
    });
  });
}

}  // extern "C"
