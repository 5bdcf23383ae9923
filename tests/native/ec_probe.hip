// Test-only probe of csrc/ec.hpp (built by `make probe` into
// zk_amd/_lib/libzkecprobe.so; not part of the product ABI): one ec.hpp
// function applied per element to arrays of raw Montgomery words, 12 x u32 per
// Fq, with no conversion on the way in or out.
//
// Every op has two legs. device = 0: a plain host loop, no HIP call (the host
// compilation of ec.hpp: fq_mul is fqh::mul, 6 x 64-bit). device = 1: one
// thread per element on the current device, with its own hipMalloc and copies
// (the device compilation: the 12 x 32-bit CIOS). Return codes: 0 ok, 1 unknown
// op, 2 null argument, 1000 + hipError_t for a HIP error. Nothing aborts.
//
// Element layouts (u32 words): Fq 12; G1A 24 (x, y); G1J 36 (X, Y, Z);
// G1XYZZ 48 (X, Y, ZZ, ZZZ). tests/ec_cases.py holds the op numbers and
// strides; zk_ecprobe_g1_shape reports the strides so it can check them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ec.hpp"

using namespace zk;

namespace {
constexpr int kThreads = 256;

enum FqOp { FQ_ADD, FQ_SUB, FQ_NEG, FQ_DBL, FQ_MUL, FQ_SQR, FQ_TO_MONT, FQ_FROM_MONT, FQ_INV, FQ_REDUCE_ONCE,
            FQ_IS_CANONICAL, FQ_NOPS };
enum G1Op { G1_DBL, G1_ADD, G1_ADD_MIXED, G1X_DBL, G1X_ADD, G1X_ADD_MIXED, G1X_TO_JAC, G1_TO_AFFINE, G1_TO_AFFINE_ZI,
            G1_MUL_SMALL, G1_FROM_AFFINE, G1_NOPS };

// words per element of (a, b, out); b = 0: no second operand
struct Shape {
  uint32_t a, b, out;
};
ZK_HD Shape g1_shape(int op) {
  switch (op) {
    case G1_DBL: return {36, 0, 36};
    case G1_ADD: return {36, 36, 36};
    case G1_ADD_MIXED: return {36, 24, 36};
    case G1X_DBL: return {48, 0, 48};
    case G1X_ADD: return {48, 48, 48};
    case G1X_ADD_MIXED: return {48, 24, 48};
    case G1X_TO_JAC: return {48, 0, 36};
    case G1_TO_AFFINE: return {36, 0, 24};
    case G1_TO_AFFINE_ZI: return {36, 12, 24};  // b: Z^-1
    case G1_MUL_SMALL: return {36, 1, 36};      // b: the u32 scalar
    case G1_FROM_AFFINE: return {24, 0, 36};
    default: return {0, 0, 0};
  }
}

template <class T>
ZK_HD T load(const uint32_t* p) {
  T r;
  uint32_t* w = reinterpret_cast<uint32_t*>(&r);
  for (uint32_t i = 0; i < sizeof(T) / 4; ++i) w[i] = p[i];
  return r;
}
template <class T>
ZK_HD void store(uint32_t* p, const T& v) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
  for (uint32_t i = 0; i < sizeof(T) / 4; ++i) p[i] = w[i];
}
static_assert(sizeof(Fq) == 48 && sizeof(G1A) == 96 && sizeof(G1J) == 144 && sizeof(G1XYZZ) == 192, "packed limbs");

template <int OP>
ZK_HD void fq_apply(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const Fq x = load<Fq>(a);
  Fq r = fq_zero();
  if constexpr (OP == FQ_ADD) r = fq_add(x, load<Fq>(b));
  if constexpr (OP == FQ_SUB) r = fq_sub(x, load<Fq>(b));
  if constexpr (OP == FQ_NEG) r = fq_neg(x);
  if constexpr (OP == FQ_DBL) r = fq_dbl(x);
  if constexpr (OP == FQ_MUL) r = fq_mul(x, load<Fq>(b));
  if constexpr (OP == FQ_SQR) r = fq_sqr(x);
  if constexpr (OP == FQ_TO_MONT) r = fq_to_mont(x);
  if constexpr (OP == FQ_FROM_MONT) r = fq_from_mont(x);
  if constexpr (OP == FQ_INV) r = fq_inv(x);
  if constexpr (OP == FQ_REDUCE_ONCE) r = fq_reduce_once(x);
  if constexpr (OP == FQ_IS_CANONICAL) r.v[0] = fq_is_canonical(x) ? 1u : 0u;  // (the flag in word 0, the rest 0)
  store(out, r);
}
constexpr bool fq_binary(int op) { return op == FQ_ADD || op == FQ_SUB || op == FQ_MUL; }

template <int OP>
ZK_HD void g1_apply(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if constexpr (OP == G1_DBL) store(out, g1_dbl(load<G1J>(a)));
  if constexpr (OP == G1_ADD) store(out, g1_add(load<G1J>(a), load<G1J>(b)));
  if constexpr (OP == G1_ADD_MIXED) store(out, g1_add_mixed(load<G1J>(a), load<G1A>(b)));
  if constexpr (OP == G1X_DBL) store(out, g1x_dbl(load<G1XYZZ>(a)));
  if constexpr (OP == G1X_ADD) store(out, g1x_add(load<G1XYZZ>(a), load<G1XYZZ>(b)));
  if constexpr (OP == G1X_ADD_MIXED) store(out, g1x_add_mixed(load<G1XYZZ>(a), load<G1A>(b)));
  if constexpr (OP == G1X_TO_JAC) store(out, g1x_to_jac(load<G1XYZZ>(a)));
  if constexpr (OP == G1_TO_AFFINE) store(out, g1_to_affine(load<G1J>(a)));
  if constexpr (OP == G1_TO_AFFINE_ZI) store(out, g1_to_affine_zi(load<G1J>(a), load<Fq>(b)));
  if constexpr (OP == G1_MUL_SMALL) store(out, g1_mul_small(load<G1J>(a), b[0]));
  if constexpr (OP == G1_FROM_AFFINE) store(out, g1_from_affine(load<G1A>(a)));
}

template <int OP>
__global__ __launch_bounds__(kThreads) void k_fq(const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  fq_apply<OP>(a + 12 * i, fq_binary(OP) ? b + 12 * i : a, out + 12 * i);
}
template <int OP>
__global__ __launch_bounds__(kThreads) void k_g1(const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const Shape s = g1_shape(OP);
  g1_apply<OP>(a + (uint64_t)s.a * i, s.b ? b + (uint64_t)s.b * i : a, out + (uint64_t)s.out * i);
}

// device buffers of one call, freed on every path
struct Bufs {
  uint32_t *a = nullptr, *b = nullptr, *out = nullptr;
  ~Bufs() {
    (void)hipFree(a);
    (void)hipFree(b);
    (void)hipFree(out);
  }
};
#define PROBE_HIP(x)                         \
  do {                                       \
    const hipError_t e_ = (x);               \
    if (e_ != hipSuccess) return 1000 + (int)e_; \
  } while (0)

// copy in, run `launch(a, b, out)` on n threads' worth of blocks, copy out
template <class Launch>
int on_device(const uint32_t* a, uint32_t wa, const uint32_t* b, uint32_t wb, uint64_t n, uint32_t* out, uint32_t wo,
              Launch&& launch) {
  Bufs d;
  PROBE_HIP(hipMalloc(&d.a, n * wa * 4));
  PROBE_HIP(hipMalloc(&d.out, n * wo * 4));
  PROBE_HIP(hipMemcpy(d.a, a, n * wa * 4, hipMemcpyHostToDevice));
  if (wb) {
    PROBE_HIP(hipMalloc(&d.b, n * wb * 4));
    PROBE_HIP(hipMemcpy(d.b, b, n * wb * 4, hipMemcpyHostToDevice));
  }
  launch(d.a, d.b, d.out);
  PROBE_HIP(hipGetLastError());
  PROBE_HIP(hipDeviceSynchronize());
  PROBE_HIP(hipMemcpy(out, d.out, n * wo * 4, hipMemcpyDeviceToHost));
  return 0;
}

template <int OP>
int run_fq(int device, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  if (!device) {
    for (uint64_t i = 0; i < n; ++i) fq_apply<OP>(a + 12 * i, fq_binary(OP) ? b + 12 * i : a, out + 12 * i);
    return 0;
  }
  const uint32_t blocks = (uint32_t)((n + kThreads - 1) / kThreads);
  return on_device(a, 12, b, fq_binary(OP) ? 12 : 0, n, out, 12, [&](uint32_t* da, uint32_t* db, uint32_t* dout) {
    k_fq<OP><<<blocks, kThreads>>>(da, db, n, dout);
  });
}
template <int OP>
int run_g1(int device, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  const Shape s = g1_shape(OP);
  if (!device) {
    for (uint64_t i = 0; i < n; ++i)
      g1_apply<OP>(a + (uint64_t)s.a * i, s.b ? b + (uint64_t)s.b * i : a, out + (uint64_t)s.out * i);
    return 0;
  }
  const uint32_t blocks = (uint32_t)((n + kThreads - 1) / kThreads);
  return on_device(a, s.a, b, s.b, n, out, s.out, [&](uint32_t* da, uint32_t* db, uint32_t* dout) {
    k_g1<OP><<<blocks, kThreads>>>(da, db, n, dout);
  });
}
}  // namespace

extern "C" {

// out[i] = op(a[i] [, b[i]]) over n Fq elements; b is read by add, sub and mul only
int zk_ecprobe_fq(int op, int device, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  if (op < 0 || op >= FQ_NOPS) return 1;
  if (n == 0) return 0;
  if (!a || !out || (fq_binary(op) && !b)) return 2;
  switch (op) {
    case FQ_ADD: return run_fq<FQ_ADD>(device, a, b, n, out);
    case FQ_SUB: return run_fq<FQ_SUB>(device, a, b, n, out);
    case FQ_NEG: return run_fq<FQ_NEG>(device, a, b, n, out);
    case FQ_DBL: return run_fq<FQ_DBL>(device, a, b, n, out);
    case FQ_MUL: return run_fq<FQ_MUL>(device, a, b, n, out);
    case FQ_SQR: return run_fq<FQ_SQR>(device, a, b, n, out);
    case FQ_TO_MONT: return run_fq<FQ_TO_MONT>(device, a, b, n, out);
    case FQ_FROM_MONT: return run_fq<FQ_FROM_MONT>(device, a, b, n, out);
    case FQ_INV: return run_fq<FQ_INV>(device, a, b, n, out);
    case FQ_REDUCE_ONCE: return run_fq<FQ_REDUCE_ONCE>(device, a, b, n, out);
    default: return run_fq<FQ_IS_CANONICAL>(device, a, b, n, out);
  }
}

// words per element of a, b (0: unused) and out for a G1 op; 1 for an unknown op
int zk_ecprobe_g1_shape(int op, uint32_t shape[3]) {
  if (op < 0 || op >= G1_NOPS || !shape) return 1;
  const Shape s = g1_shape(op);
  shape[0] = s.a;
  shape[1] = s.b;
  shape[2] = s.out;
  return 0;
}

// out[i] = op(a[i] [, b[i]]) over n elements laid out as zk_ecprobe_g1_shape says
int zk_ecprobe_g1(int op, int device, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out) {
  if (op < 0 || op >= G1_NOPS) return 1;
  if (n == 0) return 0;
  if (!a || !out || (g1_shape(op).b && !b)) return 2;
  switch (op) {
    case G1_DBL: return run_g1<G1_DBL>(device, a, b, n, out);
    case G1_ADD: return run_g1<G1_ADD>(device, a, b, n, out);
    case G1_ADD_MIXED: return run_g1<G1_ADD_MIXED>(device, a, b, n, out);
    case G1X_DBL: return run_g1<G1X_DBL>(device, a, b, n, out);
    case G1X_ADD: return run_g1<G1X_ADD>(device, a, b, n, out);
    case G1X_ADD_MIXED: return run_g1<G1X_ADD_MIXED>(device, a, b, n, out);
    case G1X_TO_JAC: return run_g1<G1X_TO_JAC>(device, a, b, n, out);
    case G1_TO_AFFINE: return run_g1<G1_TO_AFFINE>(device, a, b, n, out);
    case G1_TO_AFFINE_ZI: return run_g1<G1_TO_AFFINE_ZI>(device, a, b, n, out);
    case G1_MUL_SMALL: return run_g1<G1_MUL_SMALL>(device, a, b, n, out);
    default: return run_g1<G1_FROM_AFFINE>(device, a, b, n, out);
  }
}

}  // extern "C"
