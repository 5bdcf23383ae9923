// gfx950 kernels of the sum-check hot path (device code; included once by
// sumcheck.hip). Tables are arrays of 32-byte Montgomery elements in HBM,
// index bit (n-1-i) <-> variable i (variable 0 = MSB), exactly the
// `Vec<F>` layout of MultilinearPoly (multilinear_polynomial_evaluation.rs:19-37).
//
// Every fold in the hot path is `partial_evaluate(0, r)` (:52-63): the pair
// (j, j + L/2) collapses to a + r(b - a), so both operands of every pair sit
// in two contiguous half-tables and every load/store is a coalesced 32-byte
// per-lane access (two dwordx4).
#pragma once
#include "field.hpp"
#include "dfs.hpp"
#include "gkr_plan.hpp"  // tail_region, dtail_region

namespace zk {

constexpr int kBlock = 256;  // 4 waves of 64

// Device bounds checks (debug build only: make -C
// zk-research-implementations_amd checks, -DZK_DEVICE_CHECKS): every table
// index of the matrix-core and MSM kernels is asserted against the table's
// length; a failure prints the condition, block and thread, then traps.
#ifdef ZK_DEVICE_CHECKS
#define ZK_DCHECK(cond)                                                                                          \
  do {                                                                                                           \
    if (!(cond)) {                                                                                               \
      printf("zk device check failed: %s (%s:%d) block %u thread %u\n", #cond, __FILE__, __LINE__, blockIdx.x, \
             threadIdx.x);                                                                                       \
      __builtin_trap();                                                                                          \
    }                                                                                                            \
  } while (0)
#else
#define ZK_DCHECK(cond) \
  do {                  \
  } while (0)
#endif

__device__ __forceinline__ Fe ld_fe(const Fe* __restrict__ p, uint64_t i) {
  const uint4* q = reinterpret_cast<const uint4*>(p) + 2 * i;
  const uint4 a = q[0], b = q[1];
  Fe r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
}
// a pointer the compiler cannot prove wave-uniform (selected by the wave
// index), made uniform: its address arithmetic stays on the scalar unit
__device__ __forceinline__ const Fe* uniform_ptr(const Fe* p) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return reinterpret_cast<const Fe*>(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void st_fe(Fe* __restrict__ p, uint64_t i, const Fe& x) {
  uint4* q = reinterpret_cast<uint4*>(p) + 2 * i;
  q[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  q[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}
// (Folded tables are stored with st_fe too: plain write-back stores. A
// non-temporal hint and write-through (sc1) stores were tried, so that a round
// would not end with the L2 full of dirty table lines; plain stores won.)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// An element as four 64-bit words (the 8-byte accesses of the tables that
// blocks hand to each other, and of the host tables): word k = limbs 2k, 2k+1.
__device__ __forceinline__ uint64_t fe_word64(const Fe& x, int k) {
  return (uint64_t)x.v[2 * k] | ((uint64_t)x.v[2 * k + 1] << 32);
}
__device__ __forceinline__ void fe_set_word64(Fe& x, int k, uint64_t w) {
  x.v[2 * k] = (uint32_t)w;
  x.v[2 * k + 1] = (uint32_t)(w >> 32);
}
// Element loads and stores whose bytes another block of the SAME kernel reads
// or wrote (k_gkr_tail, k_gkr_dtail): relaxed agent-scope 8-byte atomics (sc1)
// on both sides, MI355X_MICROARCH.md "Valid forms".
__device__ __forceinline__ Fe ld_fe_a(const Fe* p, uint64_t i) {
  const uint64_t* q = reinterpret_cast<const uint64_t*>(p + i);
  Fe r;
#pragma unroll
  for (int k = 0; k < 4; ++k) fe_set_word64(r, k, __hip_atomic_load(q + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return r;
}
__device__ __forceinline__ void st_fe_a(Fe* p, uint64_t i, const Fe& x) {
  uint64_t* q = reinterpret_cast<uint64_t*>(p + i);
#pragma unroll
  for (int k = 0; k < 4; ++k) __hip_atomic_store(q + k, fe_word64(x, k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// element i of a word-major table of n elements in pinned host memory (word k
// at k n + i), system-scope stores: see k_gkr_dtail
__device__ __forceinline__ void st_fe_sys(uint64_t* p, uint64_t n, uint64_t i, const Fe& x) {
#pragma unroll
  for (int k = 0; k < 4; ++k) __hip_atomic_store(p + k * n + i, fe_word64(x, k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// How a round step reads and writes table elements: a one-launch kernel with
// plain 32-byte accesses, all loads of an output issued before any arithmetic
// where the step says so (sched_barrier, the tuned form of the double round);
// a persistent kernel with the agent-scope atomics above and no such fence.
struct PlainIo {
  static __device__ __forceinline__ Fe ld(const Fe* p, uint64_t i) { return ld_fe(p, i); }
  static __device__ __forceinline__ void st(Fe* p, uint64_t i, const Fe& x) { st_fe(p, i, x); }
  static __device__ __forceinline__ void loads_first() { __builtin_amdgcn_sched_barrier(0); }
};
struct AgentIo {
  static __device__ __forceinline__ Fe ld(const Fe* p, uint64_t i) { return ld_fe_a(p, i); }
  static __device__ __forceinline__ void st(Fe* p, uint64_t i, const Fe& x) { st_fe_a(p, i, x); }
  static __device__ __forceinline__ void loads_first() {}
};

// a + r (b - a)
template <class F>
__device__ __forceinline__ Fe fold1(const Fe& a, const Fe& b, const Fe& r) {
  return fe_add<F>(a, fe_mul<F>(r, fe_sub<F>(b, a)));
}
// X(2) = 2 X_hi - X_lo  (partial_evaluate at F::from(2))
template <class F>
__device__ __forceinline__ Fe at2(const Fe& lo, const Fe& hi) {
  return fe_sub<F>(fe_dbl<F>(hi), lo);
}

// ---------------------------------------------------------------------------
// Folding by challenges that are constant for a whole step. For a challenge x
// the block builds, once, the 10 constants c_x[k] = x * 2^(26k + 64) mod p
// (k = 0..9: `fold_consts`, one Montgomery multiply each by the compile-time
// K_k = 2^(26k+64) mod p). A product x * d (d a Montgomery image) is then
//   sum_k d_k c_x[k] = x d 2^64 (mod p), d_k = 26-bit limbs of d,
// whose eight 32-bit column sums stay below 2^63 even for three challenges
// at once, so every column is ONE chain of v_mad_u64_u32 with its 64-bit
// addend (no carry instructions), followed by two 32-bit REDC steps
// (/2^64: the Montgomery image of x d, < 2p) and one conditional subtraction.
// 80 + 16 multiply-adds for one fold (fe_mul: 136 plus ~140 carry
// instructions); 240 + 16 for the three products of fold2.
// ---------------------------------------------------------------------------
#define ZK_FOLDK_INIT(F)                                                                                            \
  {pow2_mod_p<F>(64), pow2_mod_p<F>(90), pow2_mod_p<F>(116), pow2_mod_p<F>(142), pow2_mod_p<F>(168),                 \
   pow2_mod_p<F>(194), pow2_mod_p<F>(220), pow2_mod_p<F>(246), pow2_mod_p<F>(272), pow2_mod_p<F>(298)}
static __constant__ Fe kFoldKBn254Fr[10] = ZK_FOLDK_INIT(Bn254Fr);
static __constant__ Fe kFoldKBn254Fq[10] = ZK_FOLDK_INIT(Bn254Fq);
static __constant__ Fe kFoldKBls12_381Fr[10] = ZK_FOLDK_INIT(Bls12_381Fr);
template <class F>
__device__ __forceinline__ Fe foldk(uint32_t k) {
  if constexpr (F::id == BN254_FR) return kFoldKBn254Fr[k];
  else if constexpr (F::id == BN254_FQ) return kFoldKBn254Fq[k];
  else return kFoldKBls12_381Fr[k];
}
// ct[10 x + k] = c_x[k] for the NX challenges xs (Montgomery images); ends with a barrier
template <class F, int NX>
__device__ __forceinline__ void fold_consts(const Fe& x0, const Fe& x1, const Fe& x2, Fe (&ct)[NX * 10]) {
  const uint32_t t = threadIdx.x;
  if (t < (uint32_t)(NX * 10)) {
    const uint32_t x = t / 10, k = t % 10;
    const Fe r = x == 0 ? x0 : (x == 1 ? x1 : x2);
    ct[t] = fe_mul<F>(r, foldk<F>(k));  // x R K R^-1 = x K
  }
  __syncthreads();
}
// sum_x d[x] * challenge(OFF + x) mod p (Montgomery images in, fully reduced out)
template <class F, int NX, int OFF, int NC>
__device__ __forceinline__ Fe lin_redc(const Fe (&d)[NX], const Fe (&ct)[NC]) {
  static_assert(OFF + NX <= NC / 10, "constant table too small");
  uint64_t S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int x = 0; x < NX; ++x) {
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      const int bit = 26 * k, w = bit >> 5, o = bit & 31;
      const uint32_t lo = d[x].v[w], hi = w + 1 < 8 ? d[x].v[w + 1] : 0u;
      const uint32_t dk = (o == 0 ? lo : __builtin_amdgcn_alignbit(hi, lo, (uint32_t)o)) & 0x3FFFFFFu;
      const Fe c = ct[(OFF + x) * 10 + k];
#pragma unroll
      for (int j = 0; j < 8; ++j) S[j] = (uint64_t)dk * c.v[j] + S[j];
    }
  }
  uint32_t t[10];
  t[0] = (uint32_t)S[0];
  uint64_t carry = S[0] >> 32;
#pragma unroll
  for (int j = 1; j < 8; ++j) {
    const uint64_t v = S[j] + carry;
    t[j] = (uint32_t)v;
    carry = v >> 32;
  }
  t[8] = (uint32_t)carry;
  t[9] = (uint32_t)(carry >> 32);
#pragma unroll
  for (int st = 0; st < 2; ++st) {  // REDC by 2^32, twice
    const uint32_t m = t[0] * F::PINV;
    uint64_t Q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) Q[j] = mad64(m, F::P[j], t[j]);
    uint32_t c = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) t[j - 1] = addc32((uint32_t)Q[j], (uint32_t)(Q[j - 1] >> 32), c, &c);
    t[7] = addc32(t[8], (uint32_t)(Q[7] >> 32), c, &c);
    t[8] = t[9] + c;
    t[9] = 0;
  }
  Fe r;  // < 2p < 2^256: t[8] == 0
#pragma unroll
  for (int j = 0; j < 8; ++j) r.v[j] = t[j];
  return fe_reduce_once<F>(r);
}
// a + r (b - a) with r's constants at block OFF of ct
template <class F, int OFF, int NC>
__device__ __forceinline__ Fe fold1c(const Fe& a, const Fe& b, const Fe (&ct)[NC]) {
  const Fe d[1] = {fe_sub<F>(b, a)};
  return fe_add<F>(a, lin_redc<F, 1, OFF>(d, ct));
}
// fold2 (field.hpp) with the constants of (ra, rb, ra rb) at blocks 0, 1, 2 of ct
template <class F, int NC>
__device__ __forceinline__ Fe fold2c(const Fe& x00, const Fe& x01, const Fe& x10, const Fe& x11, const Fe (&ct)[NC]) {
  const Fe d1 = fe_sub<F>(x10, x00), d2 = fe_sub<F>(x01, x00);
  const Fe d[3] = {d1, d2, fe_sub<F>(fe_sub<F>(x11, x01), d1)};
  return fe_add<F>(x00, lin_redc<F, 3, 0>(d, ct));
}

// Where a round kernel's sums go. Everything after the main loop is integer
// work: a thread's accumulators (17-word unreduced product sums `Wide`, or
// 8-word element sums `Fe`) are summed over the block column by column
// (one u64 per 32-bit word: "limb sums", exact, no carries, no reduction mod
// p) through an LDS transpose, then over the grid, and the C = K*L limb sums
// are handed over as they are. The consumer (host: limbs_to_fe) does the one
// carry propagation + REDC. The multi-GPU all-reduce sums the same u64 vector.
//
// Cross-block fan-in: a single block publishes directly; up to
// RoundSink::atomic_max blocks (1024 by default, ZK_ATOMIC_FANIN) add their
// limb sums with u64 atomics and count in (measured 11 us per 24-var proof
// faster than the two-level fan-in for the 256-512-block matrix-core grids);
// larger grids meet in two levels (blockIdx % 8 shards, then a top counter)
// through per-block slots written/read with write-through (sc1) 8-byte
// accesses (MI355X_MICROARCH.md "Valid forms": no release/acquire fence, so
// the dirty L2 full of freshly folded table lines is never written back
// mid-kernel). The last block writes the totals to dev_out and/or pinned host
// memory and raises host_flag = tag; the host spins on that flag instead of
// synchronising the stream.
//
// Phase timestamps for tools/microbench_phases.hip (compile-time, off in the
// library): block b writes s_memrealtime (100 MHz, device-global) into
// zk_phase_trace[b * 8 + i] from thread 0.
#ifdef ZK_PHASE_TRACE
#define ZK_STAMP(i) \
  do { if (threadIdx.x == 0) zk_phase_trace[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// ZK_STAMP_AFTER(i, w): stamp once the 17-word accumulator w is computed
#define ZK_STAMP_AFTER(i, a_)                                         \
  do {                                                                 \
    uint32_t x_ = 0;                                                   \
    for (int k_ = 0; k_ < 17; ++k_) x_ ^= (a_).w[k_];                  \
    asm volatile("; stamp dep %0" ::"v"(x_));                          \
    ZK_STAMP(i);                                                       \
  } while (0)
#else
#define ZK_STAMP(i) do { } while (0)
#define ZK_STAMP_AFTER(i, w) do { } while (0)
#endif

constexpr int kSlotU64 = 256;  // per-block partial slot: up to 256 limb sums (2 KiB)

// Peer reduction (zk_ctx_attach_peer_reduce): the block that publishes a
// step's sums writes them straight into every rank's receive buffer (an
// uncached device allocation, IPC-mapped into each peer) and sums the world's
// contributions itself — the sharded step's all-reduce without an RCCL launch
// or a publish kernel. Receive buffer: [2 parities][world][kPeerSlotU64] u64,
// the slot's last word its sequence tag (the same on every rank: one per
// reduction, in schedule order). Parity (seq & 1) double-buffers the slots:
// a rank can only send reduction seq once it has every rank's seq - 1, which
// each rank sends after it has finished reading seq - 2 (the same parity).
constexpr uint32_t kPeerMax = 8;        // ranks of one node
constexpr uint32_t kPeerSlotU64 = 512;  // up to kSlotU64 sums, tag in the last word
constexpr uint64_t kPeerWaitTicks = 1000000000ull;  // 10 s of s_memrealtime: then flag an error and go on
constexpr uint32_t kPeerGatherMaxT = 12;  // the early gather through the peers up to 4 x 2^12 elements per rank
struct PeerSlots {
  uint64_t* slot[kPeerMax];    // rank r's receive buffer as mapped in this process (slot[rank]: our own)
  uint64_t* gather[kPeerMax];  // rank r's gather buffer: [world][4 x 2^kPeerGatherMaxT elements], then world tags
  uint32_t world, rank;
};
// Ordering of a peer hand-off (data words -> tag) in the memory model's own
// terms: the producer drains its data stores, then a SYSTEM-scope
// release fence, then the relaxed tag store; the consumer polls the tag with
// relaxed loads, then a SYSTEM-scope acquire fence, then reads the data. The
// buffers are uncached device memory and every data access is a system-scope
// (sc0 sc1) access as well, so the hardware would order them without the
// fences; ZK_PEER_FENCE=0 builds that form for the A/B of their cost
// (profiles/r6_peer_fence_ab.txt).
#ifndef ZK_PEER_FENCE
#define ZK_PEER_FENCE 1
#endif
__device__ __forceinline__ void peer_release_fence() {
#if ZK_PEER_FENCE
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the guide's compiler hazard: the flag never overtakes the write-back)
#endif
}
__device__ __forceinline__ void peer_acquire_fence() {
#if ZK_PEER_FENCE
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the polls
#endif
}


struct RoundSink {
  uint64_t* partials;   // [gridDim.x + 8][kSlotU64]: one slot per block, then 8 shard slots
  uint32_t* counter;    // 9 counters, 128 B apart: 8 XCD shards + top; zero at launch, reset by their last user
  uint64_t* accum;      // C u64 accumulator (small grids); zero at launch, reset by the last block
  uint64_t* dev_out;    // C u64 in device memory, or null
  uint64_t* host_out;   // C u64 in pinned host memory, or null
  uint32_t* host_flag;  // pinned host word, or null
  uint32_t tag;
  uint64_t* trace;      // debug (ZK_DEBUG_TAIL): 4 s_memrealtime stamps per tag (entry, challenge, publish), or null
  uint64_t* btrace;     // debug (ZK_DEBUG_BLOCKS): 8 words per block (stamps: main loop end, fan-in start, counted in; chunk count; flushed, words), or null
  uint32_t atomic_max;  // grids up to this many blocks fan in through u64 atomics (ZK_ATOMIC_FANIN)
  const PeerSlots* peer;  // sums across ranks through the peers' receive buffers, or null
  uint64_t peer_seq;      // this reduction's sequence tag (peer != null)
  uint32_t* err;          // pinned error word (a peer that never arrives), or null
};
#define ZK_BLOCK_STAMP(sk, i) \
  do { if ((sk).btrace && threadIdx.x == 0 && blockIdx.x < 8192) (sk).btrace[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// block 0 / the publishing block stamps slot i of this sink's trace row
#define ZK_SINK_STAMP(sk, i) \
  do { if ((sk).trace && threadIdx.x == 0) (sk).trace[((sk).tag & 63) * 4 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)

// ---------------------------------------------------------------------------
// Pre-enqueued rounds. The host enqueues every round kernel up front; round
// k's kernel starts as soon as round k-1's ends and waits, in-kernel, for the
// host to post r_{k-1} (after reading round k-1's sums and running the
// transcript). Only thread 0 of block 0 polls the pinned host slot: uncached
// reads of one host address from several pollers serialise (~1.5 us each,
// measured: 64 polling blocks added ~100 us to a round). Block 0 relays r
// through a device word that the other blocks poll. Every wait gives up after
// ~1 s and flags an error (the host then fails the call): no wave can spin
// forever.
// ---------------------------------------------------------------------------
struct alignas(64) RWait {
  Fe r;          // Montgomery
  uint32_t tag;  // valid for every kernel expecting a tag <= this one (tags increase)
  uint32_t pad[7];
};
struct RoundIn {
  Fe r;                // used as is when host == null
  const RWait* host;   // pinned slot the host posts r to, or null
  RWait* relay;        // device relay slot (zeroed tag at rest), used when gridDim > 1
  uint32_t* err;       // pinned error word
  uint32_t tag;
};
constexpr uint64_t kWaitTicks = 100000000ull;  // 1 s of s_memrealtime (100 MHz)

// The challenge the host posts to `host` under `tag`, in every thread of the
// block (ends with a barrier). Thread 0 of block 0 polls the host slot and,
// when other blocks wait too (`relayed`), copies r to the one relay slot:
// write-through stores, drained before the tag that announces them. Thread 0
// of every other block polls the relay (sleep 1 between polls). One slot that
// all blocks poll measured best: 8 replicas (block b polling slot b % 8) cost
// block 0 more than they saved the pollers. A wait that runs out sets *err.
__device__ __forceinline__ Fe block_wait_r(const RWait* host, RWait* relay, bool relayed, uint32_t tag, uint32_t* err) {
  __shared__ Fe s_r;
  if (threadIdx.x == 0) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    bool ok = true;
    Fe r;
    if (blockIdx.x == 0) {
      // relaxed system-scope polls: uncached (sc0 sc1) loads with no cache
      // invalidate per iteration; the r loads below are uncached too and issue
      // only after the tag has been seen
      while ((int32_t)(__hip_atomic_load(&host->tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - tag) < 0) {
        __builtin_amdgcn_s_sleep(2);
        if (__builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) { ok = false; break; }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) r.v[i] = __hip_atomic_load(&host->r.v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (relayed) {
#pragma unroll
        for (int i = 0; i < 8; ++i) __hip_atomic_store(&relay->r.v[i], r.v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&relay->tag, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    } else {
      while ((int32_t)(__hip_atomic_load(&relay->tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - tag) < 0) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) { ok = false; break; }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) r.v[i] = __hip_atomic_load(&relay->r.v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!ok) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    s_r = r;
  }
  __syncthreads();
  return s_r;
}
// a round kernel's challenge: the argument itself, or awaited (pre-enqueued rounds)
__device__ __forceinline__ Fe block_get_r(const RoundIn& in) {
  if (!in.host) return in.r;
  return block_wait_r(in.host, in.relay, gridDim.x > 1, in.tag, in.err);
}

__device__ __forceinline__ void st_u64_sc1(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_u64_sc1(uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Shared scratch of the epilogue (one instance per kernel).
template <int L>
struct LimbScratch {
  static constexpr int S = L | 1;  // odd row stride: conflict-free column reads
  uint32_t rows[kBlock * S];
  uint64_t tot[kSlotU64];
  uint64_t pp[kBlock];
  uint32_t am_last;
};

// Column sums of one L-word value per thread over the block -> sc.tot[base + c]
// (valid in threads < L after the call). Every thread then sums one column
// over a strided group of rows (G = kBlock / L groups, ~kBlock / G rows each);
// threads < L add the G group sums.
template <int L, class Sc>
__device__ __forceinline__ void block_limb_sums(const uint32_t (&v)[L], Sc& sc, int base) {
  constexpr uint32_t G = kBlock / L;
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < L; ++i) sc.rows[t * Sc::S + i] = v[i];
  __syncthreads();
  const uint32_t c = t % L, g = t / L;
  uint64_t s0 = 0, s1 = 0;
  if (g < G) {
    uint32_t r = g;
    for (; r + G < (uint32_t)kBlock; r += 2 * G) {
      s0 += sc.rows[r * Sc::S + c];
      s1 += sc.rows[(r + G) * Sc::S + c];
    }
    if (r < (uint32_t)kBlock) s0 += sc.rows[r * Sc::S + c];
  }
  sc.pp[t] = s0 + s1;
  __syncthreads();
  if (t < (uint32_t)L) {
    uint64_t tot = 0;
#pragma unroll
    for (uint32_t q = 0; q < G; ++q) tot += sc.pp[q * L + t];
    sc.tot[base + t] = tot;
  }
}
template <class Sc>
__device__ __forceinline__ void block_limb_sums(const Wide& w, Sc& sc, int base) {
  block_limb_sums<17>(w.w, sc, base);
}
template <class Sc>
__device__ __forceinline__ void block_limb_sums(const Fe& x, Sc& sc, int base) {
  block_limb_sums<8>(x.v, sc, base);
}

// sc.tot[0..C) (written by wave 0 lanes) -> dev_out / host_out + host flag.
// Wave 0 only: its lanes store the host copy with system-scope (write-through,
// sc0 sc1) stores — plain stores to the pinned page would sit in L2 — drain,
// then lane 0 raises the flag. No L2 writeback (buffer_wbl2) is needed since
// nothing the host reads was written with plain stores.
// The world's sum of this rank's value v (threads < C; the publishing waves
// only: wave 0 when C <= 64, else the whole block). Stores and polls are
// system-scope (sc0 sc1: they bypass the caches), and every store has
// drained before the tag that announces it is written.
template <int C>
__device__ __forceinline__ uint64_t peer_allreduce(uint64_t v, const RoundSink& sk) {
  const uint32_t t = threadIdx.x;
  const PeerSlots* ps = sk.peer;
  const uint32_t W = ps->world, me = ps->rank;
  const uint64_t par = sk.peer_seq & 1u;
  const uint64_t mine = (par * W + me) * kPeerSlotU64;
  if (t < (uint32_t)C)
    for (uint32_t r = 0; r < W; ++r) __hip_atomic_store(ps->slot[r] + mine + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (C > 64) __syncthreads();  // every storing wave has drained before the tags
  if (t == 0) {
    peer_release_fence();
    for (uint32_t r = 0; r < W; ++r)
      __hip_atomic_store(ps->slot[r] + mine + kPeerSlotU64 - 1, sk.peer_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  uint64_t* own = ps->slot[me];
  if (t < W) {  // lane r waits for rank r's tag
    const uint64_t* tag = own + (par * W + t) * kPeerSlotU64 + kPeerSlotU64 - 1;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != sk.peer_seq) {
      __builtin_amdgcn_s_sleep(1);
      if (__builtin_amdgcn_s_memrealtime() - t0 > kPeerWaitTicks) {
        if (sk.err) __hip_atomic_store(sk.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
    }
  }
  if (C > 64) __syncthreads();  // (C <= 64: wave 0 alone, reconverged after the polls)
  peer_acquire_fence();  // every loading wave: after the polls (and the barrier), before the data loads
  uint64_t s = 0;
  if (t < (uint32_t)C)
    for (uint32_t r = 0; r < W; ++r) s += __hip_atomic_load(own + (par * W + r) * kPeerSlotU64 + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return s;
}

template <int C, class Sc>
__device__ __forceinline__ void publish_limbs(Sc& sc, const RoundSink& sk) {
  const uint32_t t = threadIdx.x;
  if (C <= 64 && t >= 64) return;  // wave 0 alone
  uint64_t pv = 0;
  if (sk.peer) pv = peer_allreduce<C>(t < (uint32_t)C ? sc.tot[t] : 0, sk);
  if (t < (uint32_t)C) {
    const uint64_t v = sk.peer ? pv : sc.tot[t];
    if (sk.dev_out) sk.dev_out[t] = v;
    if (sk.host_out) __hip_atomic_store(sk.host_out + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ZK_SINK_STAMP(sk, 2);
  if (C > 64) __syncthreads();  // every storing wave has drained before the flag
  if (t == 0 && sk.host_flag) __hip_atomic_store(sk.host_flag, sk.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// sum `count` slots (slot index first + i*stride) of C limb sums -> sc.tot (wave 0 lanes)
template <int C, class Sc>
__device__ __forceinline__ void sum_slots(uint64_t* slots, uint32_t first, uint32_t stride, uint32_t count, Sc& sc) {
  constexpr uint32_t P = kBlock / C;  // parts per column
  const uint32_t t = threadIdx.x, c = t % C, p = t / C;
  uint64_t s = 0;
  if (p < P) {
    uint32_t i = p;
    for (; i + 7 * P < count; i += 8 * P) {  // 8 independent loads in flight
      uint64_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ld_u64_sc1(slots + (uint64_t)(first + (i + u * P) * stride) * kSlotU64 + c);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; i < count; i += P) s += ld_u64_sc1(slots + (uint64_t)(first + i * stride) * kSlotU64 + c);
  }
  sc.pp[t] = s;
  __syncthreads();
  if (t < (uint32_t)C) {
    uint64_t tot = 0;
    for (uint32_t q = 0; q < P; ++q) tot += sc.pp[q * C + t];
    sc.tot[t] = tot;
  }
}

// Counting in: what a block wrote for the others (slot stores, accumulator
// adds, table stores) is complete before the others can see it counted. Every
// wave drains its own stores (vmcnt(0)), the barrier collects the waves, then
// thread 0 adds 1 to `counter` (and first zeroes `rearm`, a counter this block
// was the last to count in on, for the next launch). True in every thread of
// the n-th block to arrive (after a second barrier); what that block then
// reads are device-coherent accesses (sc1 / atomics) that hit the values
// drained before the adds. The acquire fence at wavefront scope emits no
// instruction: it keeps the compiler from moving those reads above the add.
template <class Sc>
__device__ __forceinline__ bool count_in(Sc& sc, uint32_t* counter, uint32_t n, uint32_t* rearm = nullptr) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    if (rearm) __hip_atomic_store(rearm, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sc.am_last = prev == n - 1;
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return sc.am_last;
}

// Fan-in of n blocks through the u64 accumulator: every block adds its limb
// sums sc.tot[0..C) (no-return u64 atomics, device-coherent level; n * 256 *
// 2^32 < 2^64 stays exact) and counts in; the last one takes the totals back
// into sc.tot (threads < C) and re-arms accumulator and counter for the next
// use. Returns whether this block is that last one.
template <int C, class Sc>
__device__ __forceinline__ bool atomic_fan_in(Sc& sc, const RoundSink& sk, uint32_t n) {
  const uint32_t t = threadIdx.x;
  if (t < (uint32_t)C) __hip_atomic_fetch_add(sk.accum + t, sc.tot[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = count_in(sc, sk.counter, n);
  if (last) {
    if (t < (uint32_t)C)
      sc.tot[t] = __hip_atomic_exchange(sk.accum + t, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) __hip_atomic_store(sk.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return last;
}

// Block limb sums are in sc.tot[0..C) (valid for threads < C); finish over the grid.
// G: the blocks taking part (blocks 0 .. G-1; default the whole grid).
template <int C, class Sc>
__device__ __forceinline__ void grid_finish(Sc& sc, const RoundSink& sk, uint32_t G = 0) {
  static_assert(C <= kSlotU64 && C <= kBlock, "limb vector too long");
  if (G == 0) G = gridDim.x;
  const uint32_t t = threadIdx.x;
  ZK_BLOCK_STAMP(sk, 1);
  if (G == 1) {
    ZK_STAMP(4);
    ZK_STAMP(5);
    publish_limbs<C>(sc, sk);
    ZK_STAMP(6);
    return;
  }
  if (G <= sk.atomic_max) {
    const bool last = atomic_fan_in<C>(sc, sk, G);
    ZK_STAMP(4);
    ZK_BLOCK_STAMP(sk, 2);
    if (!last) return;
    ZK_STAMP(5);
    publish_limbs<C>(sc, sk);
    ZK_STAMP(6);
    return;
  }
  const uint32_t shard = blockIdx.x & 7u, nshards = G < 8 ? G : 8u;
  const uint32_t in_shard = (G - shard + 7u) / 8u;
  if (t < (uint32_t)C) st_u64_sc1(sk.partials + (uint64_t)blockIdx.x * kSlotU64 + t, sc.tot[t]);
  const bool last_in_shard = count_in(sc, sk.counter + 32 * shard, in_shard);
  ZK_STAMP(4);
  ZK_BLOCK_STAMP(sk, 2);
  if (!last_in_shard) return;
  sum_slots<C>(sk.partials, shard, 8u, in_shard, sc);
  if (t < (uint32_t)C) st_u64_sc1(sk.partials + (uint64_t)(G + shard) * kSlotU64 + t, sc.tot[t]);
  if (!count_in(sc, sk.counter + 32 * 8, nshards, /*rearm=*/sk.counter + 32 * shard)) return;
  __syncthreads();  // pp is reused
  sum_slots<C>(sk.partials, G, 1u, nshards, sc);
  if (t == 0) __hip_atomic_store(sk.counter + 32 * 8, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ZK_STAMP(5);
  publish_limbs<C>(sc, sk);
  ZK_STAMP(6);
}

// copy n u64 (e.g. after an RCCL all-reduce) to pinned host memory + flag
static __global__ void k_publish(const uint64_t* __restrict__ src, int n, uint64_t* host_out, uint32_t* host_flag,
                          uint32_t tag) {
  for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x)  // (n <= 768: the 729-limb step)
    __hip_atomic_store(host_out + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(host_flag, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------
// GKR round 0: e_t = sum_j A_t S_t + M_t P_t for t = 0,1,2 over the input
// tables (size 2h), X_t = X_lo + t (X_hi - X_lo)  — sum_check_protocol.rs:152-166
// with composed_polynomial.rs:78-99 (reduce = A*S + M*P). 6 unreduced products / pair.
// ---------------------------------------------------------------------------
// Two threads per pair: waves alternate between the product A*S (q = 0) and
// M*P (q = 1), so a thread issues its 4 (round 0) or 8 (fused round) loads at
// once and keeps register pressure low enough for 4 waves/SIMD.
__device__ __forceinline__ void pair_slot(uint64_t& j, uint32_t& q, uint64_t& step) {
  const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  q = (uint32_t)(g >> 6) & 1u;
  j = ((g >> 7) << 6) | (g & 63);
  step = (uint64_t)gridDim.x * (kBlock / 2);
}

template <class F>
__global__ __launch_bounds__(kBlock) void k_gkr_round0(const Fe* __restrict__ A, const Fe* __restrict__ S,
                                                       const Fe* __restrict__ M, const Fe* __restrict__ P,
                                                       uint64_t h, RoundSink sink) {
  if (blockIdx.x == 0) ZK_SINK_STAMP(sink, 0);
  // products accumulate unreduced (Wide) and are reduced once per thread
  Wide w0 = wide_zero<F>(), w1 = wide_zero<F>(), w2 = wide_zero<F>();
  uint64_t j, step;
  uint32_t q;
  pair_slot(j, q, step);
  const Fe* __restrict__ X = q ? M : A;
  const Fe* __restrict__ Z = q ? P : S;
  for (; j < h; j += step) {
    const Fe x0 = ld_fe(X, j), x1 = ld_fe(X, j + h), z0 = ld_fe(Z, j), z1 = ld_fe(Z, j + h);
    __builtin_amdgcn_sched_barrier(0);  // issue all loads before any arithmetic
    wide_mac<F>(w0, x0, z0);
    wide_mac<F>(w1, x1, z1);
    wide_mac<F>(w2, at2<F>(x0, x1), at2<F>(z0, z1));
  }
  ZK_STAMP(1);
  ZK_STAMP(2);
  __shared__ LimbScratch<17> sc;
  block_limb_sums(w0, sc, 0);
  block_limb_sums(w1, sc, 17);
  block_limb_sums(w2, sc, 34);
  __syncthreads();
  ZK_STAMP(3);
  grid_finish<51>(sc, sink);
}

// ---------------------------------------------------------------------------
// GKR round k >= 1, fused: fold the previous round's tables (size 4h) by
// r_{k-1} (SumPoly::partial_evaluate(r), sum_check_protocol.rs:107) into
// out (size 2h) and accumulate this round's e0 and e2 on the folded values.
// Output pair j needs old j, j+h, j+2h, j+3h: folded lo = old[j] + r(old[j+2h]-old[j]),
// folded hi = old[j+h] + r(old[j+3h]-old[j+h]). e1 is not computed: the host
// derives it exactly as s_{k-1}(r_{k-1}) - e0. out must not alias
// in (the host ping-pongs two workspaces). 8 reduced muls + 4 unreduced products / pair.
// ---------------------------------------------------------------------------
// Measured choices: one wave per SIMD with all 256 VGPRs (asking for two made
// the kernel spill and run slower); all eight loads issued ahead of the
// arithmetic; the folds by the step-constant tables (fold1c) rather than
// fe_mul.
template <class F>
__global__ __launch_bounds__(kBlock, 1) void k_gkr_round(const Fe* __restrict__ A, const Fe* __restrict__ S,
                                                      const Fe* __restrict__ M, const Fe* __restrict__ P,
                                                      Fe* __restrict__ A2, Fe* __restrict__ S2,
                                                      Fe* __restrict__ M2, Fe* __restrict__ P2, uint64_t h,
                                                      RoundIn rin, RoundSink sink) {
  ZK_STAMP(0);
  if (blockIdx.x == 0) ZK_SINK_STAMP(sink, 0);
  const Fe r = block_get_r(rin);
  if (blockIdx.x == 0) ZK_SINK_STAMP(sink, 1);
  __shared__ Fe ct[10];
  fold_consts<F, 1>(r, r, r, ct);
  Wide w0 = wide_zero<F>(), w2 = wide_zero<F>();
  uint64_t j, step;
  uint32_t q;
  pair_slot(j, q, step);
  const Fe* __restrict__ X = q ? M : A;
  const Fe* __restrict__ Z = q ? P : S;
  Fe* __restrict__ X2 = q ? M2 : A2;
  Fe* __restrict__ Z2 = q ? P2 : S2;
  for (; j < h; j += step) {
    const Fe x0 = ld_fe(X, j), x1 = ld_fe(X, j + h), x2 = ld_fe(X, j + 2 * h), x3 = ld_fe(X, j + 3 * h);
    const Fe z0 = ld_fe(Z, j), z1 = ld_fe(Z, j + h), z2 = ld_fe(Z, j + 2 * h), z3 = ld_fe(Z, j + 3 * h);
    __builtin_amdgcn_sched_barrier(0);  // issue all loads before any arithmetic
    const Fe a0 = fold1c<F, 0>(x0, x2, ct), a1 = fold1c<F, 0>(x1, x3, ct);
    const Fe s0 = fold1c<F, 0>(z0, z2, ct), s1 = fold1c<F, 0>(z1, z3, ct);
    st_fe(X2, j, a0);
    st_fe(X2, j + h, a1);
    st_fe(Z2, j, s0);
    st_fe(Z2, j + h, s1);
    wide_mac<F>(w0, a0, s0);
    wide_mac<F>(w2, at2<F>(a0, a1), at2<F>(s0, s1));
  }
  ZK_STAMP_AFTER(1, w0);
  ZK_STAMP_AFTER(2, w2);
  __shared__ LimbScratch<17> sc;
  block_limb_sums(w0, sc, 0);
  block_limb_sums(w2, sc, 17);
  __syncthreads();
  ZK_STAMP(3);
  grid_finish<34>(sc, sink);
}

// ---------------------------------------------------------------------------
// Same round as k_gkr_round for SMALL tables, where a thread-per-pair kernel is
// latency-bound (one wave serialises 12 dependent 256-bit multiplies). Here 8
// lanes share a pair: lane s folds table s>>1, half s&1 (one multiply); odd
// lanes turn (lo, hi) into X(2) = 2 hi - lo; lanes {0,1,4,5} multiply with lane
// s+2 (A*S / M*P at t = 0 and t = 2), accumulated unreduced. Critical path:
// one multiply + one unreduced product.
// ---------------------------------------------------------------------------
__device__ __forceinline__ Fe shfl_fe(const Fe& x, int src) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = __shfl(x.v[i], src, 64);
  return r;
}
// The step over h pairs by nb blocks: this lane's table X (4h elements, table
// (threadIdx & 7) >> 1 of A, S, M, P) folds by r into Y (2h). Returns the
// lane's unreduced product sum: lanes 0,4 of a group the t = 0 products,
// lanes 1,5 the t = 2 products, the others unused.
template <class F, class Io>
__device__ __forceinline__ Wide lanes_pairs(const Fe* __restrict__ X, Fe* __restrict__ Y, uint64_t h, const Fe& r,
                                            uint32_t nb) {
  const uint32_t lane = threadIdx.x & 63, half = threadIdx.x & 1;
  Wide acc = wide_zero<F>();
  const uint64_t stride = (uint64_t)nb * (kBlock / 8);
  // the loop bound is uniform per 8-lane group (and per wave: 8 groups share j's stride)
  for (uint64_t j = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 3; j < h; j += stride) {
    const uint64_t o = j + half * h;
    const Fe f = fold1<F>(Io::ld(X, o), Io::ld(X, o + 2 * h), r);
    Io::st(Y, o, f);
    const Fe lo = shfl_fe(f, (int)(lane & ~1u));        // the group's lo for this table
    const Fe v = half ? at2<F>(lo, f) : f;               // even: X(0), odd: X(2)
    const Fe partner = shfl_fe(v, (int)((lane + 2) & 63));
    wide_mac<F>(acc, v, partner);
  }
  return acc;
}
// the block's limb sums of those products: e0 -> sc.tot[0..17), e2 -> sc.tot[17..34)
template <class F>
__device__ __forceinline__ void lanes_limb_sums(const Wide& acc, LimbScratch<17>& sc) {
  const uint32_t s = threadIdx.x & 7, half = s & 1;
  const bool mine = (s & 2u) == 0;  // s in {0, 1, 4, 5}: the product lanes
  const Wide z = wide_zero<F>();
  block_limb_sums(mine && half == 0 ? acc : z, sc, 0);
  block_limb_sums(mine && half == 1 ? acc : z, sc, 17);
  __syncthreads();
}

template <class F>
__global__ __launch_bounds__(kBlock) void k_gkr_round_lanes(const Fe* __restrict__ A, const Fe* __restrict__ S,
                                                            const Fe* __restrict__ M, const Fe* __restrict__ P,
                                                            Fe* __restrict__ A2, Fe* __restrict__ S2,
                                                            Fe* __restrict__ M2, Fe* __restrict__ P2, uint64_t h,
                                                            RoundIn rin, RoundSink sink) {
  ZK_STAMP(0);
  const Fe r = block_get_r(rin);
  const uint32_t tb = (threadIdx.x & 7) >> 1;
  const Fe* __restrict__ X = tb == 0 ? A : tb == 1 ? S : tb == 2 ? M : P;
  Fe* __restrict__ Y = tb == 0 ? A2 : tb == 1 ? S2 : tb == 2 ? M2 : P2;
  const Wide acc = lanes_pairs<F, PlainIo>(X, Y, h, r, gridDim.x);
  ZK_STAMP(1);
  ZK_STAMP(2);
  __shared__ LimbScratch<17> sc;
  lanes_limb_sums<F>(acc, sc);
  ZK_STAMP(3);
  grid_finish<34>(sc, sink);
}

// ---------------------------------------------------------------------------
// The tail of a GKR proof in ONE persistent kernel: the last `nrounds` rounds
// (pairs h0, h0/2, ..., each round the k_gkr_round_lanes step) without a
// kernel boundary between them. Per round, block 0 waits for the host-posted
// challenge (tag rtag0 + m) and relays it; the active blocks fold and
// evaluate; their limb sums meet in the u64 accumulator; the last block
// publishes them (sink tag tag0 + m) and the host answers with the next
// challenge. What a boundary cost each small round — dispatch, the end-of-
// kernel cache write-back, a cold instruction cache for the 256-bit multiply
// code — is paid once.
//
// Inter-block data (the folded tables of round m, read by other blocks in
// round m + 1) follows the guide's 8-byte agent-atomics form on both sides
// (MI355X_MICROARCH.md "Valid forms"): every store and every load of those
// bytes is a relaxed agent-scope 8-B atomic (sc1), every storing wave drains
// (vmcnt(0)) before its block's counter add, and a consumer only loads after
// the relayed challenge, which the host posts after the last block's publish.
// Each round writes a fresh region (no address is rewritten in the kernel), so
// no L2 can hold an older copy of a line it reads. The relay is one fresh
// 64-B slot per round for the same reason. Active blocks per round are
// min(gridDim, ceil(8h / kBlock)), non-increasing, so a block that is idle
// in a round exits; every wait gives up after ~1 s like block_get_r.
// ---------------------------------------------------------------------------
struct TailArgs {
  const Fe* in[4];    // tables of the round before the first tail round (4 h0 elements each)
  Fe* out;            // fresh regions: round m writes 4 tables of 2 (h0 >> m) at out + 8 (h0 - (h0 >> m))
  uint64_t h0;        // pairs in the first tail round
  uint32_t nrounds;   // tail rounds
  uint32_t rtag0;     // challenge tag awaited by round 0
  const RWait* host;  // pinned challenge slot
  RWait* relay;       // nrounds fresh 64-B relay slots
  uint32_t* err;      // pinned error word
  uint64_t* trace;    // debug (ZK_DEBUG_TAIL): per round 8 s_memrealtime stamps, or null
};
// slot i of step m's trace row in a persistent kernel with arguments `a`
// (TailArgs / DTailArgs; tools/trace_print.py names the slots)
#define ZK_TAIL_STAMP(m, i) \
  do { if (a.trace) a.trace[(m) * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)

template <class F>
__global__ __launch_bounds__(kBlock) void k_gkr_tail(TailArgs a, RoundSink sink) {
  __shared__ LimbScratch<17> sc;
  const uint32_t tb = (threadIdx.x & 7) >> 1;
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  for (uint32_t m = 0; m < a.nrounds; ++m) {
    const uint64_t h = a.h0 >> m;
    const uint64_t want = (8 * h + kBlock - 1) / kBlock;
    const uint32_t nb = want < gridDim.x ? (uint32_t)want : gridDim.x;
    if (blockIdx.x >= nb) return;  // idle from here on (nb never grows)
    // ---- challenge r_{k-1}: block 0 polls the host, the others this round's relay slot ----
    if (lead) ZK_TAIL_STAMP(m, 0);
    const Fe r = block_wait_r(a.host, a.relay + m, nb > 1, a.rtag0 + m, a.err);
    if (lead) ZK_TAIL_STAMP(m, 1);
    // ---- fold by r and evaluate e0, e2 (the k_gkr_round_lanes step) ----
    const Fe* X;
    if (m == 0) {
      X = a.in[tb];
    } else {
      X = a.out + tail_region(a.h0, m - 1) + (uint64_t)tb * 4 * h;  // previous round: 4 tables of 4h
    }
    Fe* Y = a.out + tail_region(a.h0, m) + (uint64_t)tb * 2 * h;
    const Wide acc = lanes_pairs<F, AgentIo>(X, Y, h, r, nb);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's table stores have landed
    if (lead) ZK_TAIL_STAMP(m, 2);
    lanes_limb_sums<F>(acc, sc);
    // ---- fan-in over the nb active blocks, publish ----
    RoundSink sk = sink;
    sk.tag = sink.tag + m;
    if (nb == 1 || atomic_fan_in<34>(sc, sk, nb)) {
      if (threadIdx.x == 0) ZK_TAIL_STAMP(m, 3);
      publish_limbs<34>(sc, sk);
      if (threadIdx.x == 0) ZK_TAIL_STAMP(m, 4);
    }
    __syncthreads();  // sc and the challenge's LDS copy are reused next round
  }
}

// ---------------------------------------------------------------------------
// Two rounds per kernel ("double round"). The tables of every other level are
// never materialised: the kernel applies the NP pending challenges of the
// previous step (NP = 2: r_{m-2}, r_{m-1} by one fold2 per output; NP = 1:
// r_{m-1}) to the input tables (size 4 NP Q) and writes the level-m tables Z
// (size 4Q: index bit 2Q = variable m, bit Q = variable m+1). A quad j < Q
// holds the corners V(a,b) = Z[j + (2a + b) Q] of a bilinear function of
// (x_m, x_{m+1}); extended to a, b in {0,1,2} (V(2,b) = 2V(1,b) - V(0,b),
// V(a,2) = 2V(a,1) - V(a,0)) it gives every value either round needs:
//   round m:    e0 = sum V(0,0)^2 + V(0,1)^2,  e2 = sum V(2,0)^2 + V(2,1)^2
//               (sum_check_protocol.rs:152-166 on the folded tables);
//   round m+1:  with r_m still unknown, folding by r gives lo = V(r,0),
//               X(2) = V(r,2), so e0'(r) and e2'(r) are quadratics in r given
//               by their values at r = 0, 1, 2: V(.,0)^2 and V(.,2)^2.
// ("V^2" = the A-side value times the S-side value, plus M times P.) That is
// the 3x3 grid without its centre: 8 product sums. A quad of one product
// (A*S or M*P) is a unit of 8 lanes, 4 tab + k: lane k of table tab computes
// corner k (one fold per lane) and forms, by quad_perm DPP moves (no LDS, no
// barrier), its two grid points:
//   k = 0 (0,0): V(0,0), V(2,2)     k = 1 (0,1): V(0,1), V(0,2)
//   k = 2 (1,0): V(1,0), V(2,0)     k = 3 (1,1): V(2,1), V(1,2)
// then trades one point with its partner in the other table (lane ^ 4) and
// multiplies slot tab + 1. Category c = 2k + slot: 0 V00, 1 V22, 2 V01,
// 3 V02, 4 V10, 5 V20, 6 V21, 7 V12 (limb sums of values in [0, p): exact). The host finishes round m,
// draws r_m, interpolates round m+1's values at r_m, draws r_{m+1} and posts
// (r_m, r_{m+1}, r_m r_{m+1}): one hand-off and one kernel per two rounds.
//
// Challenges arrive as 24 self-tagged words (tag << 32 | limb of ra, rb, rab):
// one load per lane polls and reads them at once, block 0 relays the same
// words; a word is valid when its tag is >= the awaited one, so no ordering
// between the words is needed.
// ---------------------------------------------------------------------------
struct alignas(64) RPost {
  // ra, rb, rab in words 0-23 (the device-FS tail also the digest, 24-31, and
  // the claim, 32-39); a fold by three reads the eight eq weights, words 0-63
  uint64_t w[64];
};
struct DIn {
  Fe ra, rb, rab;      // used as is when host == null
  const RPost* host;   // pinned slot the host posts to, or null
  RPost* relay;        // device relay slot (used when gridDim > 1)
  uint32_t* err;       // pinned error word
  uint32_t tag;
};
// NV tagged values (8 words each) into s_w[8 NV] (LDS; valid after the barrier).
// Block 0 polls the host slot and copies the words to the device relay when
// `relay`; the other blocks poll the relay. dev_only: every block polls the
// relay, which a previous step's device-side Fiat-Shamir wrote (dfs.hpp).
template <int NV>
__device__ __forceinline__ void block_get_words(const DIn& in, uint32_t* s_w, bool relay, bool dev_only) {
  if (threadIdx.x < 64) {  // wave 0
    const uint32_t lane = threadIdx.x;
    const bool mine = lane < 8 * NV;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    const bool direct = blockIdx.x == 0 && !dev_only;
    uint64_t v = 0;
    bool ok = true;
    while (true) {
      if (mine)
        v = direct ? __hip_atomic_load(&in.host->w[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                   : __hip_atomic_load(&in.relay->w[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool ready = !mine || (int32_t)((uint32_t)(v >> 32) - in.tag) >= 0;
      if (__all(ready)) break;
      if (direct) __builtin_amdgcn_s_sleep(2); else __builtin_amdgcn_s_sleep(1);
      if (__builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) { ok = false; break; }
    }
    if (direct && relay && mine) __hip_atomic_store(&in.relay->w[lane], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ok && lane == 0) __hip_atomic_store(in.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (mine) s_w[lane] = (uint32_t)v;
  }
  __syncthreads();
}
__device__ __forceinline__ void block_get_rs(const DIn& in, Fe& ra, Fe& rb, Fe& rab, bool relay) {
  if (!in.host) {
    ra = in.ra;
    rb = in.rb;
    rab = in.rab;
    return;
  }
  __shared__ uint32_t s_w[24];
  block_get_words<3>(in, s_w, relay, false);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ra.v[i] = s_w[i];
    rb.v[i] = s_w[8 + i];
    rab.v[i] = s_w[16 + i];
  }
}

// The eight eq weights eq((ra, rb, rc), c), c = 4a + 2b + c0, of a fold by the
// three pending challenges (k_gkr_t33, k_gkr_dm3) into eqw[0..7] (LDS; valid
// after the caller's next barrier): a pre-enqueued step reads them as posted by
// the host (64 tagged words: two dependent Montgomery products per weight off
// the step's critical path), a step launched after its challenges forms them
// from din's (ra, rb, rab = rc).
template <class F>
__device__ __forceinline__ void block_get_eq8(const DIn& in, Fe* eqw, bool relay) {
  const uint32_t t = threadIdx.x;
  if (in.host) {
    __shared__ uint32_t s_w[64];
    block_get_words<8>(in, s_w, relay, false);
    if (t < 8) {
#pragma unroll
      for (int i = 0; i < 8; ++i) eqw[t].v[i] = s_w[8 * t + i];
    }
  } else if (t < 8) {
    const Fe one = fe_one<F>();
    const Fe fa = (t & 4) ? in.ra : fe_sub<F>(one, in.ra), fb = (t & 2) ? in.rb : fe_sub<F>(one, in.rb);
    const Fe fc = (t & 1) ? in.rab : fe_sub<F>(one, in.rab);
    eqw[t] = fe_mul<F>(fe_mul<F>(fa, fb), fc);
  }
}

constexpr int kDCats = 8;             // product-sum categories of a double round
constexpr int kDLimbs = kDCats * 17;  // 136 limb sums
constexpr uint32_t kDQuads = 16;      // quads per block iteration (8 lanes each: 2 tables x 4 corners, 2 products)
struct DScratch {
  uint32_t rows[kBlock * 17];  // limb-sum transpose: 17 words per thread (odd stride)
  uint64_t tot[kSlotU64];
  uint64_t pp[kBlock];
  uint32_t am_last;
};
// quad_perm DPP move of a field element: lane 4i + k reads lane 4i + perm[k]
template <int CTRL>
__device__ __forceinline__ Fe dpp_fe(const Fe& x) {
  Fe r;
#pragma unroll
  for (int w = 0; w < 8; ++w) r.v[w] = (uint32_t)__builtin_amdgcn_mov_dpp((int)x.v[w], CTRL, 0xF, 0xF, false);
  return r;
}
// lane i reads lane i ^ 4 (ds_swizzle bit mode: and 0x1F, xor 4; no LDS memory)
__device__ __forceinline__ Fe xor4_fe(const Fe& x) {
  Fe r;
#pragma unroll
  for (int w = 0; w < 8; ++w) r.v[w] = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x.v[w], 0x101F);
  return r;
}
__device__ __forceinline__ Fe sel_fe(bool c, const Fe& a, const Fe& b) {
  Fe r;
#pragma unroll
  for (int w = 0; w < 8; ++w) r.v[w] = c ? a.v[w] : b.v[w];
  return r;
}
constexpr int kQP0001 = 0x40, kQP3333 = 0xFF, kQP2222 = 0xAA;  // quad_perm [0,0,0,1], [3,3,3,3], [2,2,2,2]
// corner q of lane k -> (slot 1, slot 2) points (see the table above)
template <class F>
__device__ __forceinline__ void grid_points(const Fe& q, uint32_t k, Fe& s1, Fe& s2) {
  const Fe e1 = at2<F>(dpp_fe<kQP0001>(q), q);  // k=1: V02, k=2: V20, k=3: V21
  const Fe xa = dpp_fe<kQP3333>(e1), ya = dpp_fe<kQP2222>(e1), yb = dpp_fe<kQP2222>(q);
  const Fe e2 = at2<F>(sel_fe(k == 0, ya, yb), sel_fe(k == 0, xa, q));  // k=0: V22, k=3: V12
  s1 = sel_fe(k == 3, e1, q);
  s2 = sel_fe(k == 0 || k == 3, e2, e1);
}
// One quad-product unit = 8 lanes: lane u = 4 tab + k holds corner k of table
// tab (A or M for tab 0, S or P for tab 1). After grid_points each lane owns
// the product of slot tab + 1: it sends the other slot's point to its partner
// lane (u ^ 4) and multiplies its own point by the partner's. Category of a
// lane: c = 2k + tab.
template <class F>
__device__ __forceinline__ void unit_product(const Fe& z, uint32_t k, uint32_t tab, Wide& acc) {
  Fe s1, s2;
  grid_points<F>(z, k, s1, s2);
  const Fe mine = tab ? s2 : s1;
  const Fe other = xor4_fe(tab ? s1 : s2);
  wide_mac<F>(acc, mine, other);
}
// limb sums of one accumulator per thread: category c = 2k + tab over the
// threads with (lane & 7) == 4 tab + k -> sc.tot[17 c + word] (valid after the call)
__device__ __forceinline__ void dround_limb_sums(const Wide& acc, DScratch& sc) {
#pragma unroll
  for (int w = 0; w < 17; ++w) sc.rows[threadIdx.x * 17 + w] = acc.w[w];
  __syncthreads();
  const uint32_t t = threadIdx.x;
  if (t < (uint32_t)kDLimbs) {
    const uint32_t c = t / 17, w = t % 17, u = 4 * (c & 1) + (c >> 1);
    uint64_t s0 = 0, s1 = 0;
#pragma unroll 8
    for (uint32_t m = 0; m < kBlock / 8; m += 2) {
      s0 += sc.rows[(8 * m + u) * 17 + w];
      s1 += sc.rows[(8 * m + 8 + u) * 17 + w];
    }
    sc.tot[t] = s0 + s1;
  }
  __syncthreads();
}
// A thread's place in a double step. Wave w: product w & 1 (A*S or M*P), quads
// (w >> 1) * 8 + [0, 8) of each kDQuads; lane = 8 unit + 4 tab + k.
struct DLanes {
  uint32_t k, tab, pp, jl;  // corner, table of the product, product, quad of the block's 16
  __device__ __forceinline__ DLanes() {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    k = lane & 3, tab = (lane >> 2) & 1, pp = wv & 1, jl = (wv >> 1) * 8 + (lane >> 3);
  }
  __device__ __forceinline__ uint32_t table() const { return 2 * pp + tab; }  // 0..3: A, S, M, P
  template <class T>
  __device__ __forceinline__ T* pick(T* a, T* s, T* m, T* p) const { return pp ? (tab ? p : m) : (tab ? s : a); }
};
// The step over Q quads by nb blocks: every lane folds its corner of table X
// (4 NP tables' worth: 16 Q or 8 Q elements) by the pending challenges into X2
// (4Q), or, with H2, into the word-major host table (st_fe_sys below), and
// multiplies. two: NP = 2, the fold by (ra, rb) through the constants of
// (ra, rb, ra rb) in ct[30]; else the fold by rb alone, whose constants are
// block 1 of ct[30] or all of ct[10]. Returns the lane's product sum
// (category 2k + tab).
template <class F, class Io, int NC>
__device__ __forceinline__ Wide dstep_quads(const DLanes& L, const Fe* __restrict__ X, Fe* __restrict__ X2, uint64_t* H2,
                                            uint64_t Q, uint32_t nb, bool two, const Fe (&ct)[NC]) {
  static_assert(NC == 30 || NC == 10, "constants of (ra, rb, ra rb) or of rb");
  const uint64_t h4 = 4 * Q;
  Wide acc = wide_zero<F>();
  for (uint64_t jb = (uint64_t)blockIdx.x * kDQuads; jb < Q; jb += (uint64_t)nb * kDQuads) {
    const uint64_t j = jb + L.jl;
    if (j < Q) {  // uniform over the 8 lanes of a unit
      const uint64_t i = j + L.k * Q;
      Fe z;
      if (two) {
        if constexpr (NC == 30) {
          const Fe x00 = Io::ld(X, i), x01 = Io::ld(X, i + h4), x10 = Io::ld(X, i + 2 * h4), x11 = Io::ld(X, i + 3 * h4);
          Io::loads_first();
          z = fold2c<F>(x00, x01, x10, x11, ct);
        }
      } else {
        const Fe x0 = Io::ld(X, i), x1 = Io::ld(X, i + h4);
        Io::loads_first();
        z = fold1c<F, NC == 30 ? 1 : 0>(x0, x1, ct);
      }
      if (H2)
        st_fe_sys(H2, h4, i, z);
      else
        Io::st(X2, i, z);
      unit_product<F>(z, L.k, L.tab, acc);
    }
  }
  return acc;
}

template <class F, int NP>
__global__ __launch_bounds__(kBlock) void k_gkr_dround(const Fe* __restrict__ A, const Fe* __restrict__ S,
                                                       const Fe* __restrict__ M, const Fe* __restrict__ P,
                                                       Fe* __restrict__ A2, Fe* __restrict__ S2,
                                                       Fe* __restrict__ M2, Fe* __restrict__ P2, uint64_t Q,
                                                       DIn din, RoundSink sink) {
  static_assert(NP == 1 || NP == 2, "one or two pending challenges");
  Fe ra, rb, rab;
  if (blockIdx.x == 0) ZK_SINK_STAMP(sink, 0);
  block_get_rs(din, ra, rb, rab, gridDim.x > 1);
  if (blockIdx.x == 0) ZK_SINK_STAMP(sink, 1);
  __shared__ Fe ct[NP == 2 ? 30 : 10];  // fold constants of (ra, rb, ra rb) or rb
  if constexpr (NP == 2)
    fold_consts<F, NP == 2 ? 3 : 1>(ra, rb, rab, ct);
  else
    fold_consts<F, NP == 2 ? 3 : 1>(rb, rb, rb, ct);
  __shared__ DScratch sc;
  const DLanes L;
  const Fe* __restrict__ X = L.pick(A, S, M, P);
  Fe* __restrict__ X2 = L.pick(A2, S2, M2, P2);
  const Wide acc = dstep_quads<F, PlainIo>(L, X, X2, nullptr, Q, gridDim.x, NP == 2, ct);
  dround_limb_sums(acc, sc);
  grid_finish<kDLimbs>(sc, sink);
}

// Rounds 0 and 1 from the input tables in one pass (even round counts,
// k_gkr_d0m in mfma.hpp): nothing to fold, so the quad's corners are the
// inputs themselves; round 0 needs e0, e1, e2 and round 1 the two quadratics
// through V(.,0) and V(.,2) — all nine grid points, the eight of a double step
// plus the corner V11 (category 8). The next step folds the inputs by
// (r_0, r_1) at once.
constexpr int kD0Cats = 9;
constexpr int kD0Limbs = kD0Cats * 17;  // 153 limb sums

// ---------------------------------------------------------------------------
// The small double rounds of a proof in ONE persistent kernel: step s is the
// k_gkr_dround step over Q0 >> 2s quads (two pending challenges, the first
// step np0), run by min(gridDim, Q/16) blocks. The instruction cache stays
// warm and no launch sits between steps; per step block 0 waits for the
// host's three challenges (tag rtag0 + s) and relays them through a fresh
// slot, the active blocks fold and evaluate, their 136 limb sums meet in the
// u64 accumulator (<= 64 blocks), and the last block publishes (sink tag
// tag0 + s). Tables written in step s are read by other blocks in step s+1:
// every store and load of them is an 8-byte agent-scope atomic (sc1), every
// storing wave drains before its block counts in, and each step writes a
// fresh region (MI355X_MICROARCH.md "Valid forms"), as in k_gkr_tail.
// ---------------------------------------------------------------------------
struct DTailArgs {
  const Fe* in[4];    // input tables of step 0 (4 np0 Q0 elements each)
  Fe* out;            // step s writes 4 tables of 4 (Q0 >> 2s) at out + dtail_region(Q0, s)
  uint64_t Q0;        // quads of step 0
  uint32_t nsteps;
  uint32_t np0;       // pending challenges at step 0 (1 or 2)
  uint32_t rtag0;     // challenge tag awaited by step 0
  const RPost* host;  // pinned challenge words
  RPost* relay;       // nsteps fresh relay slots
  uint32_t* err;      // pinned error word
  uint64_t* trace;    // debug (ZK_DEBUG_TAIL): per step 8 s_memrealtime stamps, or null
  uint64_t* host_tab; // pinned host memory: the last step's 4 output tables (16 Q elements), or null (host-side rounds)
  FsLog* fslog;       // (DFS) pinned: per step but the last, the rounds the device drew (dfs.hpp)
};

// The last device step (host_tab set) stores its output tables to pinned host
// memory instead, with system-scope stores, word-major per table (word k of
// element i at k n + i: one store instruction writes 512 contiguous bytes —
// element-major 8-byte stores crossed the host link one by one, ~20 ns each);
// every storing wave drains (vmcnt(0)) before its block counts in, so the flag
// the last block raises comes after every table store has completed: the host
// runs the remaining rounds on them (host.hpp "host rounds"): st_fe_sys.

// DFS (ZK_DEVICE_FS=1, dfs.hpp): every step but the last draws the next
// step's challenges on the device. The host posts step 0's (ra, rb, rab), the
// transcript digest and the running claim; after each later step's sums the
// block that counts in last runs both rounds' Fiat-Shamir on wave 0 (dfs_double)
// and writes the next step's words to its relay slot (tagged, agent scope),
// which every block polls — no host round trip inside the tail. The host
// replays the logged rounds into its transcript afterwards and compares the
// challenges; the last step publishes its sums as usual.
template <class F, bool DFS>
__global__ __launch_bounds__(kBlock) void k_gkr_dtail(DTailArgs a, RoundSink sink) {
  __shared__ DScratch sc;
  __shared__ Fe ct[30];
  __shared__ uint32_t s_w[kFsWords];  // (DFS) the step's relay words
  const DLanes L;
  const uint32_t tb = L.table();
  const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
  for (uint32_t st = 0; st < a.nsteps; ++st) {
    const uint64_t Q = a.Q0 >> (2 * st);
    const uint64_t want = (Q + kDQuads - 1) / kDQuads;
    const uint32_t nb = want < gridDim.x ? (uint32_t)want : gridDim.x;
    if (blockIdx.x >= nb) {  // idle from here on (nb never grows)
      if (DFS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // a logged step's host stores land before the final flag
      return;
    }
    DIn din{};
    din.host = a.host;
    din.relay = a.relay + st;
    din.err = a.err;
    din.tag = a.rtag0 + st;
    Fe ra, rb, rab;
    if (lead) ZK_TAIL_STAMP(st, 0);
    if constexpr (DFS) {
      block_get_words<kFsWords / 8>(din, s_w, nb > 1, st > 0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        ra.v[i] = s_w[i];
        rb.v[i] = s_w[8 + i];
        rab.v[i] = s_w[16 + i];
      }
    } else {
      block_get_rs(din, ra, rb, rab, nb > 1);
    }
    if (lead) ZK_TAIL_STAMP(st, 1);
    const bool two = st > 0 || a.np0 == 2;
    fold_consts<F, 3>(ra, rb, rab, ct);  // blocks 0, 1, 2: ra, rb, ra rb
    if (lead) ZK_TAIL_STAMP(st, 6);
    const Fe* X;
    if (st == 0) {
      X = a.in[tb];
    } else {
      const Fe* prev = a.out + dtail_region(a.Q0, st - 1);  // 4 tables of 16 Q
      X = prev + (uint64_t)tb * 16 * Q;
    }
    Fe* X2 = a.out + dtail_region(a.Q0, st) + (uint64_t)tb * 4 * Q;
    uint64_t* H2 = a.host_tab && st + 1 == a.nsteps ? a.host_tab + (uint64_t)tb * 16 * Q : nullptr;
    const Wide acc = dstep_quads<F, AgentIo>(L, X, X2, H2, Q, nb, two, ct);
    if (lead) ZK_TAIL_STAMP(st, 7);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's table stores have landed
    if (lead) ZK_TAIL_STAMP(st, 2);
    dround_limb_sums(acc, sc);
    if (lead) ZK_TAIL_STAMP(st, 3);
    RoundSink sk = sink;
    sk.tag = sink.tag + st;
    const uint32_t t = threadIdx.x;
    // (a single block holds the step's totals in sc.tot already)
    if (nb == 1 || atomic_fan_in<kDLimbs>(sc, sk, nb)) {
      if (t == 0) ZK_TAIL_STAMP(st, 4);
      if (DFS && st + 1 < a.nsteps) {
        __syncthreads();  // sc.tot complete
        if (t < 64) {  // wave 0: both rounds' Fiat-Shamir, then the next step's relay words
          __shared__ DfsScratch dsc;
          Fe claim, rr[3];
          uint32_t dig[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            dig[i] = s_w[24 + i];
            claim.v[i] = s_w[32 + i];
          }
          dfs_double<F>(sc.tot, claim, dig, rr, a.fslog + st, dsc);
          if (t < (uint32_t)kFsWords) {
            const uint32_t q = t & 7, g = t >> 3;
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j)  // (static indices: lane-indexed register arrays would live in scratch)
              if (q == (uint32_t)j)
                v = g == 0 ? rr[0].v[j] : g == 1 ? rr[1].v[j] : g == 2 ? rr[2].v[j] : g == 3 ? dig[j] : claim.v[j];
            __hip_atomic_store(&a.relay[st + 1].w[t], ((uint64_t)(din.tag + 1) << 32) | v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
          }
          if (t == 0) __hip_atomic_store(&a.fslog[st].tag, din.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      } else {
        publish_limbs<kDLimbs>(sc, sk);
      }
      if (t == 0) ZK_TAIL_STAMP(st, 5);
    }
    __syncthreads();  // sc is reused next step
  }
}

// ---------------------------------------------------------------------------
// Plain sum-check round (sum_check_protocol.rs:36-46, :168-175).
// FIRST: s0 = sum X[0,h), s1 = sum X[h,2h) over the input table.
// else : fold the previous table (size 4h) by r into out (size 2h) and sum
//        the folded halves. out must not alias X.
// ---------------------------------------------------------------------------
template <class F, bool FIRST>
__global__ __launch_bounds__(kBlock) void k_sc_round(const Fe* __restrict__ X, Fe* __restrict__ Y, uint64_t h,
                                                     RoundIn rin, RoundSink sink) {
  const Fe r = FIRST ? rin.r : block_get_r(rin);
  Fe acc[2] = {fe_zero<F>(), fe_zero<F>()};
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < h; j += stride) {
    if (FIRST) {
      acc[0] = fe_add<F>(acc[0], ld_fe(X, j));
      acc[1] = fe_add<F>(acc[1], ld_fe(X, j + h));
    } else {
      const Fe x0 = ld_fe(X, j), x1 = ld_fe(X, j + h), x2 = ld_fe(X, j + 2 * h), x3 = ld_fe(X, j + 3 * h);
      const Fe f0 = fold1<F>(x0, x2, r), f1 = fold1<F>(x1, x3, r);
      st_fe(Y, j, f0);
      st_fe(Y, j + h, f1);
      acc[0] = fe_add<F>(acc[0], f0);
      acc[1] = fe_add<F>(acc[1], f1);
    }
  }
  __shared__ LimbScratch<8> sc;
  block_limb_sums(acc[0], sc, 0);
  block_limb_sums(acc[1], sc, 8);
  __syncthreads();
  grid_finish<16>(sc, sink);
}

// ---------------------------------------------------------------------------
// MultilinearPoly::partial_evaluate(bit, r) (:52-63) with pair_points/insert_bit
// (:39-50, :158-164): out[v] = in[lo] + r (in[hi] - in[lo]),
// lo = insert_bit(v, s) (s = nvars-1-bit), hi = lo | 1<<s.  bit 0 -> s = n-1 ->
// lo = v, hi = v + half (contiguous halves).
// ---------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(kBlock) void k_fold(const Fe* __restrict__ X, Fe* __restrict__ Y, uint64_t half,
                                                 uint32_t s, Fe r) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint64_t mask = ((uint64_t)1 << s) - 1;
  for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < half; v += stride) {
    const uint64_t lo = ((v >> s) << (s + 1)) | (v & mask);
    const uint64_t hi = lo | ((uint64_t)1 << s);
    st_fe(Y, v, fold1<F>(ld_fe(X, lo), ld_fe(X, hi), r));
  }
}

// Sharded proofs, after the gather (host.hpp gkr_prove_device): the one-hot
// buffer holds rank g's 4 tables of T elements at [g][table][m]; the global
// table t is indexed m G + g (rank g owns the low index bits g).
template <class F>
__global__ __launch_bounds__(kBlock) void k_interleave(const Fe* __restrict__ in, Fe* __restrict__ out, uint64_t T,
                                                      uint32_t G) {
  const uint64_t n = 4 * (uint64_t)G * T, stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t o = (uint64_t)blockIdx.x * kBlock + threadIdx.x; o < n; o += stride) {
    const uint64_t t = o / (G * T), rem = o % (G * T), m = rem / G, g = rem % G;
    st_fe(out, o, ld_fe(in, (g * 4 + t) * T + m));
  }
}

// fold four tables by r at bit 0 (used before the multi-GPU all-gather)
template <class F>
__global__ __launch_bounds__(kBlock) void k_fold4(const Fe* __restrict__ A, const Fe* __restrict__ S,
                                                  const Fe* __restrict__ M, const Fe* __restrict__ P,
                                                  Fe* __restrict__ A2, Fe* __restrict__ S2, Fe* __restrict__ M2,
                                                  Fe* __restrict__ P2, uint64_t half, Fe r) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t v = (uint64_t)blockIdx.x * kBlock + threadIdx.x; v < half; v += stride) {
    st_fe(A2, v, fold1<F>(ld_fe(A, v), ld_fe(A, v + half), r));
    st_fe(S2, v, fold1<F>(ld_fe(S, v), ld_fe(S, v + half), r));
    st_fe(M2, v, fold1<F>(ld_fe(M, v), ld_fe(M, v + half), r));
    st_fe(P2, v, fold1<F>(ld_fe(P, v), ld_fe(P, v + half), r));
  }
}

// ---------------------------------------------------------------------------
// The table builders on either side of the sum-check (multilinear_polynomial_
// evaluation.rs): element-wise Add / Mul / Sub of two MLEs (:113-151, zip ->
// the shorter length), scale (:93-97: op MUL against the broadcast scalar) and
// tensor_add_mul_polynomials (:99-110: out[i nb + j] = op(a[i], b[j]), which is
// how a GKR layer's S = w_b + w_c and P = w_b * w_c are laid out). Streaming:
// one 32-B store per output, the tensor's operands are L2-resident re-reads.
// ---------------------------------------------------------------------------
enum MleOp : uint32_t { MLE_ADD = 0, MLE_MUL = 1, MLE_SUB = 2 };

template <class F>
__device__ __forceinline__ Fe mle_apply(uint32_t op, const Fe& a, const Fe& b) {
  return op == MLE_ADD ? fe_add<F>(a, b) : op == MLE_MUL ? fe_mul<F>(a, b) : fe_sub<F>(a, b);
}

// Y[i] = op(X[i], Z ? Z[i] : s)
template <class F>
__global__ __launch_bounds__(kBlock) void k_mle_map(const Fe* __restrict__ X, const Fe* __restrict__ Z, Fe s,
                                                    Fe* __restrict__ Y, uint64_t n, uint32_t op) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    st_fe(Y, i, mle_apply<F>(op, ld_fe(X, i), Z ? ld_fe(Z, i) : s));
}

// Y[i << lgb | j] = op(A[i], B[j]) over na << lgb outputs
template <class F>
__global__ __launch_bounds__(kBlock) void k_mle_tensor(const Fe* __restrict__ A, const Fe* __restrict__ B,
                                                       Fe* __restrict__ Y, uint64_t n, uint32_t lgb, uint32_t op) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const uint64_t bm = ((uint64_t)1 << lgb) - 1;
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += stride)
    st_fe(Y, t, mle_apply<F>(op, ld_fe(A, t >> lgb), ld_fe(B, t & bm)));
}

// ---------------------------------------------------------------------------
// canonical <-> Montgomery (in place allowed)
// ---------------------------------------------------------------------------
template <class F, bool TO_MONT>
__global__ __launch_bounds__(kBlock) void k_convert(const Fe* X, Fe* Y, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const Fe x = ld_fe(X, i);
    st_fe(Y, i, TO_MONT ? fe_to_mont<F>(x) : fe_from_mont<F>(x));
  }
}
// flag non-canonical inputs (>= p) so the host can reject them (ark would
// never hold such a value)
template <class F>
__global__ __launch_bounds__(kBlock) void k_check_canonical(const Fe* X, uint64_t n, uint32_t* bad) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  uint32_t b = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    b |= fe_is_canonical<F>(ld_fe(X, i)) ? 0u : 1u;
  if (b) atomicOr(bad, 1u);
}

// ---------------------------------------------------------------------------
// Synthetic tables: limb k of global element i of table t is
// splitmix64(key + 4i + k), key = splitmix64(splitmix64(seed) + t); the
// 256-bit LE value is reduced mod p and stored in Montgomery form.
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
template <class F>
__global__ __launch_bounds__(kBlock) void k_synth(Fe* Y, uint64_t n, uint64_t key, uint64_t index0, uint64_t step) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t m = (uint64_t)blockIdx.x * kBlock + threadIdx.x; m < n; m += stride) {
    const uint64_t i = index0 + m * step;
    Fe x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t w = splitmix64(key + 4 * i + (uint64_t)k);
      x.v[2 * k] = (uint32_t)w;
      x.v[2 * k + 1] = (uint32_t)(w >> 32);
    }
    // value < 2^256 < 6p for every supported p: at most 5 subtractions
#pragma unroll
    for (int t = 0; t < 5; ++t) x = fe_reduce_once<F>(x);
    st_fe(Y, m, fe_to_mont<F>(x));
  }
}

// ---------------------------------------------------------------------------
// GKR layer tables on device. A layer of G gates reads L = 2G
// values w (its inputs). The reference builds the wiring predicate add_i /
// mul_i densely over 2^(3g+2) points (gkr_circuit.rs:39-104) and folds its
// output bits (partial_evaluate / multi_partial_evaluate, scale, add:
// gkr_protocol.rs:243-292); the folded table over (b, c) in [0, L)^2 is
// nonzero only at (2 idx, 2 idx + 1), where it equals
//   weight(idx) = alpha * eq(r_b, idx) + beta * eq(r_c, idx)
// for a gate of that op (eq over the idx field, MSB first; the output layer
// folds one variable with r0: alpha = 1, no beta term). So one streaming pass
// writes all four sum-check tables: A (add wiring), S = w_b + w_c, M (mul
// wiring), P = w_b * w_c at t = i L + j (tensor_add_mul_polynomials order).
// ---------------------------------------------------------------------------
// challenge points passed by value (kernel arguments): no host->device copy
struct LayerPts {
  Fe r[28];  // r_b then r_c, each <= 14 coordinates
};

template <class F>
__global__ __launch_bounds__(kBlock) void k_gate_weights(const LayerPts pts, uint32_t W, Fe alpha, Fe beta,
                                                         uint32_t has_c, uint32_t G, Fe* __restrict__ out) {
  const Fe* rb = pts.r;
  const Fe* rc = pts.r + W;
  const uint32_t idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= G) return;
  const Fe one = fe_one<F>();
  Fe eb = one, ec = one;
  for (uint32_t k = 0; k < W; ++k) {
    const bool bit = (idx >> (W - 1 - k)) & 1u;
    const Fe xb = ld_fe(rb, k);
    eb = fe_mul<F>(eb, bit ? xb : fe_sub<F>(one, xb));
    if (has_c) {
      const Fe xc = ld_fe(rc, k);
      ec = fe_mul<F>(ec, bit ? xc : fe_sub<F>(one, xc));
    }
  }
  Fe wgt = fe_mul<F>(alpha, eb);
  if (has_c) wgt = fe_add<F>(wgt, fe_mul<F>(beta, ec));
  st_fe(out, idx, wgt);
}

template <class F>
__global__ __launch_bounds__(kBlock) void k_layer_tables(const Fe* __restrict__ w, uint32_t lgL,
                                                         const Fe* __restrict__ wt, const uint8_t* __restrict__ ops,
                                                         Fe* __restrict__ A, Fe* __restrict__ S, Fe* __restrict__ M,
                                                         Fe* __restrict__ P) {
  const uint64_t T = (uint64_t)1 << (2 * lgL), Lm = ((uint64_t)1 << lgL) - 1;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < T; t += stride) {
    const uint64_t i = t >> lgL, j = t & Lm;
    const Fe wi = ld_fe(w, i), wj = ld_fe(w, j);
    Fe a = fe_zero<F>(), m = fe_zero<F>();
    if ((i & 1) == 0 && j == i + 1) {
      const Fe x = ld_fe(wt, i >> 1);
      if (ops[i >> 1]) m = x;
      else a = x;
    }
    st_fe(A, t, a);
    st_fe(S, t, fe_add<F>(wi, wj));
    st_fe(M, t, m);
    st_fe(P, t, fe_mul<F>(wi, wj));
  }
}

// The same layer sum-check from tables of size L instead of L^2 (two phases,
// the linear-time GKR prover of Thaler / Libra). Variables 0 .. lgL-1 are the
// bits of b (MSB first), lgL .. 2 lgL - 1 those of c. With A(b, c) and M(b, c)
// nonzero only at (2g, 2g+1) and S = w(b) + w(c), P = w(b) w(c):
//   phase 1 (b):  sum_c [A S + M P](b, c) = W(b) U(b) + V(b) 1, with
//     W = w, U(2g) = wt_g (add) or wt_g w(2g+1) (mul), V(2g) = wt_g w(2g+1)
//     (add), U = V = 0 at odd b;
//   phase 2 (c), b bound to r_b:  A(r_b, 2g+1) = wt_g eq(r_b, 2g) (add),
//     M likewise (mul), S = w(r_b) + w(c), P = w(r_b) w(c).
// Every table is linear in the variable being folded, so each round's e0, e1,
// e2 equal the dense tables' (the same field values, hence the same proof).
template <class F>
__global__ __launch_bounds__(kBlock) void k_phase1_tables(const Fe* __restrict__ w, const Fe* __restrict__ wt,
                                                          const uint8_t* __restrict__ ops, uint32_t L,
                                                          Fe* __restrict__ W, Fe* __restrict__ U,
                                                          Fe* __restrict__ V, Fe* __restrict__ ONE) {
  const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= L) return;
  const Fe wb = ld_fe(w, b);
  Fe u = fe_zero<F>(), v = fe_zero<F>();
  if ((b & 1u) == 0) {
    const Fe x = ld_fe(wt, b >> 1), xw = fe_mul<F>(x, ld_fe(w, b + 1));
    if (ops[b >> 1]) {
      u = xw;
    } else {
      u = x;
      v = xw;
    }
  }
  st_fe(W, b, wb);
  st_fe(U, b, u);
  st_fe(V, b, v);
  st_fe(ONE, b, fe_one<F>());
}

template <class F>
__global__ __launch_bounds__(kBlock) void k_phase2_tables(const Fe* __restrict__ w, const Fe* __restrict__ wt,
                                                          const uint8_t* __restrict__ ops, uint32_t lgL,
                                                          const LayerPts rb /* lgL coordinates */, Fe wrb,
                                                          Fe* __restrict__ A, Fe* __restrict__ S,
                                                          Fe* __restrict__ M, Fe* __restrict__ P) {
  const uint32_t L = 1u << lgL, c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= L) return;
  const Fe wc = ld_fe(w, c);
  Fe a = fe_zero<F>(), m = fe_zero<F>();
  if (c & 1u) {
    const uint32_t b = c - 1;  // the gate's left input
    const Fe one = fe_one<F>();
    Fe e = ld_fe(wt, b >> 1);
    for (uint32_t k = 0; k < lgL; ++k) {
      const Fe rk = rb.r[k];
      e = fe_mul<F>(e, ((b >> (lgL - 1 - k)) & 1u) ? rk : fe_sub<F>(one, rk));
    }
    if (ops[b >> 1]) m = e;
    else a = e;
  }
  st_fe(A, c, a);
  st_fe(S, c, fe_add<F>(wrb, wc));
  st_fe(M, c, m);
  st_fe(P, c, fe_mul<F>(wrb, wc));
}

// Both evaluations w.evaluate(r_b), w.evaluate(r_c) of a layer's input table
// (gkr_protocol.rs:75-76) in one pass. evaluate folds variable 0 (the MSB)
// first, so w(r) = sum_j w[j] eq(r, j) with eq MSB-first; eq splits into the
// top and bottom halves of the index bits, eq(r, j) = E_hi[j_hi] E_lo[j_lo].
// Every block builds the four half tables in LDS, each thread accumulates
// w[j] E_hi E_lo unreduced, and the two sums leave through the integer
// epilogue (K = 2 product sums of 17 limbs). n <= 14.
template <class F>
__global__ __launch_bounds__(kBlock) void k_mle_eval2(const Fe* __restrict__ w, uint32_t n,
                                                      const LayerPts pr /* r_b[n], r_c[n] */, RoundSink sink) {
  constexpr uint32_t kHalf = 128;
  __shared__ Fe tab[4][kHalf];  // r_b hi, r_b lo, r_c hi, r_c lo
  __shared__ Fe pts[28];
  if (threadIdx.x == 0)
    for (uint32_t k = 0; k < 2 * n; ++k) pts[k] = pr.r[k];  // uniform index: scalar loads of the arguments
  __syncthreads();
  const uint32_t nl = n / 2, nhi = n - nl;
  const Fe one = fe_one<F>();
  for (uint32_t t = threadIdx.x; t < 4 * kHalf; t += kBlock) {
    const uint32_t which = t / kHalf, x = t % kHalf, hi = (which & 1u) == 0;
    const uint32_t bits = hi ? nhi : nl, off = (which >> 1) * n + (hi ? 0 : nhi);
    if (x >= (1u << bits)) continue;
    Fe e = one;
    for (uint32_t k = 0; k < bits; ++k) {
      const Fe rk = pts[off + k];
      e = fe_mul<F>(e, ((x >> (bits - 1 - k)) & 1u) ? rk : fe_sub<F>(one, rk));
    }
    tab[which][x] = e;
  }
  __syncthreads();
  Wide a0 = wide_zero<F>(), a1 = wide_zero<F>();
  const uint64_t N = (uint64_t)1 << n, stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < N; j += stride) {
    const uint32_t x = (uint32_t)(j >> nl), y = (uint32_t)(j & ((1u << nl) - 1u));
    const Fe wj = ld_fe(w, j);
    wide_mac<F>(a0, fe_mul<F>(wj, tab[0][x]), tab[1][y]);
    wide_mac<F>(a1, fe_mul<F>(wj, tab[2][x]), tab[3][y]);
  }
  __shared__ LimbScratch<17> sc;
  block_limb_sums(a0, sc, 0);
  block_limb_sums(a1, sc, 17);
  __syncthreads();
  grid_finish<34>(sc, sink);
}

// one circuit layer (gkr_circuit.rs:127-143): out[g] = in[2g] op in[2g+1]
template <class F>
__global__ __launch_bounds__(kBlock) void k_circuit_layer(const Fe* __restrict__ in, const uint8_t* __restrict__ ops,
                                                          uint32_t G, Fe* __restrict__ out) {
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= G) return;
  const Fe a = ld_fe(in, 2 * (uint64_t)g), b = ld_fe(in, 2 * (uint64_t)g + 1);
  st_fe(out, g, ops[g] ? fe_mul<F>(a, b) : fe_add<F>(a, b));
}

}  // namespace zk
