// The step schedule of a GKR sum-check phase as a pure function of a few
// knobs (no HIP, no zk_ctx): compiled into the library through host.hpp and,
// on the CPU alone, into tests/native/gkr_plan_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define ZK_PLAN_HD __host__ __device__ __forceinline__
#else
#define ZK_PLAN_HD static inline
#endif

namespace zk {
// Table regions of the persistent kernels (elements before round m / step s):
// k_gkr_tail's round m writes 4 tables of 2 (h0 >> m), k_gkr_dtail's step s 4
// tables of 4 (Q0 >> 2s).
ZK_PLAN_HD uint64_t tail_region(uint64_t h0, uint32_t m) { return 8 * (h0 - (h0 >> m)); }
ZK_PLAN_HD uint64_t dtail_region(uint64_t Q0, uint32_t s) {
  uint64_t o = 0;
  for (uint32_t t = 0; t < s; ++t) o += 16 * (Q0 >> (2 * t));
  return o;
}
}  // namespace zk

namespace zkh {
struct GStep {
  int kind;        // GS_*
  uint32_t i;      // first round (local)
  int np;          // double / dtail: pending challenges at entry (1 or 2)
  uint32_t nd = 0; // dtail: double steps it runs
  bool dfs = false;  // dtail: device-side Fiat-Shamir between its steps (ZK_DEVICE_FS)
};
enum {
  GS_ROUND0 = 0, GS_SINGLE = 1, GS_DOUBLE = 2, GS_TAIL = 3, GS_DTAIL = 4, GS_D0 = 5, GS_D0T = 6, GS_T32 = 7, GS_T33 = 8,
  GS_HOST = 11   // the last rounds on the host, from the tables the persistent tail's last step hands over
};
inline uint32_t rounds_of(const GStep& st, uint32_t nv) {
  switch (st.kind) {
    case GS_DOUBLE: case GS_D0: case GS_T32: return 2;
    case GS_D0T: case GS_T33: return 3;
    case GS_DTAIL: return 2 * st.nd;
    case GS_TAIL: case GS_HOST: return nv - st.i;
    default: return 1;
  }
}

// What the schedule reads (host.hpp plan_knobs fills it from the context).
struct PlanKnobs {
  bool pre = true;          // steps are pre-enqueued (host.hpp prelaunch())
  bool dround = true, d0 = true, d0t = true, dtail = true;  // ZK_DROUND, ZK_D0 > 0, ZK_D0T, ZK_DTAIL
  bool use_tail = true;     // persistent kernels allowed (host.hpp use_tail())
  bool cross_ranks = false; // the steps' sums are reduced over ranks
  bool device_fs = false;   // ZK_DEVICE_FS
  uint64_t dtail_max_quads = 1u << 10, tail_max_pairs = 1u << 15;
  uint32_t host_rounds = 4;
  uint32_t num_cus = 256, t33_oct64_min = 1, mall_order = 0;  // the input pass's chunk order
};

struct PhasePlan {
  std::vector<GStep> steps;
  uint32_t stop = 0;         // rounds this phase runs (nv unless cut at the gather boundary)
  uint32_t host_rounds = 0;  // the last this many of them on the host
  uint32_t d0t_order = 0;    // chunk order of the input pass (ZK_MALL_ORDER)
  uint64_t tail_elems = 0;   // table regions of the persistent kernel after its relay slots (0: no such step)
  size_t host_tab_bytes = 0; // the tables handed to the host rounds
  bool fslog = false;        // the device-FS log is needed
  const char* error = nullptr;  // set: the schedule is unusable (an internal error)
};

// The steps of `nv` rounds over tables of 2^nv elements.
// host_ok: the caller does not need the final tables, so the last rounds may
// run on the host. gather_max > 0 (sharded phases): stop after the first step
// boundary b with nv - b <= gather_max (plan.stop = b).
inline PhasePlan plan_phase(const PlanKnobs& k, uint32_t nv, bool host_ok, uint32_t gather_max) {
  PhasePlan pl;
  std::vector<GStep>& steps = pl.steps;
  const uint64_t L = (uint64_t)1 << nv;
  // rounds 0 and 1 in one pass over the inputs (default; same-box A/B at n = 24:
  // BN254 Fr 1.72-1.74 vs 1.82-1.85 ms, BLS12-381 Fr 1.76 vs 1.83 ms)
  // Three rounds per pass (ZK_D0T, nv >= 11): rounds 0-2 over the inputs
  // (k_gkr_d0t), then nt triple steps that fold by the three pending
  // challenges and run three rounds (k_gkr_t33), one two-round step that
  // folds by three (k_gkr_dm3), and double steps (the small ones in the
  // persistent k_gkr_dtail). nt: the largest count leaving an even number
  // R >= 12 of rounds after the triples, else the smallest leaving an even
  // R >= 8 (every matrix-core step needs >= 64 quads / 32 octants).
  // (Measured and removed: triple steps to the end in a persistent MFMA
  // kernel, and rounds 0-3 in the input pass with a fold by four)
  const bool d0t = k.dround && k.d0t && nv >= 11;
  int nt = -1;
  if (d0t)
    for (int q = 0; 3 + 3 * q + 8 <= (int)nv; ++q) {
      const int R = (int)nv - 3 - 3 * q;
      if (R % 2 == 0 && (R >= 12 || nt < 0)) nt = q;
    }
  const bool d0t_doubles = d0t && nt >= 0;
  const bool d0 = !d0t_doubles && k.dround && k.d0 && nv >= 2 && nv % 2 == 0;
  const bool persistent = k.pre && k.use_tail;
  if (nv >= 1) steps.push_back({d0t_doubles ? GS_D0T : (d0 ? GS_D0 : GS_ROUND0), 0, 0});
  if (d0t_doubles) {
    for (int q = 0; q < nt; ++q) steps.push_back({GS_T33, 3u + 3u * q, 3});
    steps.push_back({GS_T32, 3u + 3u * nt, 3});
  }
  if (k.dround) {
    uint32_t i = d0t_doubles ? 5u + 3u * nt : (d0 ? 2 : 1);
    int np = d0t_doubles || d0 ? 2 : 1;  // challenges pending at the first double step
    if (!d0 && !d0t_doubles) {
      if (nv >= 2) steps.push_back({GS_SINGLE, i++, 0});
      if (nv >= 3 && (nv - 2) % 2 == 1) steps.push_back({GS_SINGLE, i++, 0});
    }
    for (; i + 1 < nv; i += 2, np = 2) steps.push_back({GS_DOUBLE, i, np});
    auto small = [&](const GStep& st) { return st.kind == GS_DOUBLE && (L >> st.i) / 4 <= k.dtail_max_quads; };
    // host rounds: the last H rounds, if they are whole double steps and the
    // persistent tail keeps >= 2 device steps before them
    // (H = ZK_HOST_ROUNDS, or fewer when that leaves the tail < 2 steps: odd
    // round counts at n = 9, 11 take H = 2)
    if (host_ok && persistent && k.dtail && !k.cross_ranks && k.host_rounds >= 2) {
      for (uint32_t H = k.host_rounds & ~1u; H >= 2 && pl.host_rounds == 0; H -= 2) {
        size_t e = steps.size();
        uint32_t got = 0;
        while (got < H && e > 0 && steps[e - 1].kind == GS_DOUBLE && steps[e - 1].np == 2) {
          --e;
          got += 2;
        }
        size_t smalls = 0;  // device double steps left for the persistent tail
        for (size_t q = 0; q < e; ++q) smalls += small(steps[q]);
        if (got == H && smalls >= 2 && e == steps.size() - H / 2) {
          steps.resize(e);
          pl.host_rounds = H;
        }
      }
    }
    // the small doubles (>= 2 of them) in one persistent kernel
    if (persistent && k.dtail) {
      size_t s0 = 0;
      while (s0 < steps.size() && !small(steps[s0])) ++s0;
      const size_t nd = steps.size() - s0;
      if (s0 < steps.size() && nd >= 2 && nd <= 64) {
        const GStep first = steps[s0];
        steps.resize(s0);
        // device-side Fiat-Shamir between the tail's steps: one rank's sums only
        // (a sharded tail's sums are all-reduced on the host between steps)
        const bool dfs = k.device_fs && !k.cross_ranks;
        steps.push_back({GS_DTAIL, first.i, first.np, (uint32_t)nd, dfs});
        pl.fslog = dfs;
        pl.tail_elems = zk::dtail_region((L >> first.i) / 4, (uint32_t)nd);
      }
    }
    if (pl.host_rounds > 0) {
      if (steps.empty() || steps.back().kind != GS_DTAIL) {
        pl.error = "internal: host rounds need the persistent tail";
        return pl;
      }
      pl.host_tab_bytes = (size_t)4 * ((size_t)1 << (pl.host_rounds + 2)) * 32;
      steps.push_back({GS_HOST, nv - pl.host_rounds, 2});
    }
  } else {
    // first round >= 1 with <= tail_max_pairs pairs, if at least two rounds remain
    uint32_t tail0 = nv;
    if (persistent) {
      uint32_t i = 1;
      while (i < nv && (L >> i) / 2 > k.tail_max_pairs) ++i;
      if (i + 2 <= nv && nv - i <= 64) {
        tail0 = i;
        pl.tail_elems = 16 * ((L >> i) / 2);
      }
    }
    for (uint32_t i = 1; i < nv; ++i) {
      if (i == tail0) {
        steps.push_back({GS_TAIL, i, 0});
        break;
      }
      steps.push_back({GS_SINGLE, i, 0});
    }
  }
  pl.stop = nv;
  if (gather_max > 0) {  // sharded: stop at the first boundary leaving <= gather_max rounds (host.hpp gkr_prove_device)
    for (size_t s = 0; s < steps.size(); ++s) {
      const uint32_t b = steps[s].i + rounds_of(steps[s], nv);
      const int kind = steps[s].kind;
      if (kind == GS_TAIL || kind == GS_DTAIL || kind == GS_HOST) break;  // (persistent steps are not cut)
      if (b < nv && nv - b <= gather_max) {
        steps.resize(s + 1);
        pl.stop = b;
        break;
      }
    }
  }
  // the schedule covers rounds 0 .. stop-1 exactly once, in order (checked before anything launches)
  uint32_t next = 0;
  for (const GStep& st : steps) {
    if (st.i != next) {
      pl.error = "internal: step schedule out of order";
      return pl;
    }
    next += rounds_of(st, nv);
  }
  if (next != pl.stop) {
    pl.error = "internal: step schedule does not cover every round";
    return pl;
  }
  // ZK_MALL_ORDER: the input pass groups its chunks by the first 64-octant
  // k_gkr_t33's (16 of its 32-octant chunks per t33 chunk), that t33 takes them
  // in reverse (mfma.hpp k_gkr_d0t / k_gkr_t33 `order`); needs both steps at
  // these positions and the input pass's chunk count a multiple of 16
  const size_t ns = steps.size();
  const bool oct64_3 = (L >> 6) / 64 >= (uint64_t)k.num_cus * k.t33_oct64_min;  // first t33: 64-octant
  const bool oct64_6 = (L >> 9) / 64 >= (uint64_t)k.num_cus * k.t33_oct64_min;  // second t33: 64-octant
  pl.d0t_order = k.mall_order && ns >= 2 && steps[0].kind == GS_D0T && steps[1].kind == GS_T33 &&
                         ((L >> 3) / 32) % 16 == 0 && oct64_3 ? 1u : 0u;
  if (pl.d0t_order && k.mall_order >= 2 && ns >= 3 && steps[2].kind == GS_T33 && oct64_6 && ((L >> 6) / 64) % 8 == 0)
    pl.d0t_order = 2;
  return pl;
}
}  // namespace zkh
