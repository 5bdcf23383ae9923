// The pass plan of a radix-2 NTT of 2^m elements (fft/src/fft.rs dft :6-29 as
// a Stockham autosort, fft.hpp): pure host code, no HIP, compiled on its own by
// tests/native/fft_plan_check.cpp.
//
// The transform runs as P = ceil(m / S) passes; pass p does a_p of the m
// radix-2 stages as one in-tile DFT of R_p = 2^a_p points. With Ns_p the
// product of the radices before it (2^log_ns), pass p
//   reads   x[j + r n/R_p]                       r < R_p, j < n/R_p,
//   scales  by w_n^(r (j mod Ns_p) n/(Ns_p R_p)) (the inter-pass twiddle; pass 0 has none),
//   writes  X[k] to (j / Ns_p) Ns_p R_p + (j mod Ns_p) + k Ns_p.
// Input and output of the whole chain are in natural order; no pass permutes
// on its own.
#pragma once
#include <stdint.h>

#include <vector>

namespace zkh {
// Most radix-2 stages one pass does. A block's tile is 2^(kFftTileLog + 2)
// elements (32 KB): 2^a rows of 2^(kFftTileLog + 2 - a) >= 4 consecutive
// elements, so every run a wave reads or writes is at least 128 bytes.
constexpr uint32_t kFftTileLog = 8;
constexpr uint32_t kFftTileElemsLog = kFftTileLog + 2;
constexpr uint32_t kFftMaxLog = 28;  // ZK_EUNSUPPORTED above (a 2^28 table is 8 GiB)

struct FftPassPlan {
  uint32_t a;       // stages of this pass: its tile DFT has 2^a points
  uint32_t log_ns;  // log2 of the stride of its output digit (sum of the widths before it)
  uint32_t log_c;   // log2 of the consecutive elements per tile row
};

// stages per pass as asked for by ZK_FFT_STAGES (0 / out of range: the default)
inline uint32_t fft_stage_cap(long knob) { return knob >= 1 && knob <= (long)kFftTileLog ? (uint32_t)knob : kFftTileLog; }

// ceil(m / S) passes, widths as even as possible (the wider ones first), all in
// [1, S]; m = 0: no pass (the transform is a copy).
inline std::vector<FftPassPlan> fft_plan(uint32_t m, uint32_t S) {
  std::vector<FftPassPlan> pl;
  if (m == 0) return pl;
  if (S < 1) S = 1;
  if (S > kFftTileLog) S = kFftTileLog;
  const uint32_t P = (m + S - 1) / S, base = m / P, rem = m % P;
  uint32_t ns = 0;
  for (uint32_t p = 0; p < P; ++p) {
    FftPassPlan q;
    q.a = base + (p < rem ? 1 : 0);
    q.log_ns = ns;
    const uint32_t cols = m - q.a;  // log2 of the columns n / R there are
    q.log_c = kFftTileElemsLog - q.a < cols ? kFftTileElemsLog - q.a : cols;
    ns += q.a;
    pl.push_back(q);
  }
  return pl;
}
}  // namespace zkh
