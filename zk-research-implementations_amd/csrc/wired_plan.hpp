// The host-only plan of a wired GKR circuit (no HIP, no zk_ctx): validation
// and caps, the derived shape (table widths, round counts), and per layer the
// two groupings of its gates — by left input and by right input — that the
// phase kernels of wired.hpp gather through. Compiled into the library through
// wired.hip and, on the CPU alone, into tests/native/wired_plan_check.cpp.
//
// A wired circuit lists its layers input -> output. Layer l has gates[l] >= 1
// gates; gate g has an op (0 Add, 1 Mul) and reads wires left, right <
// n_below(l) of the layer below (n_below(0) = ninputs, else gates[l-1]). Nothing
// need be a power of two, left == right is allowed, wires may be unused or
// shared, a layer may be wider than the one below. A layer's value table is
// its inputs zero-padded to 2^kb(l), kb(l) = max(1, ceil log2 n_below(l)); its
// gate index has ka(l) = max(1, ceil log2 gates[l]) = kb(l+1) bits.
//
// Grouping. 256-bit field elements have no atomics, so a phase table is filled
// by gather: the thread that owns table row b walks the gates whose left (phase
// 1) or right (phase 2) input is b. The rows come from a counting sort of the
// gates by that input, O(gates): `start` (CSR offsets), `gate` (the gate ids,
// rows back to back, ascending inside a row). A row's fan-out is unbounded — a
// constant wire can feed every gate — so rows are cut into chunks of at most
// kWiredChunk gates, one thread each: `chunks` = (row, first, count) with
// `first` an offset into `gate`. Rows of one chunk come first (chunks
// [0, nsingle), written straight into the table); the chunks of longer rows
// follow, row by row, and write partial sums into slot (chunk index - nsingle);
// `split` lists those rows as (row, first slot, slots) for the combining pass.
// Field sums are exact, so the cut cannot change a value.
//
// kWiredChunk = 256: the rule for skewed gather lists is to cut those longer
// than a quarter of one wave's share of the work into chunks summed apart;
// at 2^16 gates over ~2^14 resident threads a thread's share is a few
// gates, so any cut in the hundreds bounds the longest thread at a small
// multiple of a layer's launch cost while leaving uniformly wired layers
// (fan-out near 1) untouched. The combining pass gives a split row one block of
// 256 threads, so a row of 2^24 gates is 2^16 slots, 256 per thread.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zkw {
constexpr uint32_t kWiredChunk = 256;       // T: gates one thread walks at most
constexpr uint32_t kWiredMaxLayers = 256;
constexpr uint32_t kWiredMaxWidthLog = 24;  // every gates[l] and ninputs <= 2^24
constexpr uint32_t kWiredMaxGatesLog = 26;  // total gates <= 2^26

// the library's error codes (zk_sumcheck.h), restated so this header stands alone
enum { W_OK = 0, W_EINVAL = 1, W_EUNSUPPORTED = 5 };

inline uint32_t ceil_log2(uint64_t x) {
  uint32_t k = 0;
  while (((uint64_t)1 << k) < x) ++k;
  return k;
}
inline uint32_t vars_of(uint64_t n) {  // max(1, ceil log2 n)
  const uint32_t k = ceil_log2(n);
  return k < 1 ? 1 : k;
}

struct WiredShape {
  uint32_t nlayers = 0, ninputs = 0;
  std::vector<uint32_t> gates, n_below, kb, ka;
  std::vector<size_t> goff;  // first gate of layer l in the concatenated arrays (nlayers + 1)
  uint32_t total_rounds = 0;  // sum of 2 kb(l)
  uint32_t out_vars = 0;      // v = ka(nlayers - 1); the output polynomial has 2^v entries
};

// Shape checks and caps; fills `s`. `*err` names what failed.
inline int wired_shape(uint32_t nlayers, const uint32_t* gates, uint32_t ninputs, WiredShape& s, const char** err) {
  *err = nullptr;
  if (nlayers == 0) return *err = "a wired circuit needs at least one layer", W_EINVAL;
  if (!gates) return *err = "null argument", W_EINVAL;
  if (ninputs == 0) return *err = "a wired circuit needs at least one input", W_EINVAL;
  for (uint32_t l = 0; l < nlayers; ++l)
    if (gates[l] == 0) return *err = "a layer has no gates", W_EINVAL;
  if (nlayers > kWiredMaxLayers) return *err = "more than 256 layers", W_EUNSUPPORTED;
  const uint32_t wmax = 1u << kWiredMaxWidthLog;
  if (ninputs > wmax) return *err = "more than 2^24 inputs", W_EUNSUPPORTED;
  uint64_t total = 0;
  for (uint32_t l = 0; l < nlayers; ++l) {
    if (gates[l] > wmax) return *err = "a layer has more than 2^24 gates", W_EUNSUPPORTED;
    total += gates[l];
  }
  if (total > ((uint64_t)1 << kWiredMaxGatesLog)) return *err = "more than 2^26 gates in all", W_EUNSUPPORTED;
  s = WiredShape{};
  s.nlayers = nlayers;
  s.ninputs = ninputs;
  s.gates.assign(gates, gates + nlayers);
  s.goff.assign(nlayers + 1, 0);
  for (uint32_t l = 0; l < nlayers; ++l) {
    const uint32_t nb = l == 0 ? ninputs : gates[l - 1];
    s.n_below.push_back(nb);
    s.kb.push_back(vars_of(nb));
    s.ka.push_back(vars_of(gates[l]));
    s.goff[l + 1] = s.goff[l] + gates[l];
    s.total_rounds += 2 * s.kb[l];
  }
  s.out_vars = s.ka[nlayers - 1];
  return W_OK;
}

// The wiring itself: ops <= 1, left / right < n_below.
inline int wired_validate(const WiredShape& s, const uint8_t* ops, const uint32_t* left, const uint32_t* right,
                          const char** err) {
  *err = nullptr;
  if (!ops || !left || !right) return *err = "null argument", W_EINVAL;
  for (uint32_t l = 0; l < s.nlayers; ++l)
    for (size_t i = s.goff[l]; i < s.goff[l + 1]; ++i) {
      if (ops[i] > 1) return *err = "gate op must be 0 (add) or 1 (mul)", W_EINVAL;
      if (left[i] >= s.n_below[l] || right[i] >= s.n_below[l])
        return *err = "a gate reads a wire the layer below does not have", W_EINVAL;
    }
  return W_OK;
}

struct WiredChunk {
  uint32_t row, first, count;
};
struct WiredCsr {
  std::vector<uint32_t> start;  // nrows + 1
  std::vector<uint32_t> gate;   // G gate ids, grouped by row
  std::vector<WiredChunk> chunks;
  uint32_t nsingle = 0;           // chunks [0, nsingle) are whole rows
  std::vector<WiredChunk> split;  // (row, first slot, slots) of the rows cut into several chunks
};

// Groups the G gates of a layer by key[g] < nrows (counting sort) and cuts the rows into chunks of <= T.
inline WiredCsr wired_csr(const uint32_t* key, uint32_t G, uint32_t nrows, uint32_t T = kWiredChunk) {
  WiredCsr c;
  c.start.assign((size_t)nrows + 1, 0);
  for (uint32_t g = 0; g < G; ++g) c.start[key[g] + 1] += 1;
  for (uint32_t r = 0; r < nrows; ++r) c.start[r + 1] += c.start[r];
  c.gate.resize(G);
  {
    std::vector<uint32_t> at(c.start.begin(), c.start.end() - 1);
    for (uint32_t g = 0; g < G; ++g) c.gate[at[key[g]]++] = g;
  }
  for (uint32_t r = 0; r < nrows; ++r) {
    const uint32_t n = c.start[r + 1] - c.start[r];
    if (n >= 1 && n <= T) c.chunks.push_back({r, c.start[r], n});
  }
  c.nsingle = (uint32_t)c.chunks.size();
  for (uint32_t r = 0; r < nrows; ++r) {
    const uint32_t n = c.start[r + 1] - c.start[r];
    if (n <= T) continue;
    const uint32_t slot0 = (uint32_t)c.chunks.size() - c.nsingle, k = (n + T - 1) / T;
    for (uint32_t j = 0; j < k; ++j) c.chunks.push_back({r, c.start[r] + j * T, j + 1 < k ? T : n - j * T});
    c.split.push_back({r, slot0, k});
  }
  return c;
}
}  // namespace zkw
