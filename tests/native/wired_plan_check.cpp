// CPU check of csrc/wired_plan.hpp (no HIP, no library): run by
// tests/test_wired_plan_cpu.py, compiled with -fsanitize=address,undefined.
//   wired_plan_check shape <ninputs> <gates...>   prints kb, ka, the round total and v
//   wired_plan_check self                         validation, caps, both groupings, chunking
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "wired_plan.hpp"

using namespace zkw;

static int g_checks = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    ++g_checks;                                                       \
    if (!(cond)) {                                                    \
      fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);      \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)((g_rng >> 11) % n);
}

// The grouping of G gates by key < nrows: a permutation of the gates, every row
// holding exactly its gates in ascending order; chunks of <= T that tile every
// non-empty row exactly, whole rows first; the split list names exactly the
// rows of several chunks with their slots.
static void check_csr(const std::vector<uint32_t>& key, uint32_t nrows, uint32_t T) {
  const uint32_t G = (uint32_t)key.size();
  const WiredCsr c = wired_csr(key.data(), G, nrows, T);
  CHECK(c.start.size() == (size_t)nrows + 1 && c.start[0] == 0 && c.start[nrows] == G);
  CHECK(c.gate.size() == G);
  std::vector<uint32_t> seen(G, 0), fan(nrows, 0);
  for (uint32_t g = 0; g < G; ++g) fan[key[g]] += 1;
  for (uint32_t r = 0; r < nrows; ++r) {
    CHECK(c.start[r + 1] - c.start[r] == fan[r]);
    for (uint32_t i = c.start[r]; i < c.start[r + 1]; ++i) {
      CHECK(c.gate[i] < G && key[c.gate[i]] == r);
      CHECK(i == c.start[r] || c.gate[i - 1] < c.gate[i]);
      seen[c.gate[i]] += 1;
    }
  }
  for (uint32_t g = 0; g < G; ++g) CHECK(seen[g] == 1);
  std::vector<uint32_t> next(c.start.begin(), c.start.end() - 1), nch(nrows, 0);
  CHECK(c.nsingle <= c.chunks.size());
  for (size_t i = 0; i < c.chunks.size(); ++i) {
    const WiredChunk& ch = c.chunks[i];
    CHECK(ch.row < nrows && ch.count >= 1 && ch.count <= T);
    CHECK(ch.first == next[ch.row]);  // the chunks of a row follow each other without gap or overlap
    next[ch.row] += ch.count;
    nch[ch.row] += 1;
    if (i < c.nsingle) CHECK(ch.count == fan[ch.row]);
    else CHECK(fan[ch.row] > T);
  }
  size_t nsplit = 0;
  for (uint32_t r = 0; r < nrows; ++r) {
    CHECK(next[r] == c.start[r + 1]);
    CHECK(nch[r] == (fan[r] + T - 1) / T);
    nsplit += nch[r] > 1;
  }
  CHECK(c.split.size() == nsplit);
  uint32_t slot = 0;
  for (const WiredChunk& s : c.split) {  // (row, first slot, slots), rows ascending, slots back to back
    CHECK(s.row < nrows && s.count == nch[s.row] && s.count > 1 && s.first == slot);
    for (uint32_t j = 0; j < s.count; ++j) CHECK(c.chunks[c.nsingle + s.first + j].row == s.row);
    slot += s.count;
  }
  CHECK(slot == c.chunks.size() - c.nsingle);
}

// rows of fan-out 0, 1, T, T + 1 and one row that takes every remaining gate
static void chunk_edges(uint32_t T) {
  std::vector<uint32_t> key;
  auto add = [&](uint32_t row, uint32_t n) { key.insert(key.end(), n, row); };
  add(1, 1);
  add(2, T);
  add(3, T + 1);
  add(5, 3 * T + 2);
  for (size_t i = key.size(); i > 1; --i) std::swap(key[i - 1], key[rnd((uint32_t)i)]);
  check_csr(key, 7, T);  // rows 0, 4, 6 have no gate
  const WiredCsr c = wired_csr(key.data(), (uint32_t)key.size(), 7, T);
  CHECK(c.nsingle == 2 && c.split.size() == 2 && c.chunks.size() == 2 + 2 + 4);
  std::vector<uint32_t> all(5 * T + 3, 0);  // one wire feeds every gate
  check_csr(all, 1, T);
  const WiredCsr a = wired_csr(all.data(), (uint32_t)all.size(), 1, T);
  CHECK(a.nsingle == 0 && a.split.size() == 1 && a.split[0].count == 6 && a.chunks.back().count == 3);
}

static void self_check() {
  const char* err = nullptr;
  WiredShape s;
  const uint32_t g3[3] = {5, 3, 1};
  CHECK(wired_shape(0, g3, 6, s, &err) == W_EINVAL && err);
  CHECK(wired_shape(3, nullptr, 6, s, &err) == W_EINVAL);
  CHECK(wired_shape(3, g3, 0, s, &err) == W_EINVAL);
  const uint32_t gz[3] = {5, 0, 1};
  CHECK(wired_shape(3, gz, 6, s, &err) == W_EINVAL);
  CHECK(wired_shape(3, g3, 6, s, &err) == W_OK && err == nullptr);
  CHECK(s.kb == (std::vector<uint32_t>{3, 3, 2}) && s.ka == (std::vector<uint32_t>{3, 2, 1}));
  CHECK(s.total_rounds == 16 && s.out_vars == 1 && s.goff == (std::vector<size_t>{0, 5, 8, 9}));
  // the wiring
  const uint8_t ops[9] = {0, 1, 0, 1, 0, 1, 1, 0, 0};
  const uint32_t left[9] = {0, 5, 2, 3, 4, 0, 4, 2, 2}, right[9] = {5, 5, 0, 1, 2, 1, 4, 3, 0};
  CHECK(wired_validate(s, ops, left, right, &err) == W_OK);
  CHECK(wired_validate(s, nullptr, left, right, &err) == W_EINVAL);
  CHECK(wired_validate(s, ops, nullptr, right, &err) == W_EINVAL);
  CHECK(wired_validate(s, ops, left, nullptr, &err) == W_EINVAL);
  for (int i = 0; i < 9; ++i) {
    uint8_t o2[9];
    uint32_t l2[9], r2[9];
    memcpy(o2, ops, sizeof ops);
    memcpy(l2, left, sizeof left);
    memcpy(r2, right, sizeof right);
    o2[i] = 2;
    CHECK(wired_validate(s, o2, left, right, &err) == W_EINVAL);
    const uint32_t nb = i < 5 ? 6 : i < 8 ? 5 : 3;  // the first index the layer below does not have
    l2[i] = nb;
    CHECK(wired_validate(s, ops, l2, right, &err) == W_EINVAL);
    r2[i] = nb;
    CHECK(wired_validate(s, ops, left, r2, &err) == W_EINVAL);
    l2[i] = r2[i] = nb - 1;
    CHECK(wired_validate(s, ops, l2, r2, &err) == W_OK);
  }
  // caps: at them is fine, above them unsupported
  const uint32_t big = 1u << 24;
  const uint32_t one_big[1] = {big}, over[1] = {big + 1};
  CHECK(wired_shape(1, one_big, big, s, &err) == W_OK && s.kb[0] == 24 && s.ka[0] == 24 && s.total_rounds == 48);
  CHECK(wired_shape(1, over, 4, s, &err) == W_EUNSUPPORTED);
  CHECK(wired_shape(1, one_big, big + 1, s, &err) == W_EUNSUPPORTED);
  std::vector<uint32_t> many(257, 1);
  CHECK(wired_shape(256, many.data(), 1, s, &err) == W_OK && s.total_rounds == 512);
  CHECK(wired_shape(257, many.data(), 1, s, &err) == W_EUNSUPPORTED);
  std::vector<uint32_t> four(4, big), five(5, big);
  five[4] = 1;
  CHECK(wired_shape(4, four.data(), 1, s, &err) == W_OK);  // 2^26 gates in all
  CHECK(wired_shape(5, five.data(), 1, s, &err) == W_EUNSUPPORTED);
  // widths of one: padded to one variable
  const uint32_t ones[2] = {1, 1};
  CHECK(wired_shape(2, ones, 1, s, &err) == W_OK && s.kb == (std::vector<uint32_t>{1, 1}) && s.total_rounds == 4);
  // groupings: both keys of the circuit above, random layers, the chunk edges
  check_csr(std::vector<uint32_t>(left, left + 5), 6, kWiredChunk);
  check_csr(std::vector<uint32_t>(right, right + 5), 6, kWiredChunk);
  for (uint32_t T : {1u, 3u, 4u, 256u})
    for (uint32_t rows : {1u, 2u, 7u, 64u, 1000u})
      for (uint32_t G : {1u, 5u, 300u, 4097u}) {
        std::vector<uint32_t> key(G);
        for (auto& k : key) k = rnd(rnd(4) == 0 ? 1 : rows) % rows;  // a quarter of the gates on row 0
        check_csr(key, rows, T);
      }
  chunk_edges(4);
  chunk_edges(kWiredChunk);
  printf("ok %d checks, T=%u\n", g_checks, kWiredChunk);
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "self")) {
    self_check();
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "shape")) {
    std::vector<uint32_t> gates;
    for (int i = 3; i < argc; ++i) gates.push_back((uint32_t)strtoul(argv[i], nullptr, 0));
    WiredShape s;
    const char* err = nullptr;
    const int rc = wired_shape((uint32_t)gates.size(), gates.data(), (uint32_t)strtoul(argv[2], nullptr, 0), s, &err);
    if (rc != W_OK) {
      printf("error=%d %s\n", rc, err);
      return 0;
    }
    printf("total=%u v=%u kb=", s.total_rounds, s.out_vars);
    for (uint32_t k : s.kb) printf("%u,", k);
    printf(" ka=");
    for (uint32_t k : s.ka) printf("%u,", k);
    printf("\n");
    return 0;
  }
  fprintf(stderr, "usage: wired_plan_check self | shape <ninputs> <gates...>\n");
  return 2;
}
