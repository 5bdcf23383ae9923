// Checker for tests/test_r1cs_plan_cpu.py (test infrastructure, not the
// product): drives csrc/r1cs_plan.hpp on the CPU alone, no library loaded.
//   self                 shape validation, the caps and every error; the entry checks; the groupings of an
//                        instance with keys of 0, 1, 255, 256, 257 and 513 entries (single chunk, the cut,
//                        splits into 2 and 3 slots), duplicates and tags; prints "ok chunk=256"
//   digest <field>       an instance on stdin -> its digest as hex
//   transcript <field>   an instance, a witness, io and (flag 1) a commitment's x y on stdin. Runs the whole
//                        prover on the host on a fresh transcript and prints "tau ..", "rx ..", "evals va vb vc",
//                        "rho x", "ry ..", "vw x", "polys1 n c.. | n c.. |", "polys2 ..", "next x" (one more
//                        challenge: the transcript's end state), then verifies its own proof: "verified 1"
// An instance on stdin: nrows sy npub nA nB nC, then per entry "row col value". Field values are canonical hex.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "r1cs_plan.hpp"

using namespace zk;
using namespace zkr;

static void read_words(uint64_t* out, int nwords) {  // one hex integer -> little-endian 64-bit words
  char s[200];
  if (scanf("%199s", s) != 1) exit(2);
  const size_t n = strlen(s);
  for (int i = 0; i < nwords; ++i) out[i] = 0;
  for (size_t i = 0; i < n && i < (size_t)16 * nwords; ++i) {
    const char ch = s[n - 1 - i];
    const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    out[i / 16] |= d << (4 * (i % 16));
  }
}
static uint32_t read_u32() {
  unsigned long v;
  if (scanf("%lu", &v) != 1) exit(2);
  return (uint32_t)v;
}
template <class F>
static Fe read_fe() {
  h64::V v{};
  read_words(v.l, 4);
  return hfe_to_mont<F>(h64::fe(v));
}
template <class F>
static void print_fe(const Fe& m, const char* end) {
  const h64::V o = h64::of(hfe_from_mont<F>(m));
  printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%s", o.l[3], o.l[2], o.l[1], o.l[0], end);
}

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

struct Inst {
  R1csShape sh;
  std::vector<uint32_t> rows, cols;
  std::vector<uint64_t> vals;  // canonical, 4 words per entry
};

static int read_instance(uint32_t field, Inst& in, const char** err) {
  const uint32_t nrows = read_u32(), sy = read_u32(), npub = read_u32();
  uint32_t nnz[3];
  for (auto& x : nnz) x = read_u32();
  const int rc = r1cs_shape(field, nrows, sy, npub, nnz, in.sh, err);
  if (rc) return rc;
  const size_t n = in.sh.total();
  in.rows.resize(n);
  in.cols.resize(n);
  in.vals.resize(4 * n);
  for (size_t e = 0; e < n; ++e) {
    in.rows[e] = read_u32();
    in.cols[e] = read_u32();
    read_words(in.vals.data() + 4 * e, 4);
  }
  return R_OK;
}

static int self_check() {
  using F = Bls12_381Fr;
  const char* err = nullptr;
  R1csShape s;
  const uint32_t n3[3] = {2, 1, 0};
  CHECK(r1cs_shape(2, 5, 4, 3, n3, s, &err) == R_OK && err == nullptr);
  CHECK(s.sx == 3 && s.sy == 4 && s.total() == 3 && s.off[1] == 2 && s.off[2] == 3 && s.matrix_of(1) == 0 &&
        s.matrix_of(2) == 1);
  CHECK(r1cs_shape(0, 1, 1, 0, n3, s, &err) == R_OK && s.sx == 1);             // one constraint: sx is still 1
  CHECK(r1cs_shape(0, 2, 1, 0, n3, s, &err) == R_OK && s.sx == 1);
  CHECK(r1cs_shape(0, 3, 1, 0, n3, s, &err) == R_OK && s.sx == 2);
  CHECK(r1cs_shape(0, 1u << 24, 24, 0, n3, s, &err) == R_OK && s.sx == 24);    // the caps themselves
  CHECK(r1cs_shape(0, 5, 4, 7, n3, s, &err) == R_OK);                          // npub + 1 = 2^(sy-1)
  CHECK(r1cs_shape(0, 5, 4, 8, n3, s, &err) == R_EINVAL && err);
  CHECK(r1cs_shape(0, 5, 1, 1, n3, s, &err) == R_EINVAL);                      // sy = 1 leaves room for the 1 alone
  CHECK(r1cs_shape(0, 0, 4, 0, n3, s, &err) == R_EINVAL && err);
  CHECK(r1cs_shape(0, 5, 0, 0, n3, s, &err) == R_EINVAL && err);
  CHECK(r1cs_shape(3, 5, 4, 0, n3, s, &err) == R_EINVAL && err);
  CHECK(r1cs_shape(0, 5, 4, 0, nullptr, s, &err) == R_EINVAL && err);
  CHECK(r1cs_shape(0, 5, 25, 0, n3, s, &err) == R_EUNSUPPORTED && err);
  CHECK(r1cs_shape(0, (1u << 24) + 1, 4, 0, n3, s, &err) == R_EUNSUPPORTED && err);
  const uint32_t big[3] = {1u << 26, 1, 0}, full[3] = {1u << 25, 1u << 25, 0};
  CHECK(r1cs_shape(0, 5, 4, 0, big, s, &err) == R_EUNSUPPORTED && err);
  CHECK(r1cs_shape(0, 5, 4, 0, full, s, &err) == R_OK);                        // 2^26 entries exactly

  // the entries: ranges and values
  CHECK(r1cs_shape(2, 5, 4, 3, n3, s, &err) == R_OK);
  uint32_t rows[3] = {0, 4, 2}, cols[3] = {15, 0, 7};
  uint64_t vals[12] = {0};
  vals[0] = 1;
  for (int i = 0; i < 4; ++i) vals[4 + i] = h64::P<F>(i);  // p - 1
  vals[4] -= 1;
  std::vector<Fe> vm;
  CHECK(r1cs_entries<F>(s, rows, cols, vals, false, vm, &err) == R_OK && vm.size() == 3);
  CHECK(fe_eq<F>(vm[0], fe_one<F>()) && fe_eq<F>(vm[1], hfe_sub<F>(fe_zero<F>(), fe_one<F>())) && fe_is_zero<F>(vm[2]));
  rows[1] = 5;
  CHECK(r1cs_entries<F>(s, rows, cols, vals, false, vm, &err) == R_EINVAL && err);
  rows[1] = 4;
  cols[2] = 16;
  CHECK(r1cs_entries<F>(s, rows, cols, vals, false, vm, &err) == R_EINVAL && err);
  cols[2] = 7;
  vals[4] += 1;  // p itself
  CHECK(r1cs_entries<F>(s, rows, cols, vals, false, vm, &err) == R_EINVAL && err);
  CHECK(r1cs_entries<F>(s, rows, cols, vals, true, vm, &err) == R_EINVAL);
  vals[4] -= 1;
  CHECK(r1cs_entries<F>(s, nullptr, cols, vals, false, vm, &err) == R_EINVAL);
  CHECK(r1cs_entries<F>(s, rows, cols, nullptr, false, vm, &err) == R_EINVAL);

  // the groupings: keys 10..14 get 1, 255, 256, 257 and 513 entries, both ways; key 0 one duplicate pair
  // in A and the same (row, col) in all three; everything else empty
  const uint32_t sizes[5] = {1, 255, 256, 257, 513};
  std::vector<uint32_t> R[3], Cc[3];
  for (uint32_t k = 0; k < 5; ++k)
    for (uint32_t j = 0; j < sizes[k]; ++j) {
      R[j % 3].push_back(10 + k);  // row 10 + k reads columns 100 + j
      Cc[j % 3].push_back(100 + j);
      R[(j + 1) % 3].push_back(100 + j);  // column 40 + k is read by rows 100 + j
      Cc[(j + 1) % 3].push_back(40 + k);
    }
  R[0].insert(R[0].end(), {0, 0});
  Cc[0].insert(Cc[0].end(), {900, 900});
  for (int t = 0; t < 3; ++t) {
    R[t].push_back(1);
    Cc[t].push_back(901);
  }
  const uint32_t nn[3] = {(uint32_t)R[0].size(), (uint32_t)R[1].size(), (uint32_t)R[2].size()};
  CHECK(r1cs_shape(2, 1000, 10, 0, nn, s, &err) == R_OK && s.sx == 10);
  std::vector<uint32_t> ar, ac;
  for (int t = 0; t < 3; ++t) {
    ar.insert(ar.end(), R[t].begin(), R[t].end());
    ac.insert(ac.end(), Cc[t].begin(), Cc[t].end());
  }
  for (int by_row = 0; by_row < 2; ++by_row) {
    const R1csGroup g = r1cs_group(s, ar.data(), ac.data(), by_row != 0);
    const std::vector<uint32_t>& key = by_row ? ar : ac;
    const std::vector<uint32_t>& oth = by_row ? ac : ar;
    const uint32_t nkeys = by_row ? 1000u : 1024u;
    CHECK(g.csr.start.size() == nkeys + 1 && g.other.size() == ar.size() && g.csr.gate.size() == ar.size());
    std::vector<uint32_t> count(nkeys, 0), seen(ar.size(), 0);
    for (uint32_t k : key) count[k] += 1;
    const uint32_t base = by_row ? 10 : 40;
    for (uint32_t k = 0; k < 5; ++k) CHECK(count[base + k] == sizes[k]);
    CHECK(count[5] == 0);  // a key with no entries has no chunk
    size_t covered = 0;
    uint32_t nsplit_chunks = 0;
    for (size_t ci = 0; ci < g.csr.chunks.size(); ++ci) {
      const zkw::WiredChunk ch = g.csr.chunks[ci];
      CHECK(ch.count >= 1 && ch.count <= zkw::kWiredChunk && ch.row < nkeys && ch.row != 5);
      CHECK((ci < g.csr.nsingle) == (count[ch.row] <= zkw::kWiredChunk));
      if (ci >= g.csr.nsingle) ++nsplit_chunks;
      uint32_t last_tag = 0;
      for (uint32_t i = ch.first; i < ch.first + ch.count; ++i) {
        const uint32_t e = g.csr.gate[i];
        CHECK(key[e] == ch.row && !seen[e]);
        seen[e] = 1;
        CHECK((g.other[i] & kR1csIndexMask) == oth[e] && (g.other[i] >> kR1csTagShift) == s.matrix_of(e));
        CHECK((g.other[i] >> kR1csTagShift) >= last_tag);  // (the sort is stable: A's entries, then B's, then C's)
        last_tag = g.other[i] >> kR1csTagShift;
        ++covered;
      }
    }
    CHECK(covered == ar.size());  // every entry in exactly one chunk
    CHECK(g.csr.split.size() == 2 && nsplit_chunks == 2 + 3);  // 257 -> 2 slots, 513 -> 3
    CHECK(g.csr.split[0].row == base + 3 && g.csr.split[0].first == 0 && g.csr.split[0].count == 2);
    CHECK(g.csr.split[1].row == base + 4 && g.csr.split[1].first == 2 && g.csr.split[1].count == 3);
  }
  // public part and eq on boundary values
  const Fe one = fe_one<F>(), zero = fe_zero<F>(), pm1 = hfe_sub<F>(zero, one);
  const Fe io[2] = {pm1, zkc::fe_small<F>(9)};
  CHECK(fe_eq<F>(r1cs_public_entry<F>(io, 2, 0), one) && fe_eq<F>(r1cs_public_entry<F>(io, 2, 1), pm1) &&
        fe_eq<F>(r1cs_public_entry<F>(io, 2, 2), io[1]) && fe_is_zero<F>(r1cs_public_entry<F>(io, 2, 3)));
  const Fe at2[2] = {one, zero};  // the hypercube point 2 = (1, 0): entry 2
  CHECK(fe_eq<F>(r1cs_public_eval<F>(io, 2, at2, 2), io[1]));
  CHECK(fe_eq<F>(r1cs_public_eval<F>(io, 0, nullptr, 0), one));
  CHECK(fe_eq<F>(r1cs_eq_eval<F>(at2, at2, 2), one) && fe_eq<F>(r1cs_eq_eval<F>(nullptr, nullptr, 0), one));
  const Fe other[2] = {one, one};
  CHECK(fe_is_zero<F>(r1cs_eq_eval<F>(at2, other, 2)));
  CHECK(fe_eq<F>(r1cs_rho_combine<F>(pm1, one, one, one), one));  // 1 - 1 + 1
  printf("ok chunk=%u\n", zkw::kWiredChunk);
  return 0;
}

template <class F>
static int digest_mode(uint32_t field) {
  Inst in;
  const char* err = nullptr;
  int rc = read_instance(field, in, &err);
  std::vector<Fe> vm;
  if (!rc) rc = r1cs_entries<F>(in.sh, in.rows.data(), in.cols.data(), in.vals.data(), false, vm, &err);
  if (rc) {
    printf("error=%d %s\n", rc, err);
    return 0;
  }
  uint8_t d[32];
  r1cs_digest<F>(in.sh, in.rows.data(), in.cols.data(), vm.data(), d);
  for (int i = 0; i < 32; ++i) printf("%02x", d[i]);
  printf("\n");
  return 0;
}

template <class F>
static void print_polys(const char* name, const zkc::ComposedOut& o, uint32_t degree) {
  printf("%s", name);
  for (size_t k = 0; k < o.ncoeffs.size(); ++k) {
    printf(" %u", (unsigned)o.ncoeffs[k]);
    for (uint32_t i = 0; i < o.ncoeffs[k]; ++i) {
      printf(" ");
      print_fe<F>(o.coeffs[(size_t)(degree + 1) * k + i], "");
    }
    printf(" |");
  }
  printf("\n");
}

template <class F>
static int transcript_mode(uint32_t field) {
  Inst in;
  const char* err = nullptr;
  int rc = read_instance(field, in, &err);
  std::vector<Fe> vm;
  if (!rc) rc = r1cs_entries<F>(in.sh, in.rows.data(), in.cols.data(), in.vals.data(), false, vm, &err);
  if (rc) {
    printf("error=%d %s\n", rc, err);
    return 0;
  }
  if (in.sh.sx > 10 || in.sh.sy > 10) return 2;
  const size_t H = (size_t)1 << (in.sh.sy - 1);
  std::vector<Fe> w(H), io(in.sh.npub);
  for (auto& x : w) x = read_fe<F>();
  for (auto& x : io) x = read_fe<F>();
  uint64_t cm[12];
  const bool committed = read_u32() != 0;
  if (committed) {
    read_words(cm, 6);
    read_words(cm + 6, 6);
  }
  uint8_t digest[32];
  r1cs_digest<F>(in.sh, in.rows.data(), in.cols.data(), vm.data(), digest);
  zk_transcript tr;
  R1csProof<F> p;
  r1cs_host_prove<F>(in.sh, in.rows.data(), in.cols.data(), vm.data(), digest, w.data(), io.data(),
                     committed ? cm : nullptr, &tr, p);
  auto line = [](const char* name, const std::vector<Fe>& v) {
    printf("%s", name);
    for (const Fe& x : v) {
      printf(" ");
      print_fe<F>(x, "");
    }
    printf("\n");
  };
  line("tau", p.tau);
  line("rx", p.sc1.challenges);
  line("evals", {p.va, p.vb, p.vc});
  line("rho", {p.rho});
  line("ry", p.sc2.challenges);
  line("vw", {p.vw});
  print_polys<F>("polys1", p.sc1, kSc1Degree);
  print_polys<F>("polys2", p.sc2, kSc2Degree);
  zk_transcript end = tr;
  line("next", {zkh::challenge<F>(&end)});
  // the verifier on the same proof, on a fresh transcript: it accepts and ends in the same state
  zk_transcript tv;
  std::vector<Fe> rx, ry;
  auto me = [&](const Fe* px, const Fe* py, Fe(&m)[3]) {
    r1cs_host_matrix_evals<F>(in.sh, in.rows.data(), in.cols.data(), vm.data(), px, py, m);
  };
  const bool ok = r1cs_verify<F>(in.sh, digest, io.data(), p.sc1.coeffs.data(), p.sc1.ncoeffs.data(), p.sc2.coeffs.data(),
                                 p.sc2.ncoeffs.data(), p.va, p.vb, p.vc, p.vw, committed ? cm : nullptr, &tv, me, rx, ry);
  const bool same_end = ok && fe_eq<F>(zkh::challenge<F>(&tv), zkh::challenge<F>(&tr));
  printf("verified %d\n", ok && same_end ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string op(argv[1]);
  if (op == "self") return self_check();
  if (argc != 3) return 2;
  const uint32_t field = (uint32_t)atoi(argv[2]);
  const bool digest = op == "digest";
  if (!digest && op != "transcript") return 2;
  switch (field) {
    case 0: return digest ? digest_mode<Bn254Fr>(0) : transcript_mode<Bn254Fr>(0);
    case 1: return digest ? digest_mode<Bn254Fq>(1) : transcript_mode<Bn254Fq>(1);
    case 2: return digest ? digest_mode<Bls12_381Fr>(2) : transcript_mode<Bls12_381Fr>(2);
  }
  return 2;
}
