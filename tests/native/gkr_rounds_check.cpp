// Round-arithmetic checker for tests/test_gkr_rounds_cpu.py (test
// infrastructure, not the product): drives csrc/gkr_rounds.hpp on one fresh
// transcript. Field: argv[1] = 0 (BN254 Fr), 1 (BN254 Fq), 2 (BLS12-381 Fr).
// Commands on stdin, every field value one canonical hex integer:
//   three i0 first v0 .. v26        three_rounds from the 27 moment sums
//   two i0 first n v0 .. v(n-1)     two_rounds from n = 8 or 9 product sums
//   tables len A.. S.. M.. P..      load four tables of len entries
//   hostround i first               host_round_sums (with e1, checked against the plain variant),
//                                   round i (first: e1 from the sums), host_fold by its challenge
//   hostrounds nv i fin             host_rounds over the loaded tables (taken as level i - 2, packed
//                                   word-major as the device hands them over); fin = 1: prints "fin v0 v1 v2 v3"
//   eq8 rz ra rb                    prints the eight eq weights on one line
// Every round run prints "k m c0 c1 c2 r": its index, trimmed coefficient count,
// coefficients (zero past m) and challenge.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "gkr_rounds.hpp"

using namespace zk;
using namespace zkh;

template <class F>
Fe read_fe() {
  char s[80];
  if (scanf("%79s", s) != 1) exit(2);
  const size_t n = strlen(s);
  h64::V v{};
  for (size_t i = 0; i < n; ++i) {  // hex digits, least significant last
    const char ch = s[n - 1 - i];
    const uint64_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    if (i < 64) v.l[i / 16] |= d << (4 * (i % 16));
  }
  return hfe_to_mont<F>(h64::fe(v));
}
template <class F>
void print_fe(const Fe& m, const char* end) {
  const h64::V o = h64::of(hfe_from_mont<F>(m));
  printf("%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%016" PRIx64 "%s", o.l[3], o.l[2], o.l[1], o.l[0], end);
}

template <class F>
int run() {
  constexpr uint32_t kMax = 64;
  zk_transcript tr;
  GkrOut out;
  out.coeffs.assign(3 * kMax, fe_zero<F>());
  out.ncoeffs.assign(kMax, 0);
  out.challenges.assign(kMax, fe_zero<F>());
  Fe claim = fe_zero<F>(), r = claim;
  RoundState s{&tr, out, claim, r, 0, claim, claim, claim};
  std::vector<Fe> T[4];
  auto show = [&](uint32_t k0, uint32_t k1) {
    for (uint32_t k = k0; k < k1; ++k) {
      printf("%u %u ", k, (unsigned)out.ncoeffs[k]);
      for (int q = 0; q < 3; ++q) print_fe<F>(out.coeffs[3 * k + q], " ");
      print_fe<F>(out.challenges[k], "\n");
    }
  };
  char op[16];
  while (scanf("%15s", op) == 1) {
    const std::string o(op);
    if (o == "three") {
      uint32_t i0, first;
      if (scanf("%u %u", &i0, &first) != 2) return 2;
      Fe v[27];
      for (auto& x : v) x = read_fe<F>();
      three_rounds<F>(s, i0, first != 0, v);
      show(i0, i0 + 3);
    } else if (o == "two") {
      uint32_t i0, first, n;
      if (scanf("%u %u %u", &i0, &first, &n) != 3 || n > 9) return 2;
      Fe v[9];
      for (uint32_t q = 0; q < n; ++q) v[q] = read_fe<F>();
      two_rounds<F>(s, i0, first != 0, v);
      show(i0, i0 + 2);
    } else if (o == "tables") {
      size_t len;
      if (scanf("%zu", &len) != 1) return 2;
      for (auto& t : T) {
        t.resize(len);
        for (auto& x : t) x = read_fe<F>();
      }
    } else if (o == "hostround") {
      uint32_t i, first;
      if (scanf("%u %u", &i, &first) != 2) return 2;
      Fe e0, e1, e2, p0, p2;
      host_round_sums<F, true>(T, e0, e2, &e1);
      host_round_sums<F>(T, p0, p2);
      if (!fe_eq<F>(e0, p0) || !fe_eq<F>(e2, p2)) {
        printf("with-e1 sums differ from the plain ones\n");
        return 1;
      }
      if (first) one_round<F>(s, i, e0, e1, e2);
      else later_round<F>(s, i, e0, e2);
      host_fold<F>(T, s.r);
      show(i, i + 1);
    } else if (o == "hostrounds") {
      uint32_t nv, i, fin;
      if (scanf("%u %u %u", &nv, &i, &fin) != 3) return 2;
      const size_t len = T[0].size();
      if (len != (size_t)1 << (nv - i + 2)) return 2;
      std::vector<uint64_t> raw(16 * len);
      for (int t = 0; t < 4; ++t)
        for (size_t e = 0; e < len; ++e)
          for (int k = 0; k < 4; ++k) raw[(size_t)t * 4 * len + k * len + e] = h64::of(T[t][e]).l[k];
      FinalVals fv;
      host_rounds<F>(s, i, nv, raw.data(), fin ? &fv : nullptr);
      show(i, nv);
      if (fin) {
        printf("fin ");
        for (int t = 0; t < 4; ++t) print_fe<F>(fv.v[t], t == 3 ? "\n" : " ");
      }
    } else if (o == "eq8") {
      const Fe rz = read_fe<F>(), ra = read_fe<F>(), rb = read_fe<F>();
      Fe e[8];
      eq8_weights<F>(rz, ra, rb, e);
      for (int q = 0; q < 8; ++q) print_fe<F>(e[q], q == 7 ? "\n" : " ");
    } else {
      return 2;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  const int f = argc > 1 ? atoi(argv[1]) : 0;
  return f == 0 ? run<Bn254Fr>() : f == 1 ? run<Bn254Fq>() : run<Bls12_381Fr>();
}
