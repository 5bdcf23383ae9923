// csrc/field.hpp, the arithmetic under every kernel, compiled for the host and
// driven from tests/test_field_palette_cpu.py: a stand-alone program (host code
// only, no GPU, no library). It reads one case per line,
//   <field> add|sub|mul <a> <b>     the operation on two words below p
//   <field> inv <a>                 fe_inv
//   <field> mac <a> <b> <n>         wide_redc of n wide_mac(a, b) into one accumulator
//   <field> redc <v>                wide_redc of a 544-bit value
// (hexadecimal, no prefix; n decimal) and prints one 256-bit result per line.
// The words are what the functions see: nothing is converted on the way.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "field.hpp"

using namespace zk;

template <int W>
static bool parse(const char* s, uint32_t (&w)[W]) {
  for (int i = 0; i < W; ++i) w[i] = 0;
  const size_t n = strlen(s);
  if (n == 0 || n > 8 * (size_t)W) return false;
  for (size_t i = 0; i < n; ++i) {
    const char c = s[n - 1 - i];
    uint32_t d;
    if (c >= '0' && c <= '9') d = (uint32_t)(c - '0');
    else if (c >= 'a' && c <= 'f') d = (uint32_t)(c - 'a' + 10);
    else return false;
    w[i / 8] |= d << (4 * (i % 8));
  }
  return true;
}

static void print(const Fe& x) {
  for (int i = 7; i >= 0; --i) printf("%08x", x.v[i]);
  printf("\n");
}

template <class F>
static bool run(const char* op, char* const* arg, int nargs) {
  Fe a, b;
  if (!strcmp(op, "redc")) {
    Wide v;
    if (nargs != 1 || !parse(arg[0], v.w)) return false;
    print(wide_redc<F>(v));
    return true;
  }
  if (nargs < 1 || !parse(arg[0], a.v)) return false;
  if (!strcmp(op, "inv")) {
    if (nargs != 1) return false;
    print(fe_inv<F>(a));
    return true;
  }
  if (nargs < 2 || !parse(arg[1], b.v)) return false;
  if (!strcmp(op, "mac")) {
    if (nargs != 3) return false;
    const long n = strtol(arg[2], nullptr, 10);
    Wide acc = wide_zero<F>();
    for (long i = 0; i < n; ++i) wide_mac<F>(acc, a, b);
    print(wide_redc<F>(acc));
    return true;
  }
  if (nargs != 2) return false;
  if (!strcmp(op, "add")) print(fe_add<F>(a, b));
  else if (!strcmp(op, "sub")) print(fe_sub<F>(a, b));
  else if (!strcmp(op, "mul")) print(fe_mul<F>(a, b));
  else return false;
  return true;
}

int main() {
  static char line[1024];
  long lineno = 0;
  while (fgets(line, sizeof line, stdin)) {
    ++lineno;
    char* tok[6];
    int n = 0;
    for (char* t = strtok(line, " \n"); t && n < 6; t = strtok(nullptr, " \n")) tok[n++] = t;
    if (n == 0) continue;
    bool ok = n >= 3;
    if (ok) {
      const int field = atoi(tok[0]);
      if (field == BN254_FR) ok = run<Bn254Fr>(tok[1], tok + 2, n - 2);
      else if (field == BN254_FQ) ok = run<Bn254Fq>(tok[1], tok + 2, n - 2);
      else if (field == BLS12_381_FR) ok = run<Bls12_381Fr>(tok[1], tok + 2, n - 2);
      else ok = false;
    }
    if (!ok) {
      fprintf(stderr, "line %ld: cannot parse\n", lineno);
      return 2;
    }
  }
  return 0;
}
