// CPU test (tests/test_field_primitives_cpu.py): the host twins of the device primitives on the
// operand vectors of tests/fieldref.py.  Reads lines "<op> <fr|fq> <hex operand>..." (256-bit
// values, most significant digit first), calls the library's own host function (bn254.hpp) and
// prints one line of hex results a case.  No arithmetic of its own.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bn254.hpp"
using namespace tns;

template <class C>
static Fp<C> parse(const char *h) {
  Fp<C> r = Fp<C>::zero();
  for (int i = 0; i < 64; i++) {
    const char c = h[i];
    const u32 d = c <= '9' ? c - '0' : (c | 32) - 'a' + 10;
    const int bit = 4 * (63 - i);
    r.v[bit >> 5] |= d << (bit & 31);
  }
  return r;
}
template <class C>
static void put(const Fp<C> &a) {
  for (int i = 7; i >= 0; i--) printf("%08x", a.v[i]);
}
static void put(const G1Xyzz &p) {
  put(p.x), putchar(' '), put(p.y), putchar(' '), put(p.zz), putchar(' '), put(p.zzz);
}

template <class C>
static bool field_op(const std::string &op, const std::vector<std::string> &a) {
  auto F = [&](int i) { return parse<C>(a[i].c_str()); };
  if (op == "mul_cios" && a.size() == 2) put(mul_cios(F(0), F(1)));
  else if (op == "mul_cios64" && a.size() == 2) put(mul_cios64(F(0), F(1)));
  else if (op == "add" && a.size() == 2) put(add(F(0), F(1)));
  else if (op == "sub" && a.size() == 2) put(sub(F(0), F(1)));
  else if (op == "neg" && a.size() == 1) put(neg(F(0)));
  else if (op == "reduce_once" && a.size() == 1) {
    Fp<C> x = F(0);
    reduce_once(x);
    put(x);
  } else if (op == "inv_binary_host" && a.size() == 1) put(inv_binary_host(F(0)));
  else return false;
  return true;
}

static bool point_op(const std::string &op, const std::vector<std::string> &a) {
  auto F = [&](int i) { return parse<FqCfg>(a[i].c_str()); };
  auto X = [&](int i) {
    G1Xyzz p;
    p.x = F(i), p.y = F(i + 1), p.zz = F(i + 2), p.zzz = F(i + 3);
    return p;
  };
  if (op == "xyzz_add" && a.size() == 8) put(xyzz_add(X(0), X(4)));
  else if (op == "xyzz_madd" && a.size() == 6) {
    G1Affine q;
    q.x = F(4), q.y = F(5);
    put(xyzz_madd(X(0), q));
  } else if (op == "xyzz_dbl" && a.size() == 4) put(xyzz_dbl(X(0)));
  else return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  static char line[1024];
  while (fgets(line, sizeof line, f)) {
    std::vector<std::string> tok;
    for (char *t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
    if (tok.size() < 3) return 3;
    const std::string op = tok[0], fld = tok[1];
    const std::vector<std::string> args(tok.begin() + 2, tok.end());
    for (const std::string &s : args)
      if (s.size() != 64) return 3;
    const bool ok = op.rfind("xyzz_", 0) == 0 ? fld == "fq" && point_op(op, args)
                    : fld == "fr"             ? field_op<FrCfg>(op, args)
                    : fld == "fq"             ? field_op<FqCfg>(op, args)
                                              : false;
    if (!ok) return 3;
    putchar('\n');
  }
  fclose(f);
  return 0;
}
