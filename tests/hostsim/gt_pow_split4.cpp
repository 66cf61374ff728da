// TEST INFRASTRUCTURE: the Gt power over a four-way Frobenius split (gt_pow_split4 / gtpow4_masks, rabe_amd/csrc/bn254/gtpow4.h: what
// k_gt_pow_rows runs per lane) against gt_pow_window of the same headers, on the CPU.  Stand-alone (own main, no Python loading): it can
// be built with a host sanitizer.  Driven by tests/test_gt_pow_split4.py, which also holds the oracle's answers.
//
// stdin:  records of 804 bytes: a (384, canonical wire form), mul (384), k (32, any 256-bit little-endian word), flags (4: bit 0 invert,
//         bit 1 multiply by mul).
// stdout: per record 384 + 384 bytes: (mul *) a^(+-k) by gt_pow_split4 and by gt_pow_window.
// exit:   0 when every record agrees, 1 otherwise (the first differing records are named on stderr), 2 on malformed input.
// Built with -DRB_COUNT_MULS it also prints the Fp multiplications of the two routines (conversions of the harness not counted).
#include "../../rabe_amd/csrc/bn254/io.h"
#include "../../rabe_amd/csrc/bn254/gtpow4.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#ifdef RB_COUNT_MULS
extern "C" { unsigned long long rb_mul_counter = 0; }
#endif

using namespace rabe::bn254;

// the accumulator's home (LDS on the device): two halves + the parked Fq6
struct HostHome {
  Fp6* F;
  Fp6 ld_f6(int h) const { return F[h]; }
  void st_f6(int h, const Fp6& v) const { F[h] = v; }
  Fp6 ld_x() const { return F[2]; }
  void st_x(const Fp6& v) const { F[2] = v; }
  Fp2 ld_f2(int i) const { return (&F[i / 3].a0)[i % 3]; }
  void st_f2(int i, const Fp2& v) const { (&F[i / 3].a0)[i % 3] = v; }
  void fence() const {}
};
struct HostOperand {
  const Fp12* e;
  bool conj;
  Fp6 half(int h) const { return h ? (conj ? fp6_neg(e->c1) : e->c1) : e->c0; }
};
// the four columns, kept in memory as the kernel keeps them
struct HostBases {
  const Fp12* img;
  HostOperand operand(int i, bool conj) const { return HostOperand{img + i, conj}; }
};

static unsigned long long counter() {
#ifdef RB_COUNT_MULS
  return rb_mul_counter;
#else
  return 0;
#endif
}

int main() {
  const size_t REC = 804;
  std::vector<unsigned char> in;
  unsigned char chunk[804];
  size_t got;
  while ((got = fread(chunk, 1, REC, stdin)) == REC) in.insert(in.end(), chunk, chunk + REC);
  if (got != 0) {
    fprintf(stderr, "gt_pow_split4: input is not a whole number of 804-byte records\n");
    return 2;
  }
  const size_t n = in.size() / REC;
  size_t bad = 0;
  unsigned long long muls_split = 0, muls_window = 0;
  for (size_t r = 0; r < n; r++) {
    uint32_t rec[201];
    memcpy(rec, in.data() + REC * r, REC);
    const Fp12 a = load_gt(rec), mul_in = load_gt(rec + 96);
    const uint32_t* k = rec + 192;
    const bool invert = (rec[200] & 1u) != 0, has_mul = (rec[200] & 2u) != 0;
    uint32_t out[192];
    {
      const unsigned long long c0 = counter();
      uint32_t m[24];
      gtpow4_masks(k, invert, m);
      Fp12 img[4];
      img[0] = a;
      img[1] = fp12_frob1(a);
      img[2] = fp12_frob2(a);
      img[3] = fp12_frob3(a);
      Fp6 F[3];
      const HostHome home{F};
      const bool started = gt_pow_split4(home, HostBases{img}, m);
      if (has_mul) {
        if (started) facc_mul(home, HostOperand{&mul_in, false});
        else facc_set(home, HostOperand{&mul_in, false});
      }
      const Fp12 res = (started || has_mul) ? facc_get(home) : fp12_one();
      muls_split += counter() - c0;
      store_gt(out, res);
    }
    {
      const unsigned long long c0 = counter();
      Fp12 p = gt_pow_window(a, k);
      if (invert) p = fp12_conj(p);
      if (has_mul) p = fp12_mul(mul_in, p);
      muls_window += counter() - c0;
      store_gt(out + 96, p);
    }
    if (memcmp(out, out + 96, 384) != 0 && bad++ < 8) fprintf(stderr, "gt_pow_split4: record %zu differs\n", r);
    if (fwrite(out, 1, sizeof(out), stdout) != sizeof(out)) return 2;
  }
  fprintf(stderr, "gt_pow_split4: %zu records, %zu differ\n", n, bad);
#ifdef RB_COUNT_MULS
  if (n) fprintf(stderr, "fp_muls_per_power split4=%.1f window=%.1f\n", (double)muls_split / n, (double)muls_window / n);
#endif
  return bad ? 1 : 0;
}
