// TEST INFRASTRUCTURE: the G1 mixed addition of the table kernels (g1_madd_inl, rabe_amd/csrc/bn254/curve.h) against the generic
// jac_add_aff<Fp> of the same header, on the CPU.  The two use different formulas and return different Jacobian representatives of
// one point, so they are compared after the conversion to affine.  Stand-alone (own main, no Python loading): it can be built with
// a host sanitizer.  Driven by tests/test_g1_madd_forms.py.
//
// stdin:  records of 5 x 8 little-endian 32-bit limbs, MONTGOMERY forms (< p) of X1, Y1, Z1 (the Jacobian p; Z1 = 0: infinity) and
//         x2, y2 (the affine q; x2 = y2 = 0: infinity).  Raw limbs, so that a test can place any limb pattern in any coordinate.
// stdout: per record 64 + 64 bytes, the canonical affine result of g1_madd_inl and of jac_add_aff<Fp>.
// exit:   0 when every record agrees, 1 otherwise (the first differing records are named on stderr), 2 on malformed input.
#include "../../rabe_amd/csrc/bn254/io.h"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace rabe::bn254;

static Fp raw_fp(const uint32_t* p) {
  Fp r;
  for (int i = 0; i < 8; i++) r.v[i] = p[i];
  return r;
}

int main() {
  std::vector<uint32_t> in;
  uint32_t chunk[40];
  size_t got;
  while ((got = fread(chunk, 1, sizeof(chunk), stdin)) == sizeof(chunk)) in.insert(in.end(), chunk, chunk + 40);
  if (got != 0) {
    fprintf(stderr, "g1_madd_forms: input is not a whole number of 160-byte records\n");
    return 2;
  }
  const size_t n = in.size() / 40;
  size_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t* rec = in.data() + 40 * i;
    const G1Jac p{raw_fp(rec), raw_fp(rec + 8), raw_fp(rec + 16)};
    const G1Aff q{raw_fp(rec + 24), raw_fp(rec + 32)};
    uint32_t out[32];
    store_g1(out, jac_to_aff(g1_madd_inl(p, q)));
    store_g1(out + 16, jac_to_aff(jac_add_aff<Fp>(p, q)));
    if (memcmp(out, out + 16, 64) != 0 && bad++ < 8) fprintf(stderr, "g1_madd_forms: record %zu differs\n", i);
    if (fwrite(out, 1, sizeof(out), stdout) != sizeof(out)) return 2;
  }
  fprintf(stderr, "g1_madd_forms: %zu records, %zu differ\n", n, bad);
  return bad ? 1 : 0;
}
