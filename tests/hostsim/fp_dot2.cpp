// TEST INFRASTRUCTURE: the two-term Montgomery dot product (mont_dot2_raw / dot2_inl, rabe_amd/csrc/bn254/fp.h) on the CPU: the loop
// form that follows the carry-capture plan -- a product the plan takes as safe is added WITHOUT looking at its carry, as the generated
// device routine issues it.  Stand-alone (own main, no Python loading): it can be built with a host sanitizer.  Driven by
// tests/test_mac_plan_dot2.py and tests/test_fp_dot2_host.py.
//
// fp_dot2 plan      prints the plan the kernels compile from: one line per field (Fp, Fr) of 16 safe masks and last_safe, in hex
// fp_dot2 fp | fr   stdin:  records of 4 x 8 little-endian 32-bit limbs, the RAW Montgomery residues (< modulus) a0, b0, a1, b1
//                   stdout: per record 8 + 8 limbs, the raw residues of dot2_inl(a0, b0, a1, b1) and of add(mul(a0, b0), mul(a1, b1))
// fp_dot2 walk      stdin:  records of 2 x 8 limbs, raw Montgomery residues x, y of affine G1 points (x = y = 0: infinity)
//                   stdout: 64 + 64 bytes, the canonical affine sum of all of them by a walk of g1_madd_inl from an infinite
//                           accumulator (it stays Jacobian from step to step, as in the table kernels) and by jac_add_aff<Fp>
// exit: 0 when every record agrees, 1 otherwise, 2 on malformed input or a result that is not below the modulus.
#include "../../rabe_amd/csrc/bn254/io.h"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace rabe::bn254;

template <class M>
static void print_plan() {
  constexpr ColumnPlan<M> plan(true, M::mod(7) + 1, M::mod(7) + 1, 2);
  for (int k = 0; k < 16; k++) {
    unsigned from_accessor = 0;
    for (int i = 0; i < 8; i++) from_accessor |= (unsigned)plan_dot2_safe<M>(k, i) << i;
    if (from_accessor != plan.safe[k]) printf("!");          // the accessors the routine reads ARE this plan
    printf("%x ", (unsigned)plan.safe[k]);
  }
  unsigned last = 0;
  for (int k = 0; k < 8; k++) last |= (unsigned)plan_dot2_last_safe<M>(k) << k;
  printf("%x\n", last == plan.last_safe ? (unsigned)plan.last_safe : 0xFFFFu);
}

template <class M>
static bool below_mod(const Mont<M>& a) {
  for (int i = 7; i >= 0; i--) {
    if (a.v[i] < M::mod(i)) return true;
    if (a.v[i] > M::mod(i)) return false;
  }
  return false;
}

template <class M>
static Mont<M> raw(const uint32_t* p) {
  Mont<M> r;
  for (int i = 0; i < 8; i++) r.v[i] = p[i];
  return r;
}

template <class M>
static int run() {
  std::vector<uint32_t> in;
  uint32_t chunk[32];
  size_t got;
  while ((got = fread(chunk, 1, sizeof(chunk), stdin)) == sizeof(chunk)) in.insert(in.end(), chunk, chunk + 32);
  if (got != 0) {
    fprintf(stderr, "fp_dot2: input is not a whole number of 128-byte records\n");
    return 2;
  }
  const size_t n = in.size() / 32;
  size_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t* rec = in.data() + 32 * i;
    const Mont<M> a0 = raw<M>(rec), b0 = raw<M>(rec + 8), a1 = raw<M>(rec + 16), b1 = raw<M>(rec + 24);
    const Mont<M> d = dot2_inl(a0, b0, a1, b1);
    const Mont<M> s = add(mul_inl(a0, b0), mul_inl(a1, b1));
    if (!below_mod(d)) {
      fprintf(stderr, "fp_dot2: record %zu: result not below the modulus\n", i);
      return 2;
    }
    uint32_t out[16];
    for (int j = 0; j < 8; j++) { out[j] = d.v[j]; out[8 + j] = s.v[j]; }
    if (memcmp(out, out + 8, 32) != 0 && bad++ < 8) fprintf(stderr, "fp_dot2: record %zu differs\n", i);
    if (fwrite(out, 1, sizeof(out), stdout) != sizeof(out)) return 2;
  }
  fprintf(stderr, "fp_dot2: %zu records, %zu differ\n", n, bad);
  return bad ? 1 : 0;
}

static int walk() {
  uint32_t rec[16];
  size_t got;
  G1Jac a = jac_inf<Fp>(), b = jac_inf<Fp>();
  while ((got = fread(rec, 1, sizeof(rec), stdin)) == sizeof(rec)) {
    const G1Aff q{raw<FpParams>(rec), raw<FpParams>(rec + 8)};
    a = g1_madd_inl(a, q);
    b = jac_add_aff<Fp>(b, q);
  }
  if (got != 0) return 2;
  uint32_t out[32];
  store_g1(out, jac_to_aff(a));
  store_g1(out + 16, jac_to_aff(b));
  if (fwrite(out, 1, sizeof(out), stdout) != sizeof(out)) return 2;
  return memcmp(out, out + 16, 64) ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "walk")) return walk();
  if (argc == 2 && !strcmp(argv[1], "plan")) {
    print_plan<FpParams>();
    print_plan<FrParams>();
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "fp")) return run<FpParams>();
  if (argc == 2 && !strcmp(argv[1], "fr")) return run<FrParams>();
  fprintf(stderr, "usage: fp_dot2 plan | fp | fr\n");
  return 2;
}
