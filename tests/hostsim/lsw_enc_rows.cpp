// TEST INFRASTRUCTURE: the LSW row routine (rabe_amd/csrc/bn254/lsw_rows.h: what a lane of k_lsw_enc_rows runs) on the CPU, beside a
// restatement of the path lsw::encrypt_packed runs today -- four window walks, each converted to affine bytes, and k_g1_add over two of
// them.  Stand-alone (own main, no Python loading): it can be built with a host sanitizer.  Driven by tests/test_lsw_enc_rows_host.py,
// which holds the oracle's answers.
//
// stdin:  256 bytes: g1, g1_b, g1_b2, h_b (canonical wire form); then records of 96 bytes: h, secret, sx (little-endian, canonical).
// stdout: per record 192 + 192 bytes: e3, e4, e5 of the fused routine and of the four walks plus the addition.
// exit:   0 when every record agrees, 1 otherwise (the first differing records are named on stderr), 2 on malformed input.
// Built with -DRB_COUNT_MULS it also prints the Fp / Fr Montgomery multiplications per row of the two paths.  A window-table entry is
// computed where it is asked for and not counted (the device reads it from HBM), nor is an inversion the device shares among the 256
// lanes of a block -- ONE per row in the fused routine, FOUR per row in the four walks; the addition kernel's own inversion, one per
// lane, is counted.
#include "../../rabe_amd/csrc/bn254/lsw_rows.h"
#include <stdio.h>
#include <string.h>
#include <vector>

#ifdef RB_COUNT_MULS
extern "C" { unsigned long long rb_mul_counter = 0; }
#endif

using namespace rabe::bn254;

static unsigned long long counter() {
#ifdef RB_COUNT_MULS
  return rb_mul_counter;
#else
  return 0;
#endif
}
static void set_counter(unsigned long long v) {
#ifdef RB_COUNT_MULS
  rb_mul_counter = v;
#else
  (void)v;
#endif
}
// (d 2^(16 w)) * base, computed on demand
struct LazyTable {
  G1Aff base;
  G1Aff entry(int w, uint32_t d) const {
    const unsigned long long c = counter();
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (w & 1) k[w >> 1] = d << 16; else k[w >> 1] = d;
    const G1Aff e = jac_to_aff(jac_mul_binary(base, k));
    set_counter(c);
    return e;
  }
};
static Fp shared_inv(const Fp& a) {          // the block's inversion: not a lane's work
  const unsigned long long c = counter();
  const Fp r = inv(a);
  set_counter(c);
  return r;
}
// k_table_mul_g1: one walk, the block's inversion, affine canonical bytes
static void table_mul(const LazyTable& t, const uint32_t k[8], uint32_t out[16]) {
  const G1Jac r = lsw_walk16(jac_inf<Fp>(), t, k);
  const bool inf = jac_is_inf(r);
  const Fp zinv = shared_inv(inf ? one<FpParams>() : r.z);
  store_g1(out, inf ? aff_inf<Fp>() : jac_to_aff_with_zinv(r, zinv));
}

int main() {
  uint32_t key[64];
  if (fread(key, 1, sizeof(key), stdin) != sizeof(key)) {
    fprintf(stderr, "lsw_enc_rows: no key\n");
    return 2;
  }
  const LazyTable g1{load_g1(key)}, g1_b{load_g1(key + 16)}, g1_b2{load_g1(key + 32)}, h_b{load_g1(key + 48)};
  set_counter(0);
  uint32_t rec[24];
  size_t got, n = 0, bad = 0;
  unsigned long long muls_fused = 0, muls_four = 0;
  while ((got = fread(rec, 1, sizeof(rec), stdin)) == sizeof(rec)) {
    const uint32_t *h = rec, *secret = rec + 8, *sx = rec + 16;
    uint32_t out[96];
    {
      const unsigned long long c0 = counter();
      const G1Jac a = lsw_row_e3(g1, load_fr(h), load_fr(secret));
      const G1Jac b = lsw_row_e4(g1_b, sx);
      const G1Jac c = lsw_row_e5(g1_b2, h_b, load_fr(h), sx);
      G1Three z;
      const Fp abc = g1_three_product(z, a, b, c);
      G1Aff e[3];
      g1_three_to_aff(z, shared_inv(abc), a, b, c, e);
      store_g1(out, e[0]);
      store_g1(out + 16, e[1]);
      store_g1(out + 32, e[2]);
      muls_fused += counter() - c0;
    }
    {
      // the host forms the products (lsw::encrypt_packed): not device work
      uint32_t ka[8], kc[8];
      const unsigned long long c = counter();
      from_mont<FrParams>(ka, mul(load_fr(h), load_fr(secret)));
      from_mont<FrParams>(kc, mul(load_fr(sx), load_fr(h)));
      set_counter(c);
      const unsigned long long c0 = counter();
      uint32_t t1[16], t2[16];
      table_mul(g1, ka, out + 48);
      table_mul(g1_b, sx, out + 64);
      table_mul(g1_b2, kc, t1);
      table_mul(h_b, sx, t2);
      store_g1(out + 80, jac_to_aff(jac_add_aff(aff_to_jac(load_g1(t1)), load_g1(t2))));          // k_g1_add
      muls_four += counter() - c0;
    }
    if (memcmp(out, out + 48, 192) != 0 && bad++ < 8) fprintf(stderr, "lsw_enc_rows: record %zu differs\n", n);
    if (fwrite(out, 1, sizeof(out), stdout) != sizeof(out)) return 2;
    n++;
  }
  if (got != 0) {
    fprintf(stderr, "lsw_enc_rows: input is not a whole number of 96-byte records\n");
    return 2;
  }
  fprintf(stderr, "lsw_enc_rows: %zu records, %zu differ\n", n, bad);
#ifdef RB_COUNT_MULS
  if (n) fprintf(stderr, "muls_per_row fused=%.1f four_walks_plus_add=%.1f\n", (double)muls_fused / n, (double)muls_four / n);
#endif
  return bad ? 1 : 0;
}
