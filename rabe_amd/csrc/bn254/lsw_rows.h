// One LSW ciphertext row (lsw/mod.rs:201-208): what a lane of k_lsw_enc_rows (engine_keys.hip) runs, as host + device code so that the
// same routine is checked on the CPU (tests/hostsim/lsw_enc_rows.cpp) against the oracle's point arithmetic.
//
// With h the hash of the row's attribute, `secret` the item's and sx the row's own scalar:
//   e3 = g1 * (h secret)          e4 = g1_b * sx          e5 = g1_b2 * (sx h) + h_b * sx
// Every element is a walk over the 16-bit windows of a fixed base; e5 is two walks on ONE accumulator.  A table is anything with
//   G1Aff entry(int w, uint32_t d) const          (d 2^(16 w)) * base, affine Montgomery, 1 <= d <= 65535
// (the device reads its window tables in HBM, the CPU check computes the entry it is asked for).
#pragma once
#include "io.h"
#include "table_walk.h"

namespace rabe { namespace bn254 {

// acc + tbl * k: the 16-bit walk of table_walk.h with one mixed addition (g1_madd_inl: the Z3 = Z1*H form, with its doubling and
// cancelling cases) per non-zero digit
template <class TBL>
RB_HD G1Jac lsw_walk16(G1Jac acc, const TBL& tbl, const uint32_t k[8]) {
  walk16(k, [&](int w, uint32_t d) { acc = g1_madd_inl(acc, tbl.entry(w, d)); });
  return acc;
}
// the three elements, one at a time: the scalar of a walk is formed just before it (the two products h secret and sx h in Montgomery form,
// then brought back to the canonical words the digits are cut from) and nothing but the accumulator lives across a walk
template <class TBL>
RB_HD G1Jac lsw_row_e3(const TBL& g1, const Fr& h, const Fr& secret) {
  uint32_t kk[8];
  from_mont_inl<FrParams>(kk, mul_inl(h, secret));
  return lsw_walk16(jac_inf<Fp>(), g1, kk);
}
template <class TBL>
RB_HD G1Jac lsw_row_e4(const TBL& g1_b, const uint32_t sx[8]) { return lsw_walk16(jac_inf<Fp>(), g1_b, sx); }
template <class TBL>
RB_HD G1Jac lsw_row_e5(const TBL& g1_b2, const TBL& h_b, const Fr& h, const uint32_t sx[8]) {
  uint32_t kk[8];
  from_mont_inl<FrParams>(kk, mul_inl(to_mont<FrParams>(sx), h));
  return lsw_walk16(lsw_walk16(jac_inf<Fp>(), g1_b2, kk), h_b, sx);
}

// Three Jacobian points -> affine with ONE inversion (Montgomery's trick over the three Z).  A point at infinity (Z = 0) enters the product
// as one, so it neither zeroes the product nor disturbs the inverses of the other two, and leaves as the affine identity (0, 0).
struct G1Three {
  Fp za, zb, zc, ab;
  bool ia, ib, ic;
};
// returns za zb zc, the value to invert (on the device: together with the block's other lanes)
RB_HD Fp g1_three_product(G1Three& t, const G1Jac& a, const G1Jac& b, const G1Jac& c) {
  t.ia = jac_is_inf(a); t.ib = jac_is_inf(b); t.ic = jac_is_inf(c);
  t.za = t.ia ? one<FpParams>() : a.z;
  t.zb = t.ib ? one<FpParams>() : b.z;
  t.zc = t.ic ? one<FpParams>() : c.z;
  t.ab = mul(t.za, t.zb);
  return mul(t.ab, t.zc);
}
RB_HD void g1_three_to_aff(const G1Three& t, const Fp& inv_abc, const G1Jac& a, const G1Jac& b, const G1Jac& c, G1Aff out[3]) {
  const Fp zc_inv = mul(inv_abc, t.ab);
  const Fp inv_ab = mul(inv_abc, t.zc);
  const Fp zb_inv = mul(inv_ab, t.za);
  const Fp za_inv = mul(inv_ab, t.zb);
  out[0] = t.ia ? aff_inf<Fp>() : jac_to_aff_with_zinv(a, za_inv);
  out[1] = t.ib ? aff_inf<Fp>() : jac_to_aff_with_zinv(b, zb_inv);
  out[2] = t.ic ? aff_inf<Fp>() : jac_to_aff_with_zinv(c, zc_inv);
}

}}  // namespace rabe::bn254
