// Gt exponentiation with a four-way split over the Frobenius map.
//
// Frobenius acts on Gt -- the order-r subgroup of the cyclotomic subgroup -- as the power p, so with lambda = p mod r (the eigenvalue psi
// has on G2, bn254/gls4.h)
//     a^k = a^k0 * (a^p)^k1 * (a^p^2)^k2 * (a^p^3)^k3,   k = k0 + k1 lambda + k2 lambda^2 + k3 lambda^3 (mod r),
// and the four signed sub-scalars are below 2^RB_GLS4_BITS: one joint chain of at most 66 Granger-Scott squarings and one multiplication
// per non-zero NAF digit of the four (an inverse in Gt is a conjugation), against the 256 squarings + <= 72 multiplications of
// gt_pow_window (pairing.h).  Whatever the rounding of the split, the relation holds exactly, so the result is the same field element as
// gt_pow_window's FOR MEMBERS OF Gt; on a unitary element outside Gt Frobenius is not the power lambda and the result is some other
// element (callers establish membership: rhip_gt_is_member).
//
// The digits are the plain NAFs gls4_masks makes (no odd-power table: the masks, their layout and their once-per-scalar kernel are the
// ones the G2 chain already uses, and a chain then holds nothing but its accumulator and the one operand it is fetching).
#pragma once
#include "gls4.h"

namespace rabe { namespace bn254 {

// the 24 mask words of gls4_masks for ANY 256-bit scalar word (brought below r first: 2^256 / r < 5.3), for the exponent -k when `invert`
// (the positive and the negative digits change places)
RB_HD void gtpow4_masks(const uint32_t k[8], bool invert, uint32_t m[24]) {
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kk[i] = k[i];
  for (int t = 0; t < 5; t++) {
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = subb32(kk[i], FrParams::mod(i), borrow);
    if (borrow) break;
#pragma unroll
    for (int i = 0; i < 8; i++) kk[i] = d[i];
  }
  uint32_t g[24];
  gls4_masks(kk, g);
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int w = 0; w < 3; w++) {
      m[6 * i + w] = invert ? g[6 * i + 3 + w] : g[6 * i + w];
      m[6 * i + 3 + w] = invert ? g[6 * i + w] : g[6 * i + 3 + w];
    }
}

// The joint chain on an accumulator that lives outside the register file (the FA interface of pairing.h: LDS on the device).
// BASES provides  Y operand(int i, bool conj) const  with  Fp6 Y::half(int h) const  = the halves of a^(p^i), conjugated if `conj`,
// fetched where a multiplication consumes them (kept outside the register file, as gls4_chain keeps its bases); column i is
// fp12_frob{1,2,3} of column 0.  m: the 24 mask words of the scalar.  Returns whether the accumulator was started: false (every
// sub-scalar 0, i.e. k = 0 mod r) leaves the home untouched and stands for the value 1.  A started accumulator may pass through 1
// (k = lambda - 1 on a = 1, ...): a field multiplication has no special cases.
template <class FA, class BASES>
RB_FN bool gt_pow_split4(FA acc, BASES bases, const uint32_t* m) {
  bool started = false;
#pragma unroll 1
  for (int w = RB_GLS4_WORDS - 1; w >= 0; w--) {
    uint32_t pw[4], nw[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { pw[i] = m[6 * i + w]; nw[i] = m[6 * i + 3 + w]; }
    if (!started && !(pw[0] | pw[1] | pw[2] | pw[3] | nw[0] | nw[1] | nw[2] | nw[3])) continue;
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      if (started) facc_cyclotomic_sqr(acc);
      // bit i of dg: sub-scalar i has a digit here; bit i of sg: that digit is -1
      uint32_t dg = 0, sg = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t pb = (pw[i] >> b) & 1u, nb = (nw[i] >> b) & 1u;
        dg |= (pb | nb) << i;
        sg |= nb << i;
      }
#pragma unroll 1
      for (int i = 0; dg; i++, dg >>= 1, sg >>= 1) {
        if (!(dg & 1u)) continue;
        const auto y = bases.operand(i, (sg & 1u) != 0);
        if (started) facc_mul(acc, y);
        else { facc_set(acc, y); started = true; }
      }
    }
  }
  return started;
}

}}  // namespace rabe::bn254
