// Variable-base scalar multiplication on G2 with a four-way split over the twist endomorphism (Galbraith / Scott 2008; GLS).
//
// psi = twist^-1 o Frobenius o twist (pairing.h: g2_frob1) acts on G2 -- the r-torsion of the twist -- as multiplication by p (the relation
// the membership tests of engine_jobs.hip rely on), so with lambda = p mod r
//     k P = k0 P + k1 psi(P) + k2 psi^2(P) + k3 psi^3(P),   k = k0 + k1 lambda + k2 lambda^2 + k3 lambda^3 (mod r),
// and the four signed sub-scalars are about a quarter of the length of k: one joint chain of ~66 doublings and the additions of the
// non-zero NAF digits of the four, against 254 doublings + ~127 additions of jac_mul_binary.  Whatever the rounding of the split, the
// relation above holds exactly, so the result is the same group element as `G2 * Fr` FOR POINTS OF G2; on a twist point outside G2 psi is
// not multiplication by p and the result is some other point (callers establish membership: rhip_g2_in_subgroup).
//
// The split (RB_HD: the same code runs on the host behind rabe_fr_split4): constants from tools/gen_constants.py (RB_GLS4_*).
#pragma once
#include "curve.h"
#include "pairing.h"

namespace rabe { namespace bn254 {

// words of NAF masks a sub-scalar needs: digits up to bit RB_GLS4_BITS
#define RB_GLS4_WORDS ((RB_GLS4_BITS + 32) / 32)
static_assert(RB_GLS4_WORDS <= 3, "gls4 masks are laid out for three words per sub-scalar");

// k < r (canonical) -> |k_i| as four little-endian words each and their signs
RB_HD void gls4_split(const uint32_t k[8], uint32_t mag[4][4], bool neg_[4]) {
  constexpr uint32_t GC[4][7] = RB_GLS4_G;
  constexpr uint32_t NC[4][4][4] = RB_GLS4_N;
  uint32_t kk[8];
#pragma unroll
  for (int i = 0; i < 8; i++) kk[i] = k[i];
  uint32_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int w = 0; w < 4; w++) acc[i][w] = i == 0 ? kk[w] : 0u;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    uint32_t g[7], prod[15];
#pragma unroll
    for (int w = 0; w < 7; w++) g[w] = GC[j][w];
    limbs_mul<8, 7>(kk, g, prod);
    // c = floor((k g + 2^255) / 2^256) mod 2^128: the carry of the rounding bit into word 8, then words 8 .. 11
    uint32_t c[4], carry = 0;
    (void)addc32(prod[7], 0x80000000u, carry);
#pragma unroll
    for (int w = 0; w < 4; w++) c[w] = addc32(prod[8 + w], 0u, carry);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t n[4], t[8];
#pragma unroll
      for (int w = 0; w < 4; w++) n[w] = NC[j][i][w];
      limbs_mul<4, 4>(c, n, t);
      uint32_t cy = 0;
#pragma unroll
      for (int w = 0; w < 4; w++) acc[i][w] = addc32(acc[i][w], t[w], cy);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    neg_[i] = (acc[i][3] >> 31) != 0;
    uint32_t borrow = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) mag[i][w] = neg_[i] ? subb32(0u, acc[i][w], borrow) : acc[i][w];
  }
}

// NAF masks of the four sub-scalars with their signs folded in: m[6 i + w] = positive digits of k_i (word w < 3), m[6 i + 3 + w] = negative
RB_HD void gls4_masks(const uint32_t k[8], uint32_t m[24]) {
  uint32_t mag[4][4];
  bool sg[4];
  gls4_split(k, mag, sg);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint32_t e[8], pos[8], ng[8];
#pragma unroll
    for (int w = 0; w < 8; w++) e[w] = w < 4 ? mag[i][w] : 0u;
    naf_masks(e, pos, ng);
#pragma unroll
    for (int w = 0; w < 3; w++) {
      m[6 * i + w] = sg[i] ? ng[w] : pos[w];
      m[6 * i + 3 + w] = sg[i] ? pos[w] : ng[w];
    }
  }
}

// The joint chain.  BASES provides  G2Aff base(int i) const  = psi^i(P), fetched where it is used (kept outside the register file, as
// jac_msm_naf takes its terms); m: the 24 mask words of the lane's scalar.  jac_add_aff handles an accumulator at infinity, equal to the
// addend (doubling) and opposite to it (infinity) -- all reachable here by chosen scalars (k = 1, 2, lambda +- 1, ...).
template <class BASES>
RB_FN G2Jac gls4_chain(BASES bases, const uint32_t* m) {
  G2Jac acc = jac_inf<Fp2>();
  bool started = false;
  for (int w = RB_GLS4_WORDS - 1; w >= 0; w--) {
    uint32_t pw[4], nw[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { pw[i] = m[6 * i + w]; nw[i] = m[6 * i + 3 + w]; }
    if (!started && !(pw[0] | pw[1] | pw[2] | pw[3] | nw[0] | nw[1] | nw[2] | nw[3])) continue;
    for (int b = 31; b >= 0; b--) {
      if (started) acc = jac_dbl(acc);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t pb = (pw[i] >> b) & 1u, nb = (nw[i] >> b) & 1u;
        if (pb | nb) {
          G2Aff q = bases.base(i);
          if (nb) q.y = fp2_neg(q.y);
          acc = jac_add_aff(acc, q);
          started = true;
        }
      }
    }
  }
  return acc;
}

}}  // namespace rabe::bn254
