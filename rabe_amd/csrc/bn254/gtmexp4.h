// Gt multi-exponentiation over width-4 signed windows:  prod_j x_j^(k_j)  with one shared chain of cyclotomic squarings.
//
// Every scalar is recoded into signed odd digits d in {+-1, +-3, +-5, +-7} (the width-4 non-adjacent form: a non-zero digit is followed by
// at least three zeros, density 1/5), every base gets the table x, x^3, x^5, x^7 (one cyclotomic squaring and three multiplications), and
// a non-zero digit then costs one table load, a conjugation for a negative digit (members of Gt are unitary) and one multiplication:
// ~51 multiplications per 254-bit term against the ~85 of the plain NAF walk (k_gt_multiexp_partial, engine_jobs.hip).  The squarings are
// Granger-Scott's and an inverse is a conjugate, so the bases must be members of Gt (the cyclotomic subgroup would do).
//
// Memory per term: the table is 4 x 384 = 1536 bytes (Montgomery form, kept outside the register file and fetched where a multiplication
// consumes an entry), the digits are 256 nibbles = 128 bytes per scalar.
//
// Host + device code: tests/hostsim/gt_multiexp_w4.cpp compiles this header for the CPU.
#pragma once
#include <stddef.h>
#include "pairing.h"

namespace rabe { namespace bn254 {

#define RB_GTMEXP4_WORDS 32          // digit words per scalar: 8 positions of 4 bits each
#define RB_GTMEXP4_TABLE 4           // table entries per base: x^1, x^3, x^5, x^7

// The digits of ANY 256-bit scalar word (brought below r first: 2^256 / r < 5.3), of -k when `invert`.  Position j takes nibble j & 7 of
// dg[j >> 3]: 0 = no digit, else bits 0..2 = |d| (1, 3, 5, 7: table entry |d| >> 1) and bit 3 = the digit is negative.
// The digits spell the representative of k mod r of smaller magnitude, k or k - r.  k = 0 (a multiple of r) has no digit at all.
// Why 256 positions are enough: let t be the top non-zero digit's position.  The digits below it are at least four positions apart and at
// most 7 in magnitude, so their sum is below 7 * 2^(t-4) * (1 + 1/16 + ...) < 2^(t-1); k > 0 makes d_t >= 1 and k > 2^t - 2^(t-1) =
// 2^(t-1).  With k < r < 2^254 that is t <= 254: the carry out of bit 253 lands on position 254 and nibble 255 stays empty.  The running
// value never exceeds k + 7 < 2^255, so adding 16 - u below cannot carry out of the eight limbs.
RB_HD void gtmexp4_digits(const uint32_t k_in[8], bool invert, uint32_t* dg) {
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = k_in[i];
  for (int t = 0; t < 5; t++) {
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = subb32(k[i], FrParams::mod(i), borrow);
    if (borrow) break;
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = d[i];
  }
  // the shorter of k and r - k, the sign folded into the digits (as k_naf_masks does): a Lagrange coefficient like -1 = r - 1 becomes the
  // one digit -1 instead of 254 bits of chain
  bool shortened = false;
  {
    uint32_t ng[8], borrow = 0, nz = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { ng[i] = subb32(FrParams::mod(i), k[i], borrow); nz |= k[i]; }
    bool less = false, decided = false;          // r - k < k ?
#pragma unroll
    for (int i = 7; i >= 0; i--)
      if (!decided && ng[i] != k[i]) { less = ng[i] < k[i]; decided = true; }
    if (nz && less) {
      shortened = true;
#pragma unroll
      for (int i = 0; i < 8; i++) k[i] = ng[i];
    }
  }
  const uint32_t flip = (invert != shortened) ? 8u : 0u;
#pragma unroll 1
  for (int w = 0; w < RB_GTMEXP4_WORDS; w++) {
    uint32_t word = 0;
#pragma unroll 1
    for (int b = 0; b < 8; b++) {
      if (k[0] & 1u) {
        const uint32_t u = k[0] & 15u;
        k[0] &= ~15u;
        uint32_t nib;
        if (u < 8u) {
          nib = u;                       // digit +u: the low four bits are simply cleared
        } else {
          nib = (16u - u) | 8u;          // digit -(16 - u): k += 16 - u, i.e. the cleared low bits and a carry into bit 4
          uint32_t c = 0;
          k[0] = addc32(k[0], 16u, c);
#pragma unroll
          for (int i = 1; i < 8; i++) k[i] = addc32(k[i], 0u, c);
        }
        word |= (nib ^ flip) << (4 * b);
      }
#pragma unroll
      for (int i = 0; i < 8; i++) k[i] = (k[i] >> 1) | (i < 7 ? (k[i + 1] << 31) : 0u);
    }
    dg[w] = word;
  }
}

// The table of one base on an accumulator that lives outside the register file (the FA interface of pairing.h).  SLOTS provides
//   Y entry(int i) const  -- entry i as a multiplicand (Fp6 Y::half(int h) const), fetched where a multiplication consumes it, and
//   void put(int i, const Fp12& v) const.
// Entry 0 holds x on entry.  Entry 3 carries x^2 until x^7 replaces it: one cyclotomic squaring and three multiplications, nothing but the
// accumulator held between the steps.
template <class FA, class SLOTS>
RB_FN void gt_mexp4_table(FA acc, SLOTS s) {
  facc_set(acc, s.entry(0));
  facc_cyclotomic_sqr(acc);
  s.put(3, facc_get(acc));          // x^2
  facc_mul(acc, s.entry(0));
  s.put(1, facc_get(acc));          // x^3
  facc_mul(acc, s.entry(3));
  s.put(2, facc_get(acc));          // x^5
  facc_mul(acc, s.entry(3));
  s.put(3, facc_get(acc));          // x^7
}

// One lane's chunk: prod_j x_j^(k_j) over the chunk's terms, the squarings shared.  TERMS provides
//   int count() const,  uint32_t digit_word(int j, int w) const  (word w of term j's digits),
//   Y entry(int j, int i, bool conj) const  (entry i of term j's table, conjugated if `conj`).
// Returns whether the accumulator was started: false (no term, or every scalar 0 mod r) leaves the home untouched and stands for 1.
template <class FA, class TERMS>
RB_FN bool gt_mexp4_chunk(FA acc, TERMS terms) {
  const int cnt = terms.count();
  bool started = false;
#pragma unroll 1
  for (int w = RB_GTMEXP4_WORDS - 1; w >= 0; w--) {
    if (!started) {          // leading zero digits cost nothing
      uint32_t any = 0;
      for (int j = 0; j < cnt; j++) any |= terms.digit_word(j, w);
      if (!any) continue;
    }
#pragma unroll 1
    for (int b = 7; b >= 0; b--) {
      if (started) facc_cyclotomic_sqr(acc);
#pragma unroll 1
      for (int j = 0; j < cnt; j++) {
        const uint32_t nib = (terms.digit_word(j, w) >> (4 * b)) & 15u;
        if (!nib) continue;
        const auto y = terms.entry(j, (int)((nib & 7u) >> 1), (nib & 8u) != 0);
        if (started) facc_mul(acc, y);
        else { facc_set(acc, y); started = true; }
      }
    }
  }
  return started;
}

// Chunking for the windowed walk, the sibling of rb_msm_chunks (msm_chunks.h): an item's max_terms terms are cut into L chunks of at most
// C, lane (chunk, item).  A lane pays its own chain of ~254 cyclotomic squarings plus its terms' multiplications.  rb_msm_chunks weighs a
// chain as 2 terms of the NAF walk; the chain is the same here and the instrumented counts (docs/kernels.md) put a term at 2 775 Fp
// multiplications against the NAF walk's 4 613, so a chain weighs 2 x 4 613 / 2 775 = 3.32 of these terms.  rounds x lane time, as
// rb_msm_chunks.
static inline void rb_gtmexp4_chunks(size_t n_simds, size_t n_items, size_t max_terms, uint32_t* L, uint32_t* C) {
  if (max_terms < 1) max_terms = 1;
  if (n_simds < 1) n_simds = 1;
  double best = 0;
  size_t best_c = 1;
  for (size_t c = 1; c <= 256; c++) {
    const size_t l = (max_terms + c - 1) / c;
    const size_t c_eff = (max_terms + l - 1) / l;
    const size_t waves = (n_items * l + 63) / 64;
    const size_t rounds = (waves + n_simds - 1) / n_simds;
    const double cost = (double)rounds * (3.32 + (double)c_eff);
    if (best == 0 || cost < best) { best = cost; best_c = c; }
    if (l == 1) break;
  }
  const size_t l = (max_terms + best_c - 1) / best_c;
  *C = (uint32_t)((max_terms + l - 1) / l);
  *L = (uint32_t)l;
}

}}  // namespace rabe::bn254
