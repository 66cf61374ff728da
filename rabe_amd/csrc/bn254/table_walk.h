// Fixed-base table walks: a canonical 256-bit scalar is cut into window digits and one table entry is taken per non-zero digit.
// Host + device, no runtime dependency: tests/hostsim/table_walk.cpp runs these cutters, the recoder and the loops on exact integers.
//   8-bit    32 windows, d = 1..255                       digit8, walk8:  step(window, digit)
//   16-bit   16 windows, d = 1..65535                     digit16, walk16: step(window, digit); walk16_two: two scalars through ONE loop
//                                                         of 2 x 16 steps, step(second, window, digit), for one call site of the group
//                                                         operation under both tables
//   signed   n windows of w bits, 1 <= |d| <= 2^(w-1)     scalar_bits + SignedRecoder; the three signed walks (engine_internal.h) keep
//                                                         their loops around it: a shared loop with a step changed their generated code
// What takes the entry (g1_madd_inl, jac_add_aff on G2, home_take on Gt) and where the accumulator lives (the step's capture, or the Gt
// home) is the caller's; so is the choice between an inlined and an out-of-line binding (engine_internal.h).  Every loop is
// `#pragma unroll 1`: a window's body is a whole group operation.
#pragma once
#include "curve.h"

namespace rabe { namespace bn254 {

constexpr int WALK8_WINDOWS = 32;
constexpr int WALK16_WINDOWS = 16;

// ---- digit cutters.  The word is picked by word_sel8's switch (curve.h): a runtime-indexed register array would go to scratch.
RB_HD uint32_t digit8(const uint32_t k[8], int w) { return (word_sel8(k, w >> 2) >> (8 * (w & 3))) & 255u; }
RB_HD uint32_t digit16(const uint32_t k[8], int w) {
  const uint32_t word = word_sel8(k, w >> 1);
  return (w & 1) ? (word >> 16) : (word & 0xffffu);
}
// bits b .. b + w - 1 of k (w <= 32); bits past 255 read as zero.  A window can straddle two words, so this is a switch of
// its own over word PAIRS, not two calls of word_sel8: the form the signed walks were compiled and measured with.
RB_HD uint32_t scalar_bits(const uint32_t k[8], int b, int w) {
  const int word = b >> 5, sh = b & 31;
  uint32_t lo, hi;
  switch (word) {
    case 0: lo = k[0]; hi = k[1]; break;
    case 1: lo = k[1]; hi = k[2]; break;
    case 2: lo = k[2]; hi = k[3]; break;
    case 3: lo = k[3]; hi = k[4]; break;
    case 4: lo = k[4]; hi = k[5]; break;
    case 5: lo = k[5]; hi = k[6]; break;
    case 6: lo = k[6]; hi = k[7]; break;
    default: lo = k[7]; hi = 0; break;
  }
  const uint64_t v = (((uint64_t)hi << 32) | lo) >> sh;
  return (uint32_t)v & ((1u << w) - 1u);
}

// ---- signed w-bit digits: k = sum_i d_i 2^(w i), -2^(w-1) < d_i <= 2^(w-1).  A window's bits plus the carry of the window below give
// raw in 0 .. 2^w; above half it stands for raw - 2^w and carries one into the next window (raw = 2^w: digit 0 and a carry).
struct SignedRecoder {
  int w;
  uint32_t half, carry;
  RB_HD explicit SignedRecoder(int w_) : w(w_), half(1u << (w_ - 1)), carry(0) {}
  // the magnitude |d_i| (0 .. 2^(w-1)) of the window whose bits are given; negative() then tells its sign
  RB_HD uint32_t next(uint32_t bits) {
    const uint32_t raw = bits + carry;
    carry = raw > half ? 1u : 0u;
    return carry ? (1u << w) - raw : raw;
  }
  RB_HD bool negative() const { return carry != 0; }
};

// ---- table geometry of the signed forms (T[i][|d|-1] = (|d| 2^(w i)) * base; the sign is applied to the entry on the fly).
// Wide tables (17 <= w <= 27, AC17's g): n = ceil(254 / w) windows of 2^(w-1) entries, the top one only needs 2^(254-w(n-1)) of them --
// a scalar below r < 2^254 leaves the top window at most that, carry included, and no carry leaves it.
RB_HD int wide_windows(int w) { return (254 + w - 1) / w; }
RB_HD size_t wide_count(int w, int i) {
  const int n = wide_windows(w);
  return (i < n - 1) ? ((size_t)1 << (w - 1)) : ((size_t)1 << (254 - w * (n - 1)));
}
RB_HD size_t wide_offset(int w, int i) { return (size_t)i << (w - 1); }   // windows below the top are full
// Tables with FULL windows (8 <= w <= 14; per-attribute bases of AW11): n = sgn_windows(w) windows of 2^(w-1) entries each.  n w >= 255,
// so the last carry always lands in a window.
RB_HD int sgn_windows(int w) { return (255 + w - 1) / w; }
RB_HD size_t sgn_entries(int w) { return (size_t)sgn_windows(w) << (w - 1); }

// ---- the loops: for (i = 0 .. n - 1) { mag = rec.next(scalar_bits(k, w i, w)); if (mag) take entry i, mag - 1, negated if rec.negative() }
// is the signed form, written out by its three users
template <class STEP>
RB_HD void walk8(const uint32_t k[8], STEP step) {
#pragma unroll 1
  for (int w = 0; w < WALK8_WINDOWS; w++) {
    const uint32_t d = digit8(k, w);
    if (d) step(w, d);
  }
}
template <class STEP>
RB_HD void walk16(const uint32_t k[8], STEP step) {
#pragma unroll 1
  for (int w = 0; w < WALK16_WINDOWS; w++) {
    const uint32_t d = digit16(k, w);
    if (d) step(w, d);
  }
}
// k1 then k2 in one loop; a zero k2 takes no step in the second half
template <class STEP>
RB_HD void walk16_two(const uint32_t k1[8], const uint32_t k2[8], STEP step) {
#pragma unroll 1
  for (int s = 0; s < 2 * WALK16_WINDOWS; s++) {
    const bool second = s >= WALK16_WINDOWS;
    const int w = s & (WALK16_WINDOWS - 1);
    const uint32_t d = digit16(second ? k2 : k1, w);
    if (d) step(second, w, d);
  }
}

}}  // namespace rabe::bn254
