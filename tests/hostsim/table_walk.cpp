// TEST INFRASTRUCTURE: the digit cutters, the signed recoder, the table geometry and the walk loops (the signed
// loop as its users write it out around the recoder) of rabe_amd/csrc/bn254/table_walk.h on
// the CPU, with exact integers as the "group": a step adds +-digit 2^(w window) into a limb array, and the sum has to be the scalar.
// Stand-alone (own main, no Python loading): it can be built with a host sanitizer.  Driven by tests/test_table_walk_host.py, which
// makes the scalars.
//
// stdin:  records of 32 bytes, canonical scalars below r, little-endian.
// stdout: one line, "<scalars> <steps>".
// exit:   0 when every check holds, 1 otherwise (the first failures are named on stderr), 2 on malformed input.
// Checked for every scalar k (and, for the two-scalar walks, k with the next scalar and k with 0):
//   8-bit, 16-bit walks      sum d_i 2^(w i) == k, 1 <= d_i <= 2^w - 1, windows in increasing order
//   signed, full windows     w = 8 .. 14, n = sgn_windows(w): sum +-mag_i 2^(w i) == k, 1 <= mag_i <= 2^(w-1),
//                            (i << (w-1)) + mag_i - 1 < sgn_entries(w), carry out 0
//   signed, wide windows     w = 20, 24, 26, n = wide_windows(w): the same sum, mag_i - 1 < wide_count(w, i), wide_offset(w, i) + mag_i - 1
//                            below the table's size, carry out 0
//   two-scalar 16-bit walk   the first-half steps sum to k1, the second-half steps to k2; k2 = 0 takes no second-half step
#include "../../rabe_amd/csrc/bn254/table_walk.h"
#include <stdio.h>
#include <string.h>

using namespace rabe::bn254;

static size_t failures = 0, steps = 0;
static void fail(const char* what, size_t rec, int w, int i) {
  if (failures++ < 16) fprintf(stderr, "table_walk: record %zu: %s (w = %d, window %d)\n", rec, what, w, i);
}
// an exact signed sum of terms +-m 2^b, b < 288, m < 2^27: ten limbs of 32 bits held in int64 (a limb takes at most a few hundred terms
// below 2^59), normalised at the end
struct Sum {
  long long l[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  void add(uint32_t m, int bit, bool negative) {
    const long long t = (long long)((unsigned long long)m << (bit & 31));
    l[bit >> 5] += negative ? -t : t;
  }
  bool equals(const uint32_t k[8]) const {
    long long c = 0;
    for (int i = 0; i < 10; i++) {
      const long long v = l[i] + c;
      const uint32_t low = (uint32_t)(v & 0xffffffffll);
      c = (v - (long long)low) / 4294967296ll;          // exact: v - low is a multiple of 2^32
      if (low != (i < 8 ? k[i] : 0u)) return false;
    }
    return c == 0;
  }
};

static void check_plain(size_t rec, const uint32_t k[8]) {
  {
    Sum s;
    int last = -1;
    walk8(k, [&](int w, uint32_t d) {
      steps++;
      if (d < 1 || d > 255u) fail("8-bit digit out of range", rec, 8, w);
      if (w <= last || w >= WALK8_WINDOWS) fail("8-bit windows out of order", rec, 8, w);
      if (d != digit8(k, w)) fail("8-bit digit is not digit8", rec, 8, w);
      last = w;
      s.add(d, 8 * w, false);
    });
    if (!s.equals(k)) fail("8-bit digits do not sum to the scalar", rec, 8, -1);
  }
  {
    Sum s;
    int last = -1;
    walk16(k, [&](int w, uint32_t d) {
      steps++;
      if (d < 1 || d > 65535u) fail("16-bit digit out of range", rec, 16, w);
      if (w <= last || w >= WALK16_WINDOWS) fail("16-bit windows out of order", rec, 16, w);
      if (d != digit16(k, w)) fail("16-bit digit is not digit16", rec, 16, w);
      last = w;
      s.add(d, 16 * w, false);
    });
    if (!s.equals(k)) fail("16-bit digits do not sum to the scalar", rec, 16, -1);
  }
}
static void check_signed(size_t rec, const uint32_t k[8], int w, bool wide) {
  const int n = wide ? wide_windows(w) : sgn_windows(w);
  const size_t total = wide ? wide_offset(w, n - 1) + wide_count(w, n - 1) : sgn_entries(w);
  Sum s;
  int last = -1;
  SignedRecoder sd(w);          // the loop the three signed walks of engine_internal.h write out around the recoder
  for (int i = 0; i < n; i++) {
    const uint32_t mag = sd.next(scalar_bits(k, w * i, w));
    if (!mag) continue;
    const bool negative = sd.negative();
    steps++;
    if (mag < 1 || mag > (1u << (w - 1))) fail("signed magnitude out of range", rec, w, i);
    if (i <= last || i >= n) fail("signed windows out of order", rec, w, i);
    last = i;
    const size_t index = (wide ? wide_offset(w, i) : ((size_t)i << (w - 1))) + (mag - 1);
    if (index >= total) fail("signed index past the table", rec, w, i);
    if (wide && (size_t)(mag - 1) >= wide_count(w, i)) fail("wide magnitude past its window's entries", rec, w, i);
    s.add(mag, w * i, negative);
  }
  if (sd.carry != 0) fail("a carry leaves the last window", rec, w, n - 1);
  if (!s.equals(k)) fail("signed digits do not sum to the scalar", rec, w, -1);
}
static void check_two(size_t rec, const uint32_t k1[8], const uint32_t k2[8]) {
  const bool k2_zero = (k2[0] | k2[1] | k2[2] | k2[3] | k2[4] | k2[5] | k2[6] | k2[7]) == 0;
  {
    Sum s[2];
    int last[2] = {-1, -1};
    bool seen_second = false;
    walk16_two(k1, k2, [&](bool second, int w, uint32_t d) {
      steps++;
      if (d < 1 || d > 65535u || w <= last[second] || w >= WALK16_WINDOWS) fail("two-scalar 16-bit step out of range", rec, 16, w);
      if (!second && seen_second) fail("two-scalar 16-bit walk returns to the first scalar", rec, 16, w);
      seen_second |= second;
      last[second] = w;
      s[second].add(d, 16 * w, false);
    });
    if (!s[0].equals(k1) || !s[1].equals(k2)) fail("two-scalar 16-bit digits do not sum to the scalars", rec, 16, -1);
    if (k2_zero && seen_second) fail("a zero second scalar takes a step", rec, 16, -1);
  }
}

int main() {
  static const int wide_bits[3] = {20, 24, 26};
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t first[8], prev[8], k[8];
  size_t got, n = 0;
  while ((got = fread(k, 1, sizeof(k), stdin)) == sizeof(k)) {
    check_plain(n, k);
    for (int w = 8; w <= 14; w++) check_signed(n, k, w, false);
    for (int j = 0; j < 3; j++) check_signed(n, k, wide_bits[j], true);
    check_two(n, k, zero);
    if (n) check_two(n, prev, k); else memcpy(first, k, sizeof(k));
    memcpy(prev, k, sizeof(k));
    n++;
  }
  if (got != 0) {
    fprintf(stderr, "table_walk: input is not a whole number of 32-byte records\n");
    return 2;
  }
  if (n) check_two(n, prev, first);
  // the geometry on its own: the windows cover the scalar's bits and the top wide window holds what is left of 254 bits
  for (int w = 8; w <= 14; w++)
    if (sgn_windows(w) * w < 255 || (sgn_windows(w) - 1) * w >= 255) fail("sgn_windows does not cover 255 bits", 0, w, -1);
  for (int w = 17; w <= 27; w++) {
    const int nw = wide_windows(w);
    if (nw * w < 254 || (nw - 1) * w >= 254) fail("wide_windows does not cover 254 bits", 0, w, -1);
    if (wide_count(w, nw - 1) > wide_count(w, 0)) fail("the top wide window is larger than a full one", 0, w, nw - 1);
  }
  printf("%zu %zu\n", n, steps);
  fprintf(stderr, "table_walk: %zu scalars, %zu steps, %zu failures\n", n, steps, failures);
  return failures ? 1 : 0;
}
