// Host check of rb_miller_plan_bounds (rabe_amd/csrc/miller_plan.h): the bounds and buffer sizes of a device-planned Miller launch, for the
// pair counts of tests/decrypt_launch_cases.py and for the extremes.  A program of its own (tests/test_miller_plan_bounds_host.py builds it
// plain and with the address and undefined-behaviour sanitizers); prints the number of checks it made, exits 1 on the first that fails.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../rabe_amd/csrc/miller_plan.h"

typedef unsigned __int128 u128;
static long checks = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    checks++;                                                                            \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); exit(1); }         \
  } while (0)

static const size_t BLOCK = 256, PLAN_BYTES = 16 + 2 * 66 * 4;          // RB_MILLER_BLOCK and sizeof(MillerPlan): any value serves the arithmetic

// the sizes in 128 bits: what the 64-bit arithmetic must equal (no step may wrap)
static void check_no_wrap(size_t n_cu, size_t n, size_t mx, size_t total, const rb_miller_plan_sizes& s) {
  const u128 w = (u128)total / s.c_lo + n + 64;
  CHECK(w == s.w_max);
  const u128 words = (u128)s.plan_words + s.hist_words + s.off_words;
  CHECK((u128)s.hist_words >= (u128)mx + 2 && (u128)s.off_words >= (u128)n + 1 && s.plan_words * 4 >= PLAN_BYTES);
  CHECK(words * 4 + w * 8 == s.plan_bytes);
  CHECK(((u128)total + (u128)n * (s.c_hi - 1) + 64 * (u128)s.c_hi + 64) * 12 * 16 == s.ws_bytes);
  CHECK((u128)4 * n_cu * BLOCK == (u128)(4 * n_cu * BLOCK));
}
// pairs: the pair count of every item (sum = total_pairs, max <= max_pairs)
static void check_shape(size_t n_cu, size_t mx, const std::vector<uint32_t>& pairs) {
  size_t total = 0;
  for (uint32_t p : pairs) { total += p; CHECK(p <= mx); }
  const size_t n = pairs.size();
  CHECK(mx >= 1 && n >= 1 && total >= 1 && total < n * mx);          // what sends a batch down the planned branch
  const rb_miller_plan_sizes s = rb_miller_plan_bounds(n_cu, BLOCK, PLAN_BYTES, n, mx, total);
  CHECK(1 <= s.c_lo && s.c_lo <= s.c_hi && s.c_hi <= 64 && s.c_hi <= mx);
  check_no_wrap(n_cu, n, mx, total, s);
  for (size_t c = s.c_lo; c <= s.c_hi; c++) {
    size_t chunks = 0, slots = 0;          // entries of the work list; pair slots when every lane of a wave is padded to c
    for (uint32_t p : pairs) chunks += (p + c - 1) / c;
    slots = (chunks + 63) / 64 * 64 * c;
    CHECK(chunks <= s.w_max);
    CHECK(slots * 12 * 16 <= s.ws_bytes);          // k_miller_multi: wave w of the list owns quads [w * c * 12 * 64, ...)
  }
}
// the same bounds without a list of items: n items, total pairs (the worst list has ceil(total / c) + n chunks at most)
static void check_extreme(size_t n_cu, size_t n, size_t mx, size_t total) {
  const rb_miller_plan_sizes s = rb_miller_plan_bounds(n_cu, BLOCK, PLAN_BYTES, n, mx, total);
  CHECK(1 <= s.c_lo && s.c_lo <= s.c_hi && s.c_hi <= 64);
  check_no_wrap(n_cu, n, mx, total, s);
  for (size_t c = s.c_lo; c <= s.c_hi; c++) {
    const u128 chunks = (u128)total / c + n;          // sum ceil(p_i / c) <= sum (p_i / c + 1)
    CHECK(chunks <= s.w_max);
    CHECK(((u128)total + (u128)n * (c - 1) + 63 * (u128)c) * 12 * 16 <= s.ws_bytes);
  }
}

int main() {
  const size_t cus[] = {1, 64, 256, 304};
  for (size_t n_cu : cus) {
    // the contract's ragged shapes: leaves per item [1, 3, 2, 4, 1], 65 items of 1 + i % 3 leaves with 4 in the last, [2, 0, 1];
    // pairs per item = leaves + 1 (LSW, AW11), leaves + 2 (GHW11), 2 leaves + 1 (BSW)
    const std::vector<uint32_t> ragged5 = {1, 3, 2, 4, 1}, empty = {2, 0, 1};
    std::vector<uint32_t> tiled65;
    for (uint32_t i = 0; i < 64; i++) tiled65.push_back(1 + i % 3);
    tiled65.push_back(4);
    const std::vector<const std::vector<uint32_t>*> shapes = {&ragged5, &tiled65, &empty};
    for (const std::vector<uint32_t>* leaves : shapes)
      for (uint32_t per_leaf = 1; per_leaf <= 2; per_leaf++)
        for (uint32_t other = 1; other <= 2; other++) {
          std::vector<uint32_t> pairs;
          uint32_t mx = 0;
          for (uint32_t m : *leaves) { pairs.push_back(per_leaf * m + other); mx = pairs.back() > mx ? pairs.back() : mx; }
          check_shape(n_cu, mx, pairs);
        }
    // one pair against many: max_pairs of 2, 63, 64, 65 and 201, one item at the maximum and the others at one pair
    for (uint32_t mx : {2u, 63u, 64u, 65u, 201u})
      for (size_t n : {(size_t)2, (size_t)65, (size_t)4097}) {
        std::vector<uint32_t> pairs(n, 1);
        pairs.back() = mx;
        check_shape(n_cu, mx, pairs);
        std::vector<uint32_t> nearly(n, mx);          // total_pairs just under n_items * max_pairs
        nearly[0] = mx - 1;
        check_shape(n_cu, mx, nearly);
      }
    // extremes by count alone: one item cannot be ragged unless it claims fewer pairs than max_pairs; the largest batches 32-bit offsets allow
    check_extreme(n_cu, 1, 2, 1);
    check_extreme(n_cu, 1, 64, 63);
    check_extreme(n_cu, 1, 1000, 999);
    check_extreme(n_cu, 2, 1, 1);          // max_pairs of 1: an item without pairs beside one with its pair
    check_extreme(n_cu, 0xFFFFFFFFull, 1, 0xFFFFFFFEull);
    check_extreme(n_cu, 0xFFFFFFFFull, 64, 0xFFFFFFFFull);
    check_extreme(n_cu, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull);
    check_extreme(n_cu, 0x4000000ull, 64, 0xFFFFFFFFull);          // total_pairs just under n_items * max_pairs at the 32-bit edge
  }
  printf("%ld checks\n", checks);
  return 0;
}
