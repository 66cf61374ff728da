// Bounds and buffer sizes of a device-planned Miller launch (engine_jobs.hip: run_pair_lists_mode, the ragged geometry), as a pure host
// function: no includes beyond <stddef.h> / <stdint.h>, so a host program (tests/hostsim/miller_plan_bounds.cpp) checks exactly the
// arithmetic the engine runs.  The neighbour of msm_chunks.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

// The plan (k_plan_choose) picks C pairs per chunk from [c_lo, c_hi]: no fewer than four rounds' worth of lanes need (more lanes only add
// shared squarings; a round is n_cu blocks of `block` lanes), no more than 64.  An item of p pairs then has ceil(p / C) chunks, so the work
// list holds at most total_pairs / C + n_items entries: the buffers are sized for the worst C of the range.
struct rb_miller_plan_sizes {
  size_t c_lo, c_hi;
  size_t w_max;                                 // entries of the work list, of the Miller values and lanes of the launch
  size_t plan_words, hist_words, off_words;     // 32-bit words of the plan, of the histogram [0 .. max_pairs + 1] and of chunk_off [n_items + 1], each rounded to 16 bytes
  size_t plan_bytes;                            // plan | hist | chunk_off | work list (8 bytes per entry)
  size_t ws_bytes;                              // running G2 points: 12 quads per pair slot, a wave's slots padded to C per lane
};
// needs 1 <= max_pairs, 1 <= n_items, total_pairs < n_items * max_pairs (what makes a batch ragged); plan_struct_bytes = sizeof(MillerPlan)
static inline rb_miller_plan_sizes rb_miller_plan_bounds(size_t n_cu, size_t block, size_t plan_struct_bytes, size_t n_items, size_t max_pairs, size_t total_pairs) {
  rb_miller_plan_sizes s;
  const size_t R = n_cu * block;
  s.c_lo = total_pairs / (4 * R);
  if (s.c_lo < 1) s.c_lo = 1;
  s.c_hi = max_pairs < 64 ? max_pairs : 64;
  if (s.c_lo > s.c_hi) s.c_lo = s.c_hi;
  s.w_max = total_pairs / s.c_lo + n_items + 64;
  s.hist_words = (max_pairs + 2 + 3) / 4 * 4;
  s.plan_words = (plan_struct_bytes / 4 + 3) / 4 * 4;
  s.off_words = (n_items + 1 + 3) / 4 * 4;
  s.plan_bytes = (s.plan_words + s.hist_words + s.off_words) * 4 + s.w_max * 8;
  s.ws_bytes = (total_pairs + n_items * (s.c_hi - 1) + 64 * s.c_hi + 64) * 12 * 16;
  return s;
}
