// Chunking of the shared-doubling sums (k_msm_partial / k_gt_multiexp_partial, engine_jobs.hip), as a pure host function: no includes
// beyond <stddef.h> / <stdint.h>, so the tests' host build (tests/hostsim) exports exactly the arithmetic the engine runs.
#pragma once
#include <stddef.h>
#include <stdint.h>

// An item's max_terms terms are cut into L chunks of at most C terms; lane (chunk, item) sums its chunk with shared doublings and a
// finish kernel adds the L partial sums.  A lane pays its own 254 doublings / squarings (~1.8 k in G1, ~4 k in G2, ~4.6 k in Gt) plus
// ~1 k (G1) .. 4.6 k (Gt) per term: the rounds x lane-time model of choose_chunks with a 2 : 1 doubling-to-term ratio.  As long as
// n_items * max_terms lanes fit the chip in one round (64 lanes on each of the n_simds SIMDs) the answer is C = 1, L = max_terms.
static inline void rb_msm_chunks(size_t n_simds, size_t n_items, size_t max_terms, uint32_t* L, uint32_t* C) {
  if (max_terms < 1) max_terms = 1;
  if (n_simds < 1) n_simds = 1;
  double best = 0;
  size_t best_c = 1;
  for (size_t c = 1; c <= 256; c++) {
    const size_t l = (max_terms + c - 1) / c;
    const size_t c_eff = (max_terms + l - 1) / l;
    const size_t waves = (n_items * l + 63) / 64;
    const size_t rounds = (waves + n_simds - 1) / n_simds;
    const double cost = (double)rounds * (2.0 + (double)c_eff);
    if (best == 0 || cost < best) { best = cost; best_c = c; }
    if (l == 1) break;
  }
  const size_t l = (max_terms + best_c - 1) / best_c;
  *C = (uint32_t)((max_terms + l - 1) / l);
  *L = (uint32_t)l;
}
