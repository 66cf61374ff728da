// Randomness of a batch whose entry point draws in several RUNS over all its items -- rabe_ghw11_provision_packed: r_0 .. r_{n-1}, then
// z_0 .. z_{n-1} -- when the batch is cut into blocks of items that run side by side (pipeline.cpp: for_blocks).  The draw gate of
// `produce` orders ONE run (block after block); a second run would have to start after the LAST block's first, while the first blocks
// are already past it.  So the runs are drawn here, on the calling thread, before the blocks start: `draw()` is called runs * n times,
// run after run and item after item -- the order of the uncut call, whatever the cut -- and block [lo, hi) is handed its slice of every
// run, in run order: exactly what the entry point draws when it is given that block alone.  A block that never starts leaves nobody
// waiting: nothing is shared once the blocks run.
// Header-only and free of the engine, so that the order can be checked on a CPU (tests/native/predraw_blocks.cpp).
#pragma once
#include <stddef.h>

#include <vector>

namespace rabe {
namespace pipeline {

template <class V>
class RunDraws {
 public:
  template <class DRAW>
  RunDraws(size_t runs, size_t n, DRAW draw) : runs_(runs), n_(n), v_(runs * n) {
    for (auto& x : v_) x = draw();
  }
  ~RunDraws() { scrub(v_); }
  RunDraws(const RunDraws&) = delete;
  RunDraws& operator=(const RunDraws&) = delete;
  const V& at(size_t run, size_t item) const { return v_[run * n_ + item]; }
  // what block [lo, hi) draws: its items of run 0, then its items of run 1, ...
  std::vector<V> block(size_t lo, size_t hi) const {
    std::vector<V> t;
    t.reserve(runs_ * (hi - lo));
    for (size_t r = 0; r < runs_; r++) t.insert(t.end(), v_.begin() + (r * n_ + lo), v_.begin() + (r * n_ + hi));
    return t;
  }
  // the values are secrets of the call (r, z): zeroed when their holder is done with them
  static void scrub(std::vector<V>& t) {
    volatile unsigned char* p = (volatile unsigned char*)t.data();
    for (size_t i = 0; i < t.size() * sizeof(V); i++) p[i] = 0;
  }
 private:
  size_t runs_, n_;
  std::vector<V> v_;
};

}  // namespace pipeline
}  // namespace rabe
