// The draw order of a packed call with TWO runs of draws (rabe_ghw11_provision_packed: r_0 .. r_{n-1}, then z_0 .. z_{n-1}) that is cut
// into blocks running side by side -- rabe_amd/csrc/host/predraw.h, checked without a device.  Stand-alone: its own main, no engine, no
// Python.  Meant to be built with the thread sanitizer and run directly on a CPU machine:
//
//   c++ -std=c++17 -O1 -g -fsanitize=thread -pthread -I rabe_amd/csrc/host tests/native/predraw_blocks.cpp -o predraw_blocks && ./predraw_blocks
//
// (tests/test_device_group_surface.py builds it WITHOUT a sanitizer and runs it, so the order is checked with every suite run.)
//
// For every cut the device group makes -- n items over e engines, the rule of pipeline.cpp's `cut`: sizes differ by at most one, blocks in
// engine order, fewer items than engines: one each -- a counting source is drawn 2 n times on the calling thread; then one std::thread
// per block replays its slices, except ONE block that never starts (a worker that fails before its block: nobody may wait for it).
// Checked: the program finishes; the source was drawn r in block order, then z in block order (= 0 .. 2n-1 in item order); block
// [lo, hi) saw r_lo .. r_{hi-1}, then z_lo .. z_{hi-1}; the values handed out are zeroed by scrub.
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

#include "predraw.h"

using rabe::pipeline::RunDraws;

struct Block { size_t lo, hi; };
static std::vector<Block> cut(size_t engines, size_t n) {
  const size_t chunks = n < engines ? (n ? n : 1) : engines, base = n / chunks, extra = n % chunks;
  std::vector<Block> b;
  for (size_t k = 0, at = 0; k < chunks; k++) {
    const size_t len = base + (k < extra ? 1 : 0);
    b.push_back({at, at + len});
    at += len;
  }
  return b;
}

static std::atomic<int> failures{0};
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void one_case(size_t engines, size_t n, size_t dead) {
  uint64_t counter = 0;
  std::vector<uint64_t> drawn;                                  // the order in which the one source was asked
  RunDraws<uint64_t> draws(2, n, [&] { drawn.push_back(counter); return 1000 + counter++; });
  EXPECT(drawn.size() == 2 * n, "drew %zu values for %zu items", drawn.size(), n);
  for (size_t i = 0; i < drawn.size(); i++) EXPECT(drawn[i] == i, "draw %zu came %llu-th", i, (unsigned long long)drawn[i]);
  const auto blocks = cut(engines, n);
  EXPECT(blocks.back().hi == n, "the cut does not cover the items");
  std::vector<std::vector<uint64_t>> seen(blocks.size());
  std::vector<std::thread> th;
  for (size_t k = 0; k < blocks.size(); k++) {
    if (k == dead) continue;                                    // this worker failed before its block started
    th.emplace_back([&, k] {
      std::vector<uint64_t> tape = draws.block(blocks[k].lo, blocks[k].hi);
      seen[k] = tape;                                           // what the entry point draws from its tape, front to back
      RunDraws<uint64_t>::scrub(tape);
      for (uint64_t v : tape) EXPECT(v == 0, "a scrubbed tape still holds %llu", (unsigned long long)v);
    });
  }
  for (auto& t : th) t.join();
  for (size_t k = 0; k < blocks.size(); k++) {
    if (k == dead) { EXPECT(seen[k].empty(), "the block that never started drew"); continue; }
    const size_t lo = blocks[k].lo, len = blocks[k].hi - lo;
    EXPECT(seen[k].size() == 2 * len, "block %zu of %zu items drew %zu values", k, len, seen[k].size());
    for (size_t i = 0; i < len && seen[k].size() == 2 * len; i++) {
      EXPECT(seen[k][i] == 1000 + lo + i, "block %zu: r of item %zu is draw %llu", k, lo + i, (unsigned long long)(seen[k][i] - 1000));
      EXPECT(seen[k][len + i] == 1000 + n + lo + i, "block %zu: z of item %zu is draw %llu", k, lo + i, (unsigned long long)(seen[k][len + i] - 1000));
      EXPECT(draws.at(0, lo + i) == seen[k][i] && draws.at(1, lo + i) == seen[k][len + i], "block %zu: at() and block() disagree", k);
    }
  }
}

int main() {
  const size_t cases[][2] = {{2, 5}, {3, 5}, {3, 2}, {8, 21}, {4, 4}, {1, 3}};
  for (const auto& c : cases) {
    const size_t blocks = cut(c[0], c[1]).size();
    for (size_t dead = 0; dead <= blocks; dead++) one_case(c[0], c[1], dead);          // dead = blocks: every block runs
  }
  if (failures) { fprintf(stderr, "%d failure(s)\n", failures.load()); return 1; }
  printf("predraw_blocks ok\n");
  return 0;
}
