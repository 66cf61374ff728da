"""The range bookkeeping of the GHW11 key store by itself (rabe_amd/csrc/host/block_ranges.h), without a GPU: a stand-alone program with its
own main is compiled around the header with the host compiler under -fsanitize=address,undefined and run as a plain child process.  It
checks first fit at the lowest address, merging of freed neighbours on both sides, refusal when the free total suffices but no contiguous
range does, refusal of releases that are not ranges in use, and 4000 pseudo-random allocations and releases (fixed seed) against a bitmap
model, ending with everything released and one free range of the full capacity."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "block_ranges.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
using rabe::host::BlockRanges;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
typedef std::vector<std::pair<uint64_t, uint64_t>> Ranges;

static int first_fit_and_merging() {
  BlockRanges r(16);
  uint64_t a = 99, b = 99, c = 99, d = 99;
  CHECK(r.capacity() == 16 && r.in_use() == 0 && r.largest_free() == 16);
  CHECK(r.alloc(3, &a) && a == 0);
  CHECK(r.alloc(5, &b) && b == 3);
  CHECK(r.alloc(4, &c) && c == 8);
  CHECK(r.in_use() == 12 && r.largest_free() == 4);
  CHECK((r.used_ranges() == Ranges{{0, 12}}) && (r.free_ranges() == Ranges{{12, 4}}));
  // a hole between two live ranges: the lowest address that fits wins, not the tail
  CHECK(r.release(3, 5));
  CHECK(r.in_use() == 7 && r.largest_free() == 5);
  CHECK(r.alloc(4, &d) && d == 3);
  CHECK(r.in_use() == 11 && r.largest_free() == 4);
  CHECK((r.free_ranges() == Ranges{{7, 1}, {12, 4}}));
  // 5 blocks free in all, no 5 contiguous: refused, nothing changed
  uint64_t e = 77;
  CHECK(!r.alloc(5, &e) && e == 77);
  CHECK(r.in_use() == 11 && (r.free_ranges() == Ranges{{7, 1}, {12, 4}}));
  CHECK(!r.alloc(0, &e));
  // a release merges with the free neighbour above, below, and on both sides
  CHECK(r.release(3, 4));
  CHECK((r.free_ranges() == Ranges{{3, 5}, {12, 4}}));
  CHECK(r.alloc(5, &e) && e == 3);
  CHECK(r.release(8, 4));
  CHECK((r.free_ranges() == Ranges{{8, 8}}));
  CHECK(r.release(3, 5));
  CHECK((r.free_ranges() == Ranges{{3, 13}}));
  CHECK(r.alloc(2, &e) && e == 3);
  CHECK(r.alloc(2, &e) && e == 5);
  CHECK(r.alloc(2, &e) && e == 7);
  CHECK(r.release(3, 2) && r.release(7, 2));
  CHECK((r.free_ranges() == Ranges{{3, 2}, {7, 9}}));
  CHECK(r.release(5, 2));          // both sides at once
  CHECK((r.free_ranges() == Ranges{{3, 13}}));
  // what is not a range in use is refused and changes nothing
  CHECK(!r.release(3, 1) && !r.release(2, 2) && !r.release(0, 0) && !r.release(15, 2) && !r.release(17, 1) && !r.release(1, ~0ull));
  CHECK((r.free_ranges() == Ranges{{3, 13}}) && (r.used_ranges() == Ranges{{0, 3}}));
  CHECK(r.release(0, 3));
  CHECK((r.free_ranges() == Ranges{{0, 16}}) && r.used_ranges().empty() && r.largest_free() == 16);
  BlockRanges none(0);
  CHECK(none.capacity() == 0 && none.largest_free() == 0 && !none.alloc(1, &e) && none.used_ranges().empty());
  return 0;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {          // xorshift64*, fixed seed
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static int against_a_bitmap() {
  const uint64_t cap = 257;
  BlockRanges r(cap);
  std::vector<char> used(cap, 0);
  struct Live { uint64_t first, n; };
  std::vector<Live> live;
  for (int step = 0; step < 4000; step++) {
    if (live.empty() || rnd() % 5 < 3) {
      const uint64_t n = 1 + rnd() % 23;
      uint64_t want = cap;          // the model: the lowest run of n clear bits
      for (uint64_t at = 0, run = 0; at < cap; at++) {
        run = used[at] ? 0 : run + 1;
        if (run == n) { want = at + 1 - n; break; }
      }
      uint64_t got = cap + 1;
      const bool ok = r.alloc(n, &got);
      CHECK(ok == (want != cap));
      if (ok) {
        CHECK(got == want);
        for (uint64_t k = 0; k < n; k++) used[got + k] = 1;
        live.push_back({got, n});
      }
    } else {
      const size_t j = rnd() % live.size();
      CHECK(r.release(live[j].first, live[j].n));
      CHECK(!r.release(live[j].first, live[j].n));          // twice is refused
      for (uint64_t k = 0; k < live[j].n; k++) used[live[j].first + k] = 0;
      live[j] = live.back();
      live.pop_back();
    }
    uint64_t in_use = 0, best = 0, run = 0;
    for (uint64_t at = 0; at < cap; at++) { in_use += used[at]; run = used[at] ? 0 : run + 1; if (run > best) best = run; }
    CHECK(r.in_use() == in_use && r.largest_free() == best);
    uint64_t covered = 0;
    for (const auto& u : r.used_ranges()) {
      for (uint64_t k = 0; k < u.second; k++) CHECK(used[u.first + k]);
      covered += u.second;
    }
    CHECK(covered == in_use);
  }
  while (!live.empty()) { CHECK(r.release(live.back().first, live.back().n)); live.pop_back(); }
  CHECK((r.free_ranges() == Ranges{{0, cap}}) && r.in_use() == 0 && r.largest_free() == cap);
  return 0;
}
int main() {
  if (first_fit_and_merging() || against_a_bitmap()) return 1;
  puts("block ranges: ok");
  return 0;
}
"""


def test_block_ranges_under_the_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "block_ranges_main.cpp", tmp_path / "block_ranges_main"
    src.write_text(PROGRAM)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           os.path.join(ROOT, "rabe_amd", "csrc", "host"), str(src), "-o", str(exe)]
    # the sanitizers' runtimes inside the program where the compiler has them as archives (GCC): the program then starts the same way
    # whatever else the environment loads into a process
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL, timeout=300).returncode != 0:
        subprocess.run(cmd, check=True, timeout=300)
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)          # a plain child process
    assert run.returncode == 0, run.stderr.decode()
    assert run.stdout.decode().strip() == "block ranges: ok"
