// The range bookkeeping of a store of fixed capacity whose entries take contiguous blocks (schemes.h: ghw11::TkStore -- a block is one G2
// element's prepared lines, a key of a attributes takes a + 2 of them).  Host only, no GPU dependency: tests/test_block_ranges.py compiles
// it alone.  The free blocks are kept as disjoint, non-adjacent ranges ordered by address; an allocation is FIRST FIT AT THE LOWEST
// ADDRESS, a release merges with the free neighbours on both sides.  There is no compaction: a request fails when no single free range
// holds it, whatever the free total.
#pragma once
#include <stdint.h>
#include <iterator>
#include <map>
#include <utility>
#include <vector>

namespace rabe {
namespace host {
class BlockRanges {
 public:
  explicit BlockRanges(uint64_t capacity = 0) : capacity_(capacity) {
    if (capacity) free_[0] = capacity;
  }
  uint64_t capacity() const { return capacity_; }
  uint64_t in_use() const { return capacity_ - free_total_(); }
  uint64_t largest_free() const {
    uint64_t best = 0;
    for (const auto& r : free_) if (r.second > best) best = r.second;
    return best;
  }
  // n blocks at the lowest address that has them: true and *first, or false with nothing changed (n = 0 is refused: an entry has blocks)
  bool alloc(uint64_t n, uint64_t* first) {
    if (!n) return false;
    for (auto it = free_.begin(); it != free_.end(); ++it) {
      if (it->second < n) continue;
      const uint64_t at = it->first, left = it->second - n;
      free_.erase(it);
      if (left) free_[at + n] = left;
      *first = at;
      return true;
    }
    return false;
  }
  // gives [first, first + n) back; false, with nothing changed, when the range is empty, leaves the capacity or touches a free block
  bool release(uint64_t first, uint64_t n) {
    if (!n || first > capacity_ || n > capacity_ - first) return false;
    auto next = free_.lower_bound(first);          // the first free range at or above `first`
    if (next != free_.end() && next->first < first + n) return false;
    auto prev = free_.end();
    if (next != free_.begin()) {
      prev = std::prev(next);
      if (prev->first + prev->second > first) return false;
    }
    uint64_t at = first, len = n;
    if (next != free_.end() && next->first == first + n) { len += next->second; free_.erase(next); }
    if (prev != free_.end() && prev->first + prev->second == first) { at = prev->first; len += prev->second; free_.erase(prev); }
    free_[at] = len;
    return true;
  }
  // the free ranges (first, count) by address, and the ranges in use between them, neighbours merged
  std::vector<std::pair<uint64_t, uint64_t>> free_ranges() const { return std::vector<std::pair<uint64_t, uint64_t>>(free_.begin(), free_.end()); }
  std::vector<std::pair<uint64_t, uint64_t>> used_ranges() const {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    uint64_t at = 0;
    for (const auto& r : free_) {
      if (r.first > at) out.push_back({at, r.first - at});
      at = r.first + r.second;
    }
    if (capacity_ > at) out.push_back({at, capacity_ - at});
    return out;
  }

 private:
  uint64_t free_total_() const {
    uint64_t t = 0;
    for (const auto& r : free_) t += r.second;
    return t;
  }
  uint64_t capacity_;
  std::map<uint64_t, uint64_t> free_;          // first block -> count
};
}  // namespace host
}  // namespace rabe
