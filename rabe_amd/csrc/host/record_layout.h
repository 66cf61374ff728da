// What the record writer of a packed issuing call is told, free of the engine's headers (tests/hostsim/record_sources_check.cpp runs it alone
// on a CPU, plain and under the sanitizers): the shape of a record (RecordLayout), where every item's parts lie (RecordSources) and how large
// the output becomes (record_offsets).  records.h has the functions that take them to the device.
#pragma once
#include <stddef.h>

#include <type_traits>
#include <vector>

#include "bytes.h"

namespace rabe { namespace schemes {

// the fixed part of one record shape (everything but the sealed plaintext and its u32 length): byte b is a literal or byte `o` of
// the item's part in source k (include/rabe_hip.h: rhip_assemble_records)
struct RecordLayout {
  std::vector<uint32_t> map;
  struct Part { uint32_t rec_off, len, k, part_off; };
  std::vector<Part> parts;
  void lit(const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for (size_t i = 0; i < n; i++) map.push_back(0xFF000000u | b[i]); }
  void u8(uint8_t v) { map.push_back(0xFF000000u | v); }
  void u32(uint32_t v) { for (int i = 0; i < 4; i++) map.push_back(0xFF000000u | ((v >> (8 * i)) & 0xFFu)); }
  void str(const std::string& s) { u32((uint32_t)s.size()); lit(s.data(), s.size()); }
  void src(uint32_t k, uint32_t off, uint32_t len) {
    parts.push_back({(uint32_t)map.size(), len, k, off});
    for (uint32_t i = 0; i < len; i++) map.push_back((k << 24) | (off + i));
  }
  size_t bytes() const { return map.size(); }
};

// The end of a ciphertext layout: what a record of it takes without its sealed bytes -- the layout and the u32 length of the sealed part --
// which is what record_offsets is told.  A key encapsulation has no sealed source: its layout ends in that length field, zero.
inline size_t close_ciphertext(RecordLayout& L, bool kem) {
  const size_t fixed = L.bytes() + 4;
  if (kem) L.u32(0);
  return fixed;
}

// The sources of the n records of one call: source k is a device array and a rule that says where item i's part of it starts.  Three rules:
//   by_item   base + stride * i                       one element (or a fixed group) per item
//   by_rows   base + stride * row_off[i]              a ragged array; row_off is the prefix array of the items' row counts, n + 1 entries
//   at_bytes  base + byte_off[i]                      explicit byte offsets, n entries
// dev_src / item_off are the two arrays rhip_assemble_records takes: item_off[k * n + i], every product in 64 bits.
struct RecordSources {
  explicit RecordSources(size_t n_items) : n(n_items) {}
  const size_t n;
  std::vector<const void*> dev_src;
  std::vector<uint64_t> item_off;
  RecordSources& by_item(const void* base, uint64_t stride) {
    dev_src.push_back(base);
    for (size_t i = 0; i < n; i++) item_off.push_back(stride * (uint64_t)i);
    return *this;
  }
  template <class T>
  RecordSources& by_rows(const void* base, uint64_t stride, const T* row_off, size_t entries) {
    static_assert(std::is_same<T, uint32_t>::value || std::is_same<T, size_t>::value, "a prefix array of uint32_t or size_t");
    if (entries != n + 1) throw RabeError("RecordSources: a prefix array of rows has n + 1 entries");
    dev_src.push_back(base);
    for (size_t i = 0; i < n; i++) item_off.push_back(stride * (uint64_t)row_off[i]);
    return *this;
  }
  template <class T>
  RecordSources& by_rows(const void* base, uint64_t stride, const std::vector<T>& row_off) { return by_rows(base, stride, row_off.data(), row_off.size()); }
  RecordSources& at_bytes(const void* base, const std::vector<uint64_t>& byte_off) {
    if (byte_off.size() != n) throw RabeError("RecordSources: an array of byte offsets has n entries");
    dev_src.push_back(base);
    item_off.insert(item_off.end(), byte_off.begin(), byte_off.end());
    return *this;
  }
};

// Sizing of an issuing call (n records out, item i of kind idx[i] < n_kinds).  check_index throws "<what>: <index_name> out of range";
// record_offsets calls it, then fills out_off[0 .. n]: record i takes fixed(i) bytes -- or fixed[idx[i]], for a table by kind -- and, where
// pt_off is given, its sealed plaintext (the payload + 28 bytes of nonce and tag).  Returns whether out_buf is there and holds out_off[n]
// bytes.  Nothing is drawn or written before a caller has seen the answer; what a caller does at n == 0 is its own line.
inline void check_index(const std::string& what, const char* index_name, size_t n, const uint32_t* idx, size_t n_kinds) {
  for (size_t i = 0; i < n; i++) if (idx[i] >= n_kinds) throw RabeError(what + ": " + index_name + " out of range");
}
template <class FIXED>
bool record_offsets(const std::string& what, const char* index_name, size_t n, const uint32_t* idx, size_t n_kinds, FIXED fixed, const uint64_t* pt_off,
                    const uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  check_index(what, index_name, n, idx, n_kinds);
  out_off[0] = 0;
  for (size_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + fixed(i) + (pt_off ? (pt_off[i + 1] - pt_off[i]) + 28 : 0);
  return out_buf && out_cap >= out_off[n];
}
inline bool record_offsets(const std::string& what, const char* index_name, size_t n, const uint32_t* idx, size_t n_kinds, const std::vector<size_t>& fixed,
                           const uint64_t* pt_off, const uint8_t* out_buf, size_t out_cap, uint64_t* out_off) {
  return record_offsets(what, index_name, n, idx, n_kinds, [&](size_t i) { return fixed[idx[i]]; }, pt_off, out_buf, out_cap, out_off);
}

}}  // namespace rabe::schemes
