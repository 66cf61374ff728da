// The readers of untrusted record blobs that packed.cpp's decrypts share -- check_offsets, Cursor, same -- and the reader of ONE AC17
// ciphertext record (Ac17CpCiphertext / Ac17KpCiphertext as rabe_obj_serialize writes them):
//   CP head   u32 length, policy text, one language byte               KP head   u32 count, then (u32 length, bytes) per attribute
//   body      u32 3, c_0 (3 x 128), u32 rows, per row (u32 length, name, u32 3, 3 x 64), c_p (384), u32 length, sealed plaintext
// Nothing here knows the engine: tests/hostsim/ac17_record_check.cpp runs the reader alone on a CPU, plain and under the sanitizers, over every
// prefix of a record and every overwritten count.  What it promises: it throws RabeError, or every pointer of the View lies inside
// [begin, end) with its full extent.
#pragma once
#include <string.h>

#include <utility>
#include <vector>

#include "bytes.h"

namespace rabe { namespace schemes {

// bounds of the records of an untrusted blob: monotone, inside [0, len); span = total size of the well-formed ones
inline uint64_t check_offsets(size_t n, const uint64_t* off, size_t len, std::vector<std::string>* errors) {
  uint64_t span = 0;
  for (size_t i = 0; i < n; i++) {
    if (off[i] > off[i + 1] || off[i + 1] > len) (*errors)[i] = "deserialize: record offsets are not monotone inside the blob";
    else span += off[i + 1] - off[i];
  }
  return span;
}
[[noreturn]] inline void throw_truncated() { throw RabeError("deserialize: truncated input"); }          // out of the readers' loops
struct Cursor {
  const uint8_t* p;
  const uint8_t* end;
  void need(size_t k) const { if ((size_t)(end - p) < k) throw_truncated(); }
  uint32_t u32() { need(4); uint32_t v = get_u32(p); p += 4; return v; }
  const uint8_t* raw(size_t k) { need(k); const uint8_t* q = p; p += k; return q; }
  std::pair<const char*, uint32_t> str() { uint32_t l = u32(); return {(const char*)raw(l), l}; }
};
inline bool same(const std::pair<const char*, uint32_t>& a, const std::string& b) { return a.second == b.size() && memcmp(a.first, b.data(), b.size()) == 0; }

namespace ac17 {
typedef std::pair<const char*, uint32_t> Name;
struct View {
  const uint8_t* key = nullptr;          // what a decrypt's plan is keyed by: CP the policy text, KP the whole attribute head
  uint32_t key_len = 0;
  bool human = false;                    // CP: the language byte
  const uint8_t* c0 = nullptr;           // 384
  const uint8_t* cp = nullptr;           // 384
  const uint8_t* sealed = nullptr;       // sealed_len
  uint32_t sealed_len = 0, rows = 0;
  std::vector<const uint8_t*> row_ptr;   // 192 each
};
inline void cp_head(Cursor& c, View* v) {
  v->key_len = c.u32();
  c.need((size_t)v->key_len + 1);
  v->key = c.raw(v->key_len);
  v->human = *c.raw(1) != 0;
}
inline void kp_head(Cursor& c, View* v) {
  v->key = c.p;
  const uint32_t cnt = c.u32();
  if ((size_t)cnt * 4 > (size_t)(c.end - c.p)) throw_truncated();          // before the loop: a hostile count costs nothing
  for (uint32_t k = 0; k < cnt; k++) c.str();
  v->key_len = (uint32_t)(c.p - v->key);
}
// names: the caller's scratch (one per thread: no allocation per record once it has grown); names[r] is row r's name on return
inline void read_record(const uint8_t* begin, const uint8_t* end, bool kp, std::vector<Name>& names, View* v) {
  Cursor c{begin, end};
  if (kp) kp_head(c, v); else cp_head(c, v);
  c.need(4 + 384);
  if (c.u32() != 3) throw RabeError("deserialize: c_0 does not have 3 elements");
  v->c0 = c.raw(384);
  const uint32_t rows = c.u32();
  if ((size_t)rows * 200 > (size_t)(c.end - c.p)) throw_truncated();          // before anything is sized by it
  v->rows = rows;
  v->row_ptr.resize(rows);
  names.resize(rows);
  for (uint32_t r = 0; r < rows; r++) {
    const uint32_t nl = c.u32();
    c.need((size_t)nl + 4 + 192);          // the whole row at once: a million rows per call go through here
    names[r] = {(const char*)c.p, nl};
    if (get_u32(c.p + nl) != 3) throw RabeError("deserialize: an AC17 row does not have 3 elements");
    v->row_ptr[r] = c.p + nl + 4;
    c.p += (size_t)nl + 4 + 192;
  }
  c.need(384 + 4);
  v->cp = c.raw(384);
  v->sealed_len = c.u32();
  v->sealed = c.raw(v->sealed_len);
}
}  // namespace ac17

}}  // namespace rabe::schemes
