// The reader of one AC17 ciphertext record (rabe_amd/csrc/host/ac17_record.h) on a CPU: tests/test_ac17_record_host.py builds this program
// plain and with -fsanitize=address,undefined and runs it.  One CP and one KP record of 3 rows are synthesised from arbitrary element bytes;
// the reader runs on every prefix of each, and on each record with every u32 field overwritten by 0, 3, 0xffffffff and 2 * len.  Every input
// lives on the heap at exactly its length, so a read past it is the sanitizer's to report.  For every result: the reader threw RabeError, or
// every pointer of the View lies inside [begin, end) with its full extent.  Prints the number of checks; exit 1 with the failed line otherwise.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "../../rabe_amd/csrc/host/ac17_record.h"

using namespace rabe;
using namespace rabe::schemes;

static int checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "ac17_record_check.cpp:%d: %s\n", __LINE__, #c); exit(1); } } while (0)

typedef std::vector<uint8_t> Bytes;
static void u32(Bytes& b, std::vector<size_t>* fields, uint32_t v) {
  if (fields) fields->push_back(b.size());
  for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i)));
}
static void fill(Bytes& b, size_t n, uint8_t seed) { for (size_t i = 0; i < n; i++) b.push_back((uint8_t)(seed + 7 * i)); }
static void str(Bytes& b, std::vector<size_t>* fields, const char* s) { u32(b, fields, (uint32_t)strlen(s)); b.insert(b.end(), s, s + strlen(s)); }
// fields: the offset of every u32 of the record
static Bytes record(bool kp, std::vector<size_t>* fields) {
  const char* names[3] = {"A", "department", "C"};
  Bytes b;
  if (kp) { u32(b, fields, 3); for (const char* nm : names) str(b, fields, nm); }
  else { str(b, fields, "\"A\" and (\"department\" or \"C\")"); b.push_back(1); }
  u32(b, fields, 3); fill(b, 384, 1);
  u32(b, fields, 3);
  for (int r = 0; r < 3; r++) { str(b, fields, names[r]); u32(b, fields, 3); fill(b, 192, (uint8_t)(10 + r)); }
  fill(b, 384, 99);
  u32(b, fields, 45); fill(b, 45, 5);
  return b;
}
static bool inside(const uint8_t* p, size_t n, const uint8_t* begin, const uint8_t* end) { return p >= begin && p <= end && (size_t)(end - p) >= n; }
// 1: the reader accepted the bytes and the View is inside them; 0: it threw RabeError.  Anything else ends the program.
static int run(const Bytes& bytes, bool kp) {
  std::unique_ptr<uint8_t[]> heap(new uint8_t[bytes.size()]);          // exactly as long as the record
  if (!bytes.empty()) memcpy(heap.get(), bytes.data(), bytes.size());
  const uint8_t* begin = heap.get();
  const uint8_t* end = begin + bytes.size();
  static std::vector<ac17::Name> names;
  ac17::View v;
  try {
    ac17::read_record(begin, end, kp, names, &v);
  } catch (const RabeError&) {
    return 0;
  }
  CHECK(inside(v.key, v.key_len, begin, end));
  CHECK(inside(v.c0, 384, begin, end));
  CHECK(inside(v.cp, 384, begin, end));
  CHECK(inside(v.sealed, v.sealed_len, begin, end));
  CHECK(v.row_ptr.size() == v.rows && names.size() == v.rows);
  for (uint32_t r = 0; r < v.rows; r++) {
    CHECK(inside(v.row_ptr[r], 192, begin, end));
    CHECK(inside((const uint8_t*)names[r].first, names[r].second, begin, end));
  }
  return 1;
}

int main() {
  for (int kp = 0; kp < 2; kp++) {
    std::vector<size_t> fields;
    const Bytes rec = record(kp != 0, &fields);
    CHECK(fields.size() == (kp ? 13u : 10u));
    CHECK(run(rec, kp != 0) == 1);
    // what the whole record reads as
    {
      std::vector<ac17::Name> names;
      ac17::View v;
      ac17::read_record(rec.data(), rec.data() + rec.size(), kp != 0, names, &v);
      CHECK(v.rows == 3 && v.sealed_len == 45 && v.sealed + 45 == rec.data() + rec.size() && v.human == (kp == 0));
      CHECK(same(names[1], "department") && !same(names[1], "departmen") && !same(names[0], "B"));
      CHECK(v.key == rec.data() + (kp ? 0 : 4) && v.c0 == v.key + v.key_len + (kp ? 0 : 1) + 4);
    }
    // every proper prefix is refused: each byte of the record is some field's
    for (size_t len = 0; len < rec.size(); len++) CHECK(run(Bytes(rec.begin(), rec.begin() + len), kp != 0) == 0);
    // bytes behind the sealed part are nobody's
    { Bytes longer = rec; longer.push_back(0); CHECK(run(longer, kp != 0) == 1); }
    // every u32 field overwritten
    const uint32_t values[4] = {0, 3, 0xffffffffu, (uint32_t)(2 * rec.size())};
    int accepted = 0;
    for (size_t at : fields)
      for (uint32_t val : values) {
        Bytes b = rec;
        put_u32(b.data() + at, val);
        accepted += run(b, kp != 0);
      }
    // 3 is what the five count fields hold (six with the KP attribute count), and 0 or 3 in the sealed length leave a shorter sealed part
    CHECK(accepted == (kp ? 8 : 7));
  }
  // check_offsets: decreasing, beyond the blob, n = 0, and what the span counts
  {
    std::vector<std::string> errors(3);
    const uint64_t off[4] = {0, 10, 5, 20};
    CHECK(check_offsets(3, off, 20, &errors) == 10 + 15);
    CHECK(errors[0].empty() && errors[1] == "deserialize: record offsets are not monotone inside the blob" && errors[2].empty());
    errors.assign(3, "");
    CHECK(check_offsets(3, off, 19, &errors) == 10);
    CHECK(errors[0].empty() && !errors[1].empty() && errors[2] == errors[1]);
    errors.clear();
    CHECK(check_offsets(0, off, 0, &errors) == 0);
    const uint64_t big[2] = {~(uint64_t)0, ~(uint64_t)0};
    errors.assign(1, "");
    CHECK(check_offsets(1, big, 100, &errors) == 0 && !errors[0].empty());
  }
  printf("%d checks\n", checks);
  return 0;
}
