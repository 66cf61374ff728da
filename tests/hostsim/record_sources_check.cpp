// The source table of the record writers (rabe_amd/csrc/host/record_layout.h: RecordSources, RecordLayout) on a CPU:
// tests/test_record_sources_host.py builds this program plain and with -fsanitize=address,undefined and runs it.  It includes that header
// alone.  The offset table is compared with the naive formula item_off[k * n + i]; a layout's map is then applied to small host buffers
// through those offsets, the way rhip_assemble_records reads them.  Every array is allocated at exactly the size the code may read, so
// that a read past it is the sanitizer's to report.  Prints the number of checks; exit 1 with the failed line otherwise.
#include <stdio.h>
#include <stdlib.h>

#include "../../rabe_amd/csrc/host/record_layout.h"

using namespace rabe::schemes;

static int checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "record_sources_check.cpp:%d: %s\n", __LINE__, #c); exit(1); } } while (0)

template <class FN>
static bool refused(FN fn) {
  try { fn(); } catch (const rabe::RabeError&) { return true; }
  return false;
}

// what rhip_assemble_records does for item i of a layout: literals from the map, the others from source k at the item's offset
static std::vector<uint8_t> assemble(const RecordLayout& L, const RecordSources& s, size_t i) {
  std::vector<uint8_t> out;
  for (uint32_t m : L.map) {
    const uint32_t k = m >> 24, o = m & 0xFFFFFFu;
    out.push_back(k == 0xFF ? (uint8_t)o : ((const uint8_t*)s.dev_src[k])[s.item_off[k * s.n + i] + o]);
  }
  return out;
}

int main() {
  const uint8_t* const A = (const uint8_t*)0x1000;          // bases are never read where only offsets are computed
  const uint8_t* const B = (const uint8_t*)0x2000;
  // n = 0: sources without offsets; the prefix array still has its one entry
  {
    RecordSources s(0);
    s.by_item(A, 384).by_rows(B, 64, std::vector<uint32_t>{0}).at_bytes(A, std::vector<uint64_t>{});
    CHECK(s.dev_src.size() == 3 && s.item_off.empty());
    CHECK(refused([&] { RecordSources(0).by_rows(A, 64, std::vector<uint32_t>{}); }));
  }
  // one item
  {
    RecordSources s(1);
    s.by_item(A, 384).by_rows(B, 192, std::vector<uint32_t>{0, 5});
    CHECK((s.item_off == std::vector<uint64_t>{0, 0}));
    CHECK(s.dev_src[0] == A && s.dev_src[1] == B);
  }
  // three items over rows [1, 2, 1]: row offsets 0, 1, 3; all three kinds in one list, both prefix-array types
  {
    const std::vector<uint32_t> rows32{0, 1, 3, 4};
    const std::vector<size_t> rows64{0, 1, 3, 4};
    const std::vector<uint64_t> bytes{7, 0, 1000};
    RecordSources s(3);
    s.by_item(A, 384).by_rows(B, 64, rows32).by_rows(B, 128, rows64).at_bytes(A, bytes).by_item(B, 64);
    CHECK(s.dev_src.size() == 5 && s.item_off.size() == 5 * 3);
    for (size_t i = 0; i < 3; i++) {
      CHECK(s.item_off[0 * 3 + i] == 384 * i);
      CHECK(s.item_off[1 * 3 + i] == 64 * (uint64_t)rows32[i]);
      CHECK(s.item_off[2 * 3 + i] == 128 * (uint64_t)rows64[i]);
      CHECK(s.item_off[3 * 3 + i] == bytes[i]);
      CHECK(s.item_off[4 * 3 + i] == 64 * i);
    }
    // the pointer form a part of a batch uses: a prefix array relative to the part's first row, heap-allocated at n + 1 entries
    uint32_t* rel = new uint32_t[4]{0, 2, 3, 6};
    RecordSources p(3);
    p.by_rows(B, 192, rel, 4);
    CHECK((p.item_off == std::vector<uint64_t>{0, 384, 576}));
    delete[] rel;
  }
  // a row offset of 3e9 with stride 384: the product does not wrap at 32 bits (offsets only, nothing is allocated)
  {
    RecordSources s(2);
    s.by_rows(A, 384, std::vector<uint32_t>{3000000000u, 3000000001u, 3000000002u}).by_rows(A, 384, std::vector<size_t>{3000000000u, 3000000001u, 3000000002u});
    CHECK(s.item_off[0] == 1152000000000ull && s.item_off[1] == 1152000000384ull);
    CHECK(s.item_off[2] == 1152000000000ull && s.item_off[3] == 1152000000384ull);
    RecordSources t(70000);          // and the by-item product: item 69 999 at stride 65 536 lies past 2^32
    t.by_item(A, 65536);
    CHECK(t.item_off[69999] == 65536ull * 69999);
  }
  // a prefix or offset array of the wrong length is refused, and leaves nothing behind
  {
    RecordSources s(3);
    CHECK(refused([&] { s.by_rows(A, 64, std::vector<uint32_t>{0, 1, 3}); }));          // n entries: the prefix array of a shorter call
    CHECK(refused([&] { s.by_rows(A, 64, std::vector<size_t>{0, 1, 3, 4, 5}); }));
    CHECK(refused([&] { s.at_bytes(A, std::vector<uint64_t>{0, 1, 3, 4}); }));          // n + 1 entries: a prefix array taken for offsets
    CHECK(refused([&] { s.at_bytes(A, std::vector<uint64_t>{0, 1}); }));
    CHECK(s.dev_src.empty() && s.item_off.empty());
  }
  // a layout applied through the table: two items, the second with a two-row record, against records laid out by hand
  {
    std::vector<uint8_t> head{0xA0, 0xA1, 0xA2, 0xB0, 0xB1, 0xB2};                      // 3 bytes per item
    std::vector<uint8_t> rows{0x10, 0x11, 0x20, 0x21, 0x30, 0x31};                      // 2 bytes per row: item 0 has row 0, item 1 rows 1 and 2
    std::vector<uint8_t> names{'x', 'y', 'z'};                                          // item 0: "x" at 0, item 1: "yz" at 1
    const std::vector<uint32_t> row_off{0, 1, 3};
    RecordSources s(2);
    s.by_item(head.data(), 3).by_rows(rows.data(), 2, row_off).at_bytes(names.data(), std::vector<uint64_t>{0, 1});
    RecordLayout one, two;
    one.src(0, 0, 3); one.u32(1); one.src(1, 0, 2); one.u8(1); one.src(2, 0, 1);
    two.src(0, 0, 3); two.u32(2); two.src(1, 0, 2); two.src(1, 2, 2); two.str("ab"); two.src(2, 0, 2);
    CHECK((assemble(one, s, 0) == std::vector<uint8_t>{0xA0, 0xA1, 0xA2, 1, 0, 0, 0, 0x10, 0x11, 1, 'x'}));
    CHECK((assemble(two, s, 1) == std::vector<uint8_t>{0xB0, 0xB1, 0xB2, 2, 0, 0, 0, 0x20, 0x21, 0x30, 0x31, 2, 0, 0, 0, 'a', 'b', 'y', 'z'}));
    CHECK(two.parts.size() == 4 && two.parts[2].rec_off == 9 && two.parts[2].part_off == 2 && two.parts[2].k == 1 && two.parts[2].len == 2);
    // the end of a ciphertext layout: the size counts the length field either way; only a KEM layout carries it, as zero
    const size_t before = two.bytes();
    CHECK(close_ciphertext(one, false) == 11 + 4 && one.bytes() == 11);
    CHECK(close_ciphertext(two, true) == before + 4 && two.bytes() == before + 4);
    CHECK((std::vector<uint32_t>(two.map.end() - 4, two.map.end()) == std::vector<uint32_t>(4, 0xFF000000u)));
  }
  // record_offsets: sizes by kind plus the sealed payloads, the capacity verdict, the index check
  {
    const std::vector<size_t> fixed{10, 20};
    const uint32_t idx[3] = {1, 0, 1};
    const uint64_t pt_off[4] = {0, 1, 1, 18};
    uint64_t out_off[4];
    uint8_t room[1];
    CHECK(record_offsets("t", "item", 3, idx, 2, fixed, pt_off, room, 152, out_off) && out_off[1] == 49 && out_off[2] == 87 && out_off[3] == 152);
    CHECK(!record_offsets("t", "item", 3, idx, 2, fixed, pt_off, room, 151, out_off));
    CHECK(!record_offsets("t", "item", 3, idx, 2, fixed, nullptr, nullptr, 1000, out_off) && out_off[3] == 50);
    CHECK(refused([&] { record_offsets("t", "item", 3, idx, 1, fixed, nullptr, room, 1000, out_off); }));
  }
  printf("%d checks\n", checks);
  return 0;
}
