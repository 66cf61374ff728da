// The pure helpers of the C interface (rabe_amd/csrc/host/abi_helpers.h) on a CPU: tests/test_abi_helpers_host.py builds this program plain
// and with -fsanitize=address,undefined and runs it.  Every input array lives on the heap at exactly the size the helper may read, so that
// a read past it is the sanitizer's to report.  Prints the number of checks; exit 1 with the failed line otherwise.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "../../rabe_amd/csrc/host/abi_helpers.h"

using namespace rabe::abi;

static int checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { fprintf(stderr, "abi_helpers_check.cpp:%d: %s\n", __LINE__, #c); exit(1); } } while (0)

typedef std::vector<std::vector<std::string>> Sets;

// the flat names / counts arrays of a call, each allocated at its exact length
static Sets sets_of(const std::vector<const char*>& names, const std::vector<size_t>& counts) {
  std::unique_ptr<const char*[]> a(new const char*[names.size()]);
  std::unique_ptr<size_t[]> c(new size_t[counts.size()]);
  for (size_t i = 0; i < names.size(); i++) a[i] = names[i];
  for (size_t i = 0; i < counts.size(); i++) c[i] = counts[i];
  return attr_sets(a.get(), c.get(), counts.size());
}
static uint64_t span_of(const std::vector<uint64_t>& off, size_t len) {
  std::unique_ptr<uint64_t[]> o(new uint64_t[off.size()]);
  for (size_t i = 0; i < off.size(); i++) o[i] = off[i];
  return record_span(off.size() - 1, o.get(), len);
}

int main() {
  // attr_sets: no list at all touches neither array
  CHECK(attr_sets(nullptr, nullptr, 0).empty());
  CHECK(sets_of({}, {}).empty());
  // a list of zero names between two non-empty ones takes no name and shifts none
  CHECK((sets_of({"A", "B", "C"}, {2, 0, 1}) == Sets{{"A", "B"}, {}, {"C"}}));
  // the counts sum to the length of the flat array exactly: the last name is read, nothing behind it
  CHECK((sets_of({"A", "B", "C", "D"}, {1, 3}) == Sets{{"A"}, {"B", "C", "D"}}));
  CHECK((sets_of({"A"}, {0, 0, 1}) == Sets{{}, {}, {"A"}}));
  CHECK((sets_of({}, {0, 0}) == Sets{{}, {}}));
  // names are copied, a repeated name stays repeated
  CHECK((sets_of({"A", "A"}, {2}) == Sets{{"A", "A"}}));

  // record_span: n = 0 reads no offset
  CHECK(record_span(0, nullptr, 0) == 0);
  CHECK(span_of({5}, 100) == 0);
  CHECK(span_of({0, 10, 30}, 30) == 30);
  CHECK(span_of({4, 10}, 10) == 6);                                // the first record need not start at 0
  CHECK(span_of({0, 0, 0}, 0) == 0);                               // empty records are well-formed
  // decreasing offsets: the record that runs backwards counts nothing, its neighbours count on their own bounds
  CHECK(span_of({0, 10, 5, 20}, 20) == 10 + 15);
  CHECK(span_of({10, 0}, 20) == 0);
  // an offset past len: every record that ends there is left out, the ones inside stay
  CHECK(span_of({0, 10, 31}, 30) == 10);
  CHECK(span_of({0, 31, 40}, 30) == 0);
  CHECK(span_of({0, 10, 31, 20}, 30) == 10);                       // 31 -> 20 runs backwards as well
  CHECK(span_of({0, UINT64_MAX}, 30) == 0);
  CHECK(span_of({0, 30}, 30) == 30);                               // ending AT len is inside

  // key_ptrs: the handles in order, typed; none for n = 0
  struct Key { int v; };
  Key k0{7}, k1{9};
  CHECK(key_ptrs<Key>(nullptr, 0).empty());
  std::unique_ptr<const void*[]> handles(new const void*[2]);
  handles[0] = &k1;
  handles[1] = &k0;
  const std::vector<const Key*> p = key_ptrs<Key>(handles.get(), 2);
  CHECK(p.size() == 2 && p[0] == &k1 && p[1] == &k0 && p[0]->v == 9 && p[1]->v == 7);
  printf("%d\n", checks);
  return 0;
}
