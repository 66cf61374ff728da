// Pure helpers of the C interface (host_abi.cpp): argument conversions that touch neither an engine nor a host.  Header-only and free of the
// engine's headers, so that tests/hostsim/abi_helpers_check.cpp can run them on a CPU, plain and under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace rabe { namespace abi {

// attribute lists of a bulk call: flat names + per-list counts; list s takes the next counts[s] names
inline std::vector<std::vector<std::string>> attr_sets(const char* const* attributes, const size_t* counts, size_t n_sets) {
  std::vector<std::vector<std::string>> sets(n_sets);
  size_t at = 0;
  for (size_t s = 0; s < n_sets; s++)
    for (size_t k = 0; k < counts[s]; k++) sets[s].push_back(attributes[at++]);
  return sets;
}

// What a batch cut over a device group asks of the plaintext buffer (pipeline.cpp: consume): the total size of the well-formed records, those
// whose offsets are monotone and end inside the blob.  Reads off[0 .. n].
inline uint64_t record_span(size_t n, const uint64_t* off, size_t len) {
  uint64_t span = 0;
  for (size_t i = 0; i < n; i++) if (off[i] <= off[i + 1] && off[i + 1] <= len) span += off[i + 1] - off[i];
  return span;
}

// the opaque key handles of a call as pointers to their type
template <class T>
inline std::vector<const T*> key_ptrs(const void* const* keys, size_t n) {
  std::vector<const T*> v;
  for (size_t i = 0; i < n; i++) v.push_back((const T*)keys[i]);
  return v;
}

}}  // namespace rabe::abi
