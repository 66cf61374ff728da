// What a reader of canonical records needs and nothing else: the error type and the little-endian u32 fields.  Free of the engine's headers, so
// that a record reader (ac17_record.h) can be compiled and run alone on a CPU (tests/hostsim/ac17_record_check.cpp).
#pragma once
#include <stdint.h>

#include <stdexcept>
#include <string>

namespace rabe {

// src/error.rs:19-28
struct RabeError : std::runtime_error {
  explicit RabeError(const std::string& details) : std::runtime_error(details) {}
};

inline void put_u32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
inline uint32_t get_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

}  // namespace rabe
