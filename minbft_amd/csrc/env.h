// Readers of the MBFT_* environment variables (INTEGRATION.md's table lists
// every one; tests/test_env_knobs.py keeps the two in step).  An unset
// variable gives `dflt`.  Each call reads the environment: a knob read once
// per process keeps the result in a `static const` at its use, one read per
// call is a plain call.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace mbft {

inline long env_long(const char* name, long dflt) {
  const char* v = getenv(name);
  return v ? atol(v) : dflt;
}
inline size_t env_size(const char* name, size_t dflt) {
  const char* v = getenv(name);
  return v ? (size_t)strtoull(v, nullptr, 10) : dflt;
}
inline uint32_t env_u32(const char* name, uint32_t dflt) {
  const char* v = getenv(name);
  return v ? (uint32_t)strtoul(v, nullptr, 10) : dflt;
}
inline double env_double(const char* name, double dflt) {
  const char* v = getenv(name);
  return v ? atof(v) : dflt;
}
// a switch: any number but 0 is on
inline bool env_on(const char* name, bool dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) != 0 : dflt;
}
// the variable is set to exactly `value`
inline bool env_is(const char* name, const char* value) {
  const char* v = getenv(name);
  return v && strcmp(v, value) == 0;
}
inline bool env_set(const char* name) { return getenv(name) != nullptr; }

}  // namespace mbft
