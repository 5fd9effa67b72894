// ranges.h -- the one overlap test of the argument checks.  Plain C++ with no HIP in it: tests/cpp/ranges_main.cpp compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

// the half-open byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte; a NULL pointer or an empty range overlaps nothing.
// Callers that think in scalars multiply by 32 at the call, and an in-place form (same pointer) is the caller's exception.
static inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}
