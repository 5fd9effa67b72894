// tests/cpp/ranges_main.cpp -- bls12_381_amd/csrc/ranges.h on its own (tests/test_host_ranges.py builds this with host clang++
// -fsanitize=address,undefined and runs it; it includes nothing of the library but that header).
//
// ranges_overlap is the one overlap test of the Fr argument checks.  Checked here: the named cases (disjoint, touching, nested,
// identical, one byte shared at either end, zero length and NULL on either side), symmetry in the arguments on every call, every
// pair of small ranges against a byte-by-byte count, and the scalar-unit use n * 32 at n = 1 and n = 2^28.  No pointer is read.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "ranges.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (g_fail > 20) exit(1); } } while (0)

// the verdict on (a, b) and on (b, a): they must agree; -1 when they do not
static int both(const void* a, size_t ab, const void* b, size_t bb) {
  const bool f = ranges_overlap(a, ab, b, bb), r = ranges_overlap(b, bb, a, ab);
  CHECK(f == r, "not symmetric: (%p, %zu) against (%p, %zu) gives %d, swapped %d", a, ab, b, bb, (int)f, (int)r);
  return f == r ? (int)f : -1;
}
static const void* at(uintptr_t x) { return (const void*)x; }

static void named() {
  static char buf[256];
  const char* p = buf;
  CHECK(both(p, 32, p + 64, 32) == 0, "disjoint");
  CHECK(both(p, 32, p + 32, 32) == 0, "touching: the end of one is the start of the other");
  CHECK(both(p + 32, 32, p, 32) == 0, "touching, the other way round");
  CHECK(both(p, 128, p + 32, 32) == 1, "nested");
  CHECK(both(p, 128, p, 32) == 1, "nested at the start");
  CHECK(both(p, 128, p + 96, 32) == 1, "nested at the end");
  CHECK(both(p, 64, p, 64) == 1, "identical");
  CHECK(both(p, 33, p + 32, 32) == 1, "one byte shared: the last of the first range");
  CHECK(both(p + 31, 32, p, 32) == 1, "one byte shared: the first of the first range");
  CHECK(both(p, 1, p, 1) == 1, "two one-byte ranges on the same byte");
  CHECK(both(p, 1, p + 1, 1) == 0, "two one-byte ranges side by side");
  // an empty range overlaps nothing, not even a range it lies strictly inside
  CHECK(both(p + 32, 0, p, 128) == 0, "zero length inside a range");
  CHECK(both(p, 0, p, 128) == 0, "zero length at the start of a range");
  CHECK(both(p, 0, p, 0) == 0, "two empty ranges");
  // NULL overlaps nothing, whatever its length says
  CHECK(both(nullptr, 32, p, 32) == 0, "NULL against a range");
  CHECK(both(nullptr, 32, nullptr, 32) == 0, "NULL against NULL");
  CHECK(both(nullptr, ~(size_t)0, p, 32) == 0, "NULL with the largest length");
  CHECK(both(nullptr, 0, p, 0) == 0, "NULL and empty");
}

// every pair of ranges inside a 12-byte window against the count of shared bytes
static void small() {
  const uintptr_t base = 0x10000;
  for (unsigned a = 0; a < 12; a++) for (unsigned al = 0; a + al <= 12; al++)
    for (unsigned b = 0; b < 12; b++) for (unsigned bl = 0; b + bl <= 12; bl++) {
      int shared = 0;
      for (unsigned i = 0; i < 12; i++) if (i >= a && i < a + al && i >= b && i < b + bl) shared++;
      CHECK(both(at(base + a), al, at(base + b), bl) == (shared ? 1 : 0), "[%u, +%u) against [%u, +%u): %d bytes shared", a, al, b, bl, shared);
    }
}

// the callers that think in scalars multiply by 32 at the call
static void scalars() {
  const uintptr_t base = (uintptr_t)1 << 40;
  for (size_t n : {(size_t)1, (size_t)1 << 28}) {
    const size_t bytes = n * 32;
    CHECK(bytes / 32 == n, "n * 32 wraps");
    CHECK(both(at(base), bytes, at(base), bytes) == 1, "n = %zu: identical", n);
    CHECK(both(at(base), bytes, at(base + bytes), bytes) == 0, "n = %zu: back to back", n);
    CHECK(both(at(base), bytes, at(base + bytes - 32), bytes) == 1, "n = %zu: the last scalar shared", n);
    CHECK(both(at(base), bytes, at(base + bytes - 1), bytes) == 1, "n = %zu: the last byte shared", n);
    CHECK(both(at(base + bytes), bytes, at(base), bytes + 1) == 1, "n = %zu: the first byte shared", n);
    CHECK(both(at(base), bytes, at(base + 2 * bytes), 32) == 0, "n = %zu: one scalar a vector further", n);
    CHECK(both(at(base), bytes, at(base + bytes / 2), 32) == 1, "n = %zu: one scalar from the middle on", n);
    CHECK(both(at(base), bytes, at(base + bytes), 0) == 0, "n = %zu: an empty neighbour", n);
  }
}

int main() {
  printf("named\n");
  named();
  printf("small\n");
  small();
  printf("scalars\n");
  scalars();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("all ok\n");
  return 0;
}
