// tf::LockedRanges (the page-lock registry behind tf_host_register) on plain addresses: nothing is locked, nothing is read.
#include <stdio.h>

#include "../../texturefusion_amd/csrc/tf_locked_ranges.h"

static int g_failed = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

int main() {
  using tf::LockedRanges;
  static uint8_t arena[4096];
  const uint8_t* const A = arena + 1024;  // the locked range: [A, A + 1024)
  LockedRanges r;
  LockedRanges::Answer a = r.acquire(A, 1024);
  CHECK(a.what == LockedRanges::kLockNew && a.base == A);

  // the same range acquired twice is shared, and the second release is the last
  a = r.acquire(A, 1024);
  CHECK(a.what == LockedRanges::kShare && a.base == A);
  CHECK(!r.release(A));
  // a view strictly inside a locked range shares it
  a = r.acquire(A + 100, 200);
  CHECK(a.what == LockedRanges::kShare && a.base == A);
  CHECK(!r.release(A));  // (the view's user; the first one still holds the range)
  // a range that starts inside a locked one and runs past its end overlaps
  a = r.acquire(A + 512, 1024);
  CHECK(a.what == LockedRanges::kOverlap && a.base == nullptr);
  // a range that starts below a locked one and reaches into it overlaps
  a = r.acquire(A - 512, 513);
  CHECK(a.what == LockedRanges::kOverlap && a.base == nullptr);
  // ... and neither was recorded: the range below is still free up to where the locked one starts
  // a range that ends exactly where a locked one starts is new
  a = r.acquire(A - 512, 512);
  CHECK(a.what == LockedRanges::kLockNew && a.base == A - 512);
  // ... as is one that starts exactly where it ends
  a = r.acquire(A + 1024, 16);
  CHECK(a.what == LockedRanges::kLockNew && a.base == A + 1024);
  CHECK(r.release(A - 512));
  CHECK(r.release(A + 1024));
  // a release of an unknown base is a no-op (a base inside a locked range is unknown too)
  CHECK(!r.release(arena));
  CHECK(!r.release(A + 100));
  a = r.acquire(A, 1024);
  CHECK(a.what == LockedRanges::kShare);  // (the no-ops above took nothing away)
  CHECK(!r.release(A));
  // after the last release, the same range is new again
  CHECK(r.release(A));
  CHECK(!r.release(A));
  a = r.acquire(A, 1024);
  CHECK(a.what == LockedRanges::kLockNew && a.base == A);
  CHECK(r.release(A));

  if (g_failed) return 1;
  printf("LOCKED RANGES OK\n");
  return 0;
}
