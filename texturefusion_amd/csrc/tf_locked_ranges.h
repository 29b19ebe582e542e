// tf_locked_ranges.h -- which host ranges a process has page-locked in place, and how many users each has.  Plain
// bookkeeping: the caller does the locking and unlocking and holds whatever mutex guards the registry.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <map>

namespace tf {

class LockedRanges {
 public:
  enum What { kShare, kLockNew, kOverlap };
  struct Answer {
    What what;
    const uint8_t* base;  // of the locked range that covers the request (kOverlap: null)
  };
  // [b, b + bytes) lies inside a locked range (depth / colour views inside one arena): one more user of that range, nothing
  // to lock -- locking pages that are locked already fails.  It touches none: recorded with one user, the caller locks it
  // now (and releases it again if that fails).  Anything else overlaps a range of a different extent: nothing recorded.
  Answer acquire(const uint8_t* b, size_t bytes) {
    auto it = ranges_.upper_bound(b);
    const bool have = it != ranges_.begin() && (--it, b < it->first + it->second.n);  // the range at or below b reaches b
    if (have && b + bytes <= it->first + it->second.n) {
      it->second.refs += 1;
      return {kShare, it->first};
    }
    auto up = ranges_.lower_bound(b);  // the first range that starts at or above b
    if (have || (up != ranges_.end() && up->first < b + bytes)) return {kOverlap, nullptr};
    ranges_[b] = Range{bytes, 1};
    return {kLockNew, b};
  }
  // one user less of the range that starts at base; true: that was the last one, the caller unlocks the pages now
  bool release(const uint8_t* base) {
    auto it = ranges_.find(base);
    if (it == ranges_.end() || --it->second.refs > 0) return false;
    ranges_.erase(it);
    return true;
  }

 private:
  struct Range { size_t n; int refs; };
  std::map<const uint8_t*, Range> ranges_;
};

}  // namespace tf
