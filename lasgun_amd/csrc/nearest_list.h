// lasgun_amd/csrc/nearest_list.h -- the per-point list of lg_nearest* (include/lasgun_hip.h has the contract): which candidates are admissible,
// the order between two of them, the rule between a candidate and a full list, and the insertion that keeps the list sorted.  A list is the
// first m <= k admissible candidates seen so far in ascending (d2, key) order; what falls off its end is gone, so after any stream of
// candidates it holds the first k of that stream's admissible ones in that order -- whatever order they arrived in.  Host and device: ONE
// text for k_nearest.hip (the list in dynamic LDS behind the walk's stack) and for tools/nearest_list_check.cpp, which runs it under
// AddressSanitizer / UBSan on the CPU against numpy's lexsort of (d2, key), word for word.  Storage is the caller's: `List` is anything with
// get(e) and set(e, entry) over entries 0 .. k-1.
#pragma once
#include "vecmath.h"

// tools/nearest_list_check.cpp alone is also built with 1, 2 and 3: one seeded fault each (a swapped tie, a full list that refuses a
// candidate tying its last entry whatever the key, an admissibility test that lets +INF through), which tests/test_nearest_list_host.py must
// see caught.  The product is built with 0.
#ifndef LG_NEAREST_FAULT
#define LG_NEAREST_FAULT 0
#endif

namespace lg {

struct NearestEntry {
    double d2;              // the candidate's squared distance
    unsigned long long key; // instance << 34 | kind << 32 | prim (closest_prim.h, closest_key)
    uint32_t slot;          // its leaf slot (index into the primitive table): the winner's x is evaluated again from it at the end
};

// admissible iff d2 <= r2 and d2 < +INF (a NaN fails both): lg_closest_points' rule, r2 the point's own radius squared
LG_HD bool nearest_admissible(double d2, double r2) {
#if LG_NEAREST_FAULT == 3
    return d2 <= r2;
#else
    return d2 <= r2 && d2 < INFINITY;
#endif
}
// does a come before b?  Ascending d2, an exact tie by ascending key.  (No admissible d2 is a NaN: the order is total.)
LG_HD bool nearest_before(const NearestEntry &a, const NearestEntry &b) {
#if LG_NEAREST_FAULT == 1
    return a.d2 < b.d2 || (a.d2 == b.d2 && a.key > b.key);
#else
    return a.d2 < b.d2 || (a.d2 == b.d2 && a.key < b.key);
#endif
}
// An ADMISSIBLE candidate c offered to a list of m entries with room for k.  A full list takes it iff it comes before the last entry --
// which then falls off --; it is placed behind every entry it does not come before, those after it moved up by one.
template <class List> LG_HD void nearest_insert(List &list, uint32_t &m, uint32_t k, const NearestEntry &c) {
    if (k == 0u) return;
    if (m == k) {
        const NearestEntry last = list.get(k - 1u);
#if LG_NEAREST_FAULT == 2
        if (!(c.d2 < last.d2)) return;
#else
        if (!nearest_before(c, last)) return;
#endif
    }
    uint32_t j = m < k ? m : k - 1u; // the entry that opens: behind the last, or the last itself
    while (j > 0u) {
        const NearestEntry p = list.get(j - 1u);
        if (!nearest_before(c, p)) break;
        list.set(j, p);
        --j;
    }
    list.set(j, c);
    if (m < k) ++m;
}
// The d2 above which nothing can enter the list any more: the last entry's once it is full (a candidate that ties it may still enter, by
// its key: the walk's skip test is strict), +INF before
template <class List> LG_HD double nearest_worst(const List &list, uint32_t m, uint32_t k) { return (k != 0u && m == k) ? list.get(k - 1u).d2 : INFINITY; }

} // namespace lg
