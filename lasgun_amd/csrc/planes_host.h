// lasgun_amd/csrc/planes_host.h -- what every query's host code (the *_host.h beside this file, query.cpp) shares and no device is needed
// for: the ray limit, the one overflow-checked size, the one alignment rule, the two rules over a plane table, and HostStaging, the
// host-memory half of a host form's round trip (query.cpp, RoundTrip).  A plane table is any callable that takes a visitor and calls it as
// f(the struct's pointer, the plane's elements, its alignment in bytes, its name) once per plane, in the struct's order.  Kept free of HIP:
// tools/planes_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and so does every tools/*_host_check.cpp
// whose header includes it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

namespace lg {

constexpr unsigned long long QUERY_MAX_RAYS = 0xFFFFFFFFull * 64ull; // 64-ray tiles are counted in 32 bits

// count * bytes_each as a size_t, refused where it does not fit the address space
inline size_t checked_bytes(size_t count, size_t bytes_each, const char *what) {
    if (bytes_each && count > SIZE_MAX / bytes_each) throw std::runtime_error(std::string(what) + " does not fit the address space");
    return count * bytes_each;
}
// The device forms' alignment rule for one pointer; NULL is not misaligned
inline void check_alignment(const void *p, size_t align, const char *what) {
    if (p && (uintptr_t)p % align) throw std::runtime_error(std::string(what) + " is not " + std::to_string(align) + "-byte aligned");
}
// ... for every plane of a table
template <class Table> inline void check_planes_alignment(Table &&table) {
    table([](auto *p, size_t, size_t align, const char *what) { check_alignment(p, align, what); });
}
// The NULL rule of a table: at least one plane is asked for
template <class Table> inline void require_any_plane(Table &&table) {
    bool any = false;
    table([&](auto *p, size_t, size_t, const char *) { any = any || p; });
    if (!any) throw std::runtime_error("every plane of out is NULL: at least one output");
}

// A host form's outputs on their way back: the copy from the device lands in a buffer of this call's and reaches the caller's array in
// place(), which the round trip calls after the synchronise -- so an error on the way (this object destroyed without place()) leaves the
// caller's arrays as they were.
class HostStaging {
    struct Copy { void *to; const void *from; size_t bytes; };
    std::deque<std::vector<unsigned char>> mem; // (a deque: a buffer's address outlives the next one's arrival)
    std::vector<Copy> copies;

  public:
    // n zero-initialised elements of this call's, for the form to place itself
    template <class T> T *hold(size_t n) {
        mem.emplace_back(n * sizeof(T));
        return reinterpret_cast<T *>(mem.back().data());
    }
    // ... that place() copies to `host`; a NULL array is one not asked for: NULL, nothing held
    template <class T> T *stage(T *host, size_t n) {
        if (!host) return nullptr;
        T *s = hold<T>(n);
        copies.push_back({host, s, n * sizeof(T)});
        return s;
    }
    void place() const {
        for (const Copy &c : copies)
            if (c.bytes) std::memcpy(c.to, c.from, c.bytes); // (an empty buffer has no address to copy from)
    }
};

} // namespace lg
