// tools/host_check.h -- what the stand-alone sanitized programs (tools/*_host_check.cpp) share, test support only: the EXPECT macro with its
// failure counter, thrown() and throws(), and staged_round(), a host form's staged round trip over a plane table (lasgun_amd/csrc/planes_host.h) with the
// launch stubbed out.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>

#include "../lasgun_amd/csrc/planes_host.h"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// A non-NULL, 16-byte aligned address for a tool's struct to say "this plane is asked for" with (staged_round puts the caller's block there)
alignas(16) inline unsigned char ASKED[16];

// what f() throws says; "" where it throws nothing
template <class F> static std::string thrown(F &&f) {
    try {
        f();
    } catch (const std::exception &e) {
        return e.what();
    }
    return "";
}
// does f() throw an error that says something?
template <class F> static bool throws(F &&f) { return !thrown(f).empty(); }

// What staged_round saw: the bytes staged for each plane of the table, in its order (0 for one not asked for), and their sum
struct StagedRound {
    std::vector<size_t> plane_bytes;
    size_t bytes = 0;
};
// One host form without a device, over `table` (a callable that takes a visitor f(pointer, count, align, name); it runs over a struct of the
// tool's whose non-NULL pointers say which planes are asked for, and may be called more than once).  Every plane asked for gets a "caller's"
// heap block of EXACTLY count * sizeof(element) bytes -- a copy past its end is an ASan report -- which replaces the struct's pointer; the
// planes are staged through lg::HostStaging; the stubbed launch fills every staged byte with a value of its plane and offset; the caller's
// blocks are still as they were before place() and hold every one of those bytes after it.
template <class Table> static StagedRound staged_round(Table &&table) {
    struct Plane { std::unique_ptr<unsigned char[]> caller; unsigned char *staged; size_t bytes; };
    const auto prefill = [](size_t k, size_t i) { return (unsigned char)(0xC5u ^ (k * 29u) ^ (i * 3u)); };
    const auto written = [](size_t k, size_t i) { return (unsigned char)(1u + k * 37u + i * 7u + (i >> 8)); };
    std::vector<Plane> planes;
    StagedRound round;
    lg::HostStaging staging;
    table([&](auto *&p, size_t count, size_t, const char *) {
        const size_t k = planes.size(), bytes = p ? count * sizeof *p : 0;
        planes.push_back({nullptr, nullptr, bytes});
        round.plane_bytes.push_back(bytes);
        round.bytes += bytes;
        if (!p) { EXPECT(staging.stage(p, count) == nullptr); return; }
        planes[k].caller.reset(new unsigned char[bytes]);
        for (size_t i = 0; i < bytes; ++i) planes[k].caller[i] = prefill(k, i);
        p = reinterpret_cast<decltype(+p)>(planes[k].caller.get());
        planes[k].staged = reinterpret_cast<unsigned char *>(staging.stage(p, count));
        EXPECT(planes[k].staged != nullptr || bytes == 0);
    });
    bool zeroed = true, untouched = true, placed = true;
    for (size_t k = 0; k < planes.size(); ++k) // the stubbed launch (a staged buffer starts zeroed)
        for (size_t i = 0; i < planes[k].bytes; ++i) { zeroed = zeroed && planes[k].staged[i] == 0; planes[k].staged[i] = written(k, i); }
    for (size_t k = 0; k < planes.size(); ++k)
        for (size_t i = 0; i < planes[k].bytes; ++i) untouched = untouched && planes[k].caller[i] == prefill(k, i);
    staging.place();
    for (size_t k = 0; k < planes.size(); ++k)
        for (size_t i = 0; i < planes[k].bytes; ++i) placed = placed && planes[k].caller[i] == written(k, i);
    EXPECT(zeroed);
    EXPECT(untouched);
    EXPECT(placed);
    return round;
}
