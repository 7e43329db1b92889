// tools/segments_host_check.cpp -- the device-free host code of lg_closest_segments* (lasgun_amd/csrc/segments_host.h: the five-plane table,
// every check and every refusal in its order, the sizes at their limits, the alignment rule, which plane set is the touch-only form, the host
// form's staging for every subset of the planes) compiled alone for the CPU, with its own main: nothing of HIP, nothing loaded into python.
// tests/test_segments_host_sanitized.py builds it under AddressSanitizer and UBSan.
//
// usage: segments_host_check               the self-checks; prints "segments_host_check: ok"
#include <cmath>
#include <cstdio>
#include <limits>

#include "../lasgun_amd/csrc/segments_host.h"
#include "host_check.h"

using namespace lg;

static const double INF = std::numeric_limits<double>::infinity(), QNAN = std::numeric_limits<double>::quiet_NaN();

static lg_segments_out subset(int planes, void *p) {
    return lg_segments_out{(planes & 1) ? (uint8_t *)p : nullptr, (planes & 2) ? (double *)p : nullptr, (planes & 4) ? (double *)p : nullptr, (planes & 8) ? (double *)p : nullptr,
                           (planes & 16) ? (uint32_t *)p : nullptr};
}

static void check_the_call() {
    int accel = 0;
    const double D[6] = {0, 0, 0, 0, 0, 0};
    const lg_segments_out all = subset(31, ASKED), none = subset(0, ASKED);
    const size_t HUGE_N = (size_t)-1;
    EXPECT(!throws([&] { check_segments(&accel, D, nullptr, 5, INF, &all); }));
    EXPECT(!throws([&] { check_segments(&accel, D, nullptr, 5, 0.0, &all); }));
    EXPECT(!throws([&] { check_segments(&accel, D, D, 5, -0.0, &all); }));
    EXPECT(!throws([&] { check_segments(&accel, D, nullptr, 5, -0.0, &all); })); // -0.0 is zero
    // every refusal, in its order: each call has every LATER fault too, and names the first
    EXPECT(thrown([&] { check_segments(nullptr, nullptr, nullptr, HUGE_N, -1.0, nullptr); }) == "accel is NULL");
    EXPECT(thrown([&] { check_segments(&accel, nullptr, nullptr, HUGE_N, -1.0, nullptr); }) == "segments is NULL");
    EXPECT(thrown([&] { check_segments(&accel, D, nullptr, HUGE_N, -1.0, nullptr); }) == "out is NULL");
    EXPECT(thrown([&] { check_segments(&accel, D, nullptr, HUGE_N, -1.0, &none); }).find("every plane of out is NULL") == 0);
    EXPECT(thrown([&] { check_segments(&accel, D, nullptr, HUGE_N, -1.0, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_segments(&accel, D, nullptr, HUGE_N, QNAN, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_segments(&accel, D, nullptr, HUGE_N, -INF, &all); }).find("radius is NaN or negative") == 0);
    EXPECT(thrown([&] { check_segments(&accel, D, nullptr, HUGE_N, INF, &all); }) == "too many segments in one query");
    EXPECT(thrown([&] { check_segments(&accel, D, nullptr, (size_t)(QUERY_MAX_RAYS + 1), 1.0, &all); }) == "too many segments in one query");
    EXPECT(!throws([&] { check_segments(&accel, D, nullptr, (size_t)QUERY_MAX_RAYS, 1.0, &all); }));
    // with radii the shared radius is neither read nor checked
    EXPECT(!throws([&] { check_segments(&accel, D, D, 5, -1.0, &all); }));
    EXPECT(!throws([&] { check_segments(&accel, D, D, 5, QNAN, &all); }));
    EXPECT(thrown([&] { check_segments(&accel, D, D, HUGE_N, QNAN, &all); }) == "too many segments in one query");
    for (int planes = 1; planes < 32; ++planes) { // each plane alone is enough; touch alone is the form that leaves at the first contact
        const lg_segments_out o = subset(planes, ASKED);
        EXPECT(!throws([&] { check_segments(&accel, D, nullptr, 5, 2.0, &o); }));
        EXPECT(segments_touch_only(o) == (planes == 1));
    }
    // the sizes: checked_bytes refuses what wraps
    EXPECT(thrown([&] { (void)checked_bytes(SIZE_MAX / 48 + 1, 48, "segments"); }) == "segments does not fit the address space");
    EXPECT(checked_bytes(SIZE_MAX / 48, 48, "segments") == SIZE_MAX / 48 * 48);
    // alignment: segments, radii, distance, param and point 8 bytes, id 16, touch any; NULL is not misaligned
    alignas(16) unsigned char mem[64];
    auto at = [&](size_t off) { return (void *)(mem + off); };
    EXPECT(!throws([&] { check_segments_alignment((double *)at(8), (double *)at(24), lg_segments_out{(uint8_t *)at(1), (double *)at(8), (double *)at(40), (double *)at(24), (uint32_t *)at(16)}); }));
    EXPECT(!throws([&] { check_segments_alignment((double *)at(8), nullptr, none); }));
    EXPECT(thrown([&] { check_segments_alignment((double *)at(4), nullptr, all); }) == "segments is not 8-byte aligned");
    EXPECT(thrown([&] { check_segments_alignment(D, (double *)at(4), all); }) == "radii is not 8-byte aligned");
    EXPECT(thrown([&] { check_segments_alignment(D, nullptr, lg_segments_out{nullptr, (double *)at(4), nullptr, nullptr, nullptr}); }) == "distance is not 8-byte aligned");
    EXPECT(thrown([&] { check_segments_alignment(D, nullptr, lg_segments_out{nullptr, nullptr, (double *)at(12), nullptr, nullptr}); }) == "param is not 8-byte aligned");
    EXPECT(thrown([&] { check_segments_alignment(D, nullptr, lg_segments_out{nullptr, nullptr, nullptr, (double *)at(12), nullptr}); }) == "point is not 8-byte aligned");
    EXPECT(thrown([&] { check_segments_alignment(D, nullptr, lg_segments_out{nullptr, nullptr, nullptr, nullptr, (uint32_t *)at(8)}); }) == "id is not 16-byte aligned");
    // the host form's staging, every subset of the planes, n up to a few tiles
    for (size_t n : {(size_t)1, (size_t)63, (size_t)65, (size_t)1025})
        for (int planes = 1; planes < 32; ++planes) {
            lg_segments_out o = subset(planes, ASKED);
            check_segments(&accel, D, nullptr, n, INF, &o);
            const StagedRound r = staged_round([&](auto &&f) { segments_planes(o, n, f); });
            EXPECT(r.plane_bytes.size() == 5);
            EXPECT(r.plane_bytes[0] == ((planes & 1) ? n : 0) && r.plane_bytes[1] == ((planes & 2) ? n * 8 : 0) && r.plane_bytes[2] == ((planes & 4) ? n * 8 : 0) &&
                   r.plane_bytes[3] == ((planes & 8) ? n * 24 : 0) && r.plane_bytes[4] == ((planes & 16) ? n * 16 : 0));
        }
}

int main() {
    check_the_call();
    if (failures) { std::fprintf(stderr, "segments_host_check: %d failures\n", failures); return 1; }
    std::printf("segments_host_check: ok\n");
    return 0;
}
