// lasgun_amd/csrc/raykey.h -- the 32-bit coherence key of a query ray (include/lasgun_hip.h, lg_query_order*; k_sort.hip sorts by it).
// Host and device code: nothing here but <cmath> / <cstdint> arithmetic.
//
// Rays that sit next to each other in key order should walk the same nodes.  Two things decide which nodes a ray meets: where it starts
// and where it points.  The key carries both:
//   bits 31..20  the origin's cell in a 16 x 16 x 16 grid over the scene's world bounds (the root accel's box), Morton order, clamped
//   bits 19..0   the direction's cell in a 1024 x 1024 grid over the octahedral map of d / |d|_1, Morton order
// Origin-major: shadow segments and probes start all over the scene and the origin separates them; camera rays share one origin cell and
// are ordered by direction alone, at a resolution (1024^2 over the sphere) that keeps a 4096^2 film's cells a few dozen pixels wide.
// Measured against direction-major (the same two fields swapped) and a 5-D Morton code of 6 origin + 7 direction bits per axis, 4096^2
// rays (profiles/r08_query_key_ab.jsonl): shuffled shadow segments 4.5 / 7.2 / 9.0 ms on the three scenes against 4.6 / 7.9 / 10.5 and
// 4.8 / 8.0 / 10.4; shuffled camera rays 4.5 / 7.6 / 10.0 ms against 4.3 / 7.4 / 9.9 and 5.3 / 10.5 / 15.6.
//
// The key is not part of the parity contract -- a bad key costs time, never correctness -- so any f64 input gives SOME key, the same one
// every time: every clamp is written fmin(fmax(x, 0), top), and fmax returns its other operand when x is NaN, so NaN, a zero direction
// (0 / 0) and an origin at infinity minus infinity fall to cell 0; +-infinity and far-away origins clamp to a border cell.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LG_KEY_HD __host__ __device__ inline
#else
#define LG_KEY_HD inline
#endif

namespace lg {

constexpr uint32_t KEY_ORIGIN_BITS = 4u;  // per axis
constexpr uint32_t KEY_DIR_BITS = 10u;    // per axis of the octahedral map
constexpr uint32_t KEY_BITS = 3u * KEY_ORIGIN_BITS + 2u * KEY_DIR_BITS; // 32: what the sort has to look at

// The scene's world bounds as the key uses them: cell = (o - lo) * scale * cells, scale = 1 / (hi - lo) (0 for an empty or non-finite extent)
struct KeyBounds {
    double lo[3];
    double scale[3];
};
inline KeyBounds key_bounds(const double lo[3], const double hi[3]) {
    KeyBounds b{};
    for (int k = 0; k < 3; ++k) {
        const double e = hi[k] - lo[k];
        b.lo[k] = std::isfinite(lo[k]) ? lo[k] : 0.0;
        b.scale[k] = std::isfinite(e) && e > 0.0 && std::isfinite(lo[k]) ? 1.0 / e : 0.0;
    }
    return b;
}

LG_KEY_HD uint32_t key_cell(double x, uint32_t cells) { // floor(x) clamped to 0 .. cells-1; NaN -> 0
    return (uint32_t)fmin(fmax(x, 0.0), (double)(cells - 1u));
}
LG_KEY_HD uint32_t key_spread2(uint32_t v) { // 16 bits -> every other bit
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}
LG_KEY_HD uint32_t key_spread3(uint32_t v) { // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// r: origin xyz, direction xyz
LG_KEY_HD uint32_t ray_key(const double r[6], const KeyBounds &b) {
    constexpr uint32_t OC = 1u << KEY_ORIGIN_BITS, DC = 1u << KEY_DIR_BITS;
    const double fx = (r[0] - b.lo[0]) * b.scale[0], fy = (r[1] - b.lo[1]) * b.scale[1], fz = (r[2] - b.lo[2]) * b.scale[2];
    const uint32_t ox = key_cell(fx * (double)OC, OC), oy = key_cell(fy * (double)OC, OC), oz = key_cell(fz * (double)OC, OC);
    // octahedral map: project on the octahedron |x| + |y| + |z| = 1, unfold the lower half over the upper one's square
    const double l1 = (fabs(r[3]) + fabs(r[4])) + fabs(r[5]);
    double px = r[3] / l1, py = r[4] / l1;
    if (r[5] < 0.0) {
        const double qx = (1.0 - fabs(py)) * copysign(1.0, px), qy = (1.0 - fabs(px)) * copysign(1.0, py);
        px = qx; py = qy;
    }
    const uint32_t u = key_cell((px * 0.5 + 0.5) * (double)DC, DC), v = key_cell((py * 0.5 + 0.5) * (double)DC, DC);
    const uint32_t okey = key_spread3(ox) | (key_spread3(oy) << 1) | (key_spread3(oz) << 2);
    const uint32_t dkey = key_spread2(u) | (key_spread2(v) << 1);
    return (okey << (2u * KEY_DIR_BITS)) | dkey;
}

} // namespace lg
