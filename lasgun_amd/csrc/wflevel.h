// lasgun_amd/csrc/wflevel.h -- what the kernels of the level-by-level pipeline share (k_wavefront.hip: the render's levels; k_radiance.hip:
// level 0 of a radiance query): wave-wide appends, a level's ray queue, and the two-part hit queue of a level.
#pragma once
#include "shade.h"

namespace lg {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) { // number of set bits of `mask` below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// one slot per lane of `mask` in a queue whose fill count is *counter: consecutive slots, one atomic per wavefront
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, bool want) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(want);
    if (mask == 0ull) return 0u;
    uint32_t base = 0u;
    const uint32_t leader = (uint32_t)__builtin_ctzll(mask);
    if ((threadIdx.x & 63u) == leader) base = atomicAdd(counter, (uint32_t)__builtin_popcountll(mask));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);
    return base + lanes_below(mask);
}
__device__ __forceinline__ Ray wf_load_ray(const DParams &P, unsigned long long j) {
    const unsigned long long n = P.wf_cap;
    const double *q = P.wf_q + j;
    return ray_new(V3{q[0 * n], q[1 * n], q[2 * n]}, V3{q[3 * n], q[4 * n], q[5 * n]}); // Ray3::new (ray.rs:28-33)
}
// The hit queue of a level has two parts.  A wavefront most of whose lanes hit (>= WF_FULL_MIN) keeps its hits where its
// rays are: slot = ray index, no atomic, holes marked WF_NONE -- the block IS the 8x8 tile (or the 64 consecutive queue rays),
// so the shadow pass walks the same coherent rays, and packing 61 + 3 lanes of two tiles into one wave would cost more than
// three idle lanes.  Every other wavefront marks its block empty and appends just its hits, compacted (ballot + popcount
// prefix, one atomic per wavefront), behind the dense part: sparse hits -- a small object in front of the background, the
// secondary rays of a glass object -- become full waves for the shadow and shade passes.
constexpr uint32_t WF_FULL_MIN = 48u;
// Rays per work tile of a level (a hook: a level with few, incoherent rays could be cut into tiles of fewer rays).
__device__ __forceinline__ uint32_t wf_lanes_per_tile(unsigned long long rays) {
    (void)rays;
    return 64u; // measured: narrower tiles (8 .. 32 rays per wave for levels of < 2^19 rays) do not help the mesh configs and cost the small scenes 30-80 %
}
struct HitSlots { // work tile t of a pass over the hit queue -> hit index of this lane (valid or not)
    unsigned long long n_rays, n_part;
    uint32_t tiles_dense, tiles, lpt;
};
__device__ __forceinline__ unsigned long long wf_level_rays(const DParams &P, uint32_t level) {
    if (level == 0u) return (unsigned long long)P.ntiles * 64ull;
    return P.q_ctl ? (unsigned long long)P.q_ctl[QC_LEVEL0 + QC_LEVEL_WORDS * level + QC_COUNT] * 64ull : P.wf_counts[level]; // (the queue organisation counts 64-ray packets)
}
__device__ __forceinline__ HitSlots hit_slots(const DParams &P, uint32_t level, uint32_t lpt) {
    HitSlots s;
    s.lpt = lpt;
    s.n_part = P.wf_counts[P.wf_levels + level];
    s.n_rays = wf_level_rays(P, level);
    s.tiles_dense = (uint32_t)((s.n_rays + lpt - 1u) / lpt);
    s.tiles = s.tiles_dense + (uint32_t)((s.n_part + lpt - 1u) / lpt);
    return s;
}
__device__ __forceinline__ bool hit_of(const DParams &P, const HitSlots &s, uint32_t tile, uint32_t lane, unsigned long long &h) {
    if (lane >= s.lpt) return false;
    if (tile < s.tiles_dense) {
        h = (unsigned long long)tile * s.lpt + lane;
        return h < s.n_rays && P.wf_hq[h] != WF_NONE;
    }
    const unsigned long long k = (unsigned long long)(tile - s.tiles_dense) * s.lpt + lane;
    h = P.wf_hit_cap + k;
    return k < s.n_part;
}
// ... for the shadow pass: `skip` = the closest pass flagged the hit (WF_SKIP) -- it has no shadow ray to walk and its visibility is written
__device__ __forceinline__ bool hit_of(const DParams &P, const HitSlots &s, uint32_t tile, uint32_t lane, unsigned long long &h, bool &skip) {
    skip = false;
    if (lane >= s.lpt) return false;
    uint32_t word = WF_NONE;
    if (tile < s.tiles_dense) {
        h = (unsigned long long)tile * s.lpt + lane;
        if (h < s.n_rays) word = P.wf_hq[h];
    } else {
        const unsigned long long k = (unsigned long long)(tile - s.tiles_dense) * s.lpt + lane;
        h = P.wf_hit_cap + k;
        if (k < s.n_part) word = P.wf_hq[h];
    }
    if (word == WF_NONE) return false; // (an appended hit's word is its ray index, never WF_NONE)
    skip = (word & WF_SKIP) != 0u;
    return true;
}
// the ray index of a hit's wf_hq word
__device__ __forceinline__ uint32_t hq_ray(uint32_t word) { return word & ~WF_SKIP; }

} // namespace lg
