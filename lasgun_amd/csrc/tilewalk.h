// lasgun_amd/csrc/tilewalk.h -- the device side that the tiled traversal kernels of the query family share (travform.h is their host side):
// the prologue and the tile cursor of a kernel that walks 64-item tiles claimed by a persistent grid, and the small values every such kernel
// forms -- the ray of a [n][6] buffer, the fresh Best, the lg_hit record and its id word.  The render's own kernels (k_wavefront.hip,
// k_mega.hip, k_queue.hip) do not use this.
//
// The rules below are rules of the whole family, and they stand here once:
//   * the LDS copy's barrier is reached by every wave of the workgroup: the only exit ahead of it is the uniform one of an empty launch;
//   * a launch of n tiles is claimed by the first n waves (wave_has_work, kcommon.h), asked only behind the barrier;
//   * tiles are claimed banded by XCD where the scene sits in LDS, from one head word otherwise, and "final" tiles -- a wave that has had
//     one leaves without asking again -- exist in small launches only (kcommon.h says how a launch ends);
//   * the evaluation of shade_frame that fills an lg_hit record has query_kernel's uses (k_query.hip) and no others: with more of Shade live
//     beside it the compiler forms components of ng or ns by other routes -- the same numbers, but other NaN signs.  A kernel that wants more
//     of the hit takes it from an evaluation of its own on ray_opaque's copy of the ray.
// A kernel keeps its Counters instance and calls walk<LDSS, FAST, PRUNE>(P, ray, any, tw.stack, tw.stride, b, tw.scn, cnt, tw.arec) itself.
// Over this header: k_layers.hip, k_paths.hip, k_features.hip, k_directions.hip, k_visibility.hip.  The family's other tiled kernels
// (k_query.hip, k_scan.hip, k_attributes.hip, k_view_features.hip, level0.h's closest body, rq_closest_body.h, k_lit.hip's shadow pass)
// keep this text in their own files: over the header rows of theirs measured slower than the parent's by more than its spread across
// repeats, which is the rule the project shares device text by (profiles/tilewalk_account.md; level0.h set the precedent).
#pragma once
#include "shade.h"

namespace lg {

template <bool FAST, bool LDSS> struct TileWalk {
    static constexpr uint32_t stride = LDSS ? LG_LDSS_BLOCK : LG_BLOCK; // the per-entry stride of the lane's stack
    uint32_t *stack;   // the lane's stack in LDS
    const uint4 *scn;  // the scene image in LDS (LDSS), nullptr otherwise
    const uint4 *arec; // the accel records in LDS (256-lane reference walk), nullptr otherwise
    uint32_t ntiles, band, bands_left;

    // the prologue: false when the wave has nothing to do.  `tiles`: the launch's tile count, the same in every lane of the grid
    __device__ __forceinline__ bool begin(const DParams &P, uint32_t tiles) {
        const uint32_t tid = threadIdx.x;
        ntiles = tiles;
        if (ntiles == 0u) return false; // (uniform: before the LDS copy and its barrier)
        stack = lds_stack + tid;
        scn = nullptr;
        if (LDSS) {
            uint4 *dst = reinterpret_cast<uint4 *>(lds_stack + P.stack_depth * stride);
            copy_to_lds(dst, reinterpret_cast<const uint4 *>(P.lds_image), P.lds_image_n16, tid, stride);
            __syncthreads(); // the only workgroup-wide step; every wave reaches it before pulling tiles
            scn = dst;
        }
        arec = (LDSS || FAST) ? nullptr : load_accel_image(P, P.stack_depth * LG_BLOCK);
        if (!wave_has_work(ntiles)) return false;
        band = LDSS ? xcc_id() : 0u;
        bands_left = TILE_HEADS;
        return true;
    }
    __device__ __forceinline__ bool begin(const DParams &P) { return begin(P, P.ntiles); }
    // the cursor: the next tile of this wave, the same in every lane, or NO_TILE; `final` comes back true for a final tile.  The loop is
    //     for (bool final = false; !final;) { const uint32_t tile = tw.next(P, final); if (tile == NO_TILE) break; ... }
    __device__ __forceinline__ uint32_t next(const DParams &P, bool &final) {
        if (LDSS) return claim_tile(P.tile_counter, ntiles, band, bands_left, final);
        return claim_tile_single(P.tile_counter, ntiles, final);
    }
};

// ray i of a [n][6] buffer (origin xyz, direction xyz): 48 bytes as three 16-byte loads
__device__ __forceinline__ Ray load_ray(const double *rays, unsigned long long i) {
    const double2 *r = reinterpret_cast<const double2 *>(rays + 6ull * i);
    const double2 a = r[0], b = r[1], c = r[2];
    return ray_new(V3{a.x, a.y, b.x}, V3{b.y, c.x, c.y}); // Ray3::new: the direction as given
}
// what an inactive lane holds in the ray's registers: it is never walked
__device__ __forceinline__ Ray idle_ray() { return ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0}); }
__device__ __forceinline__ Best fresh_best() {
    Best b;
    b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
    return b;
}
// a copy of the ray that the compiler cannot see through: an evaluation on it shares nothing with one on the ray itself
__device__ __forceinline__ double opaque(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ Ray ray_opaque(const Ray &r) {
    return ray_new(V3{opaque(r.o.x), opaque(r.o.y), opaque(r.o.z)}, V3{opaque(r.d.x), opaque(r.d.y), opaque(r.d.z)});
}

// ---- the lg_hit record (include/lasgun_hip.h): 96 bytes as six 16-byte stores, the last of them the id word
__device__ __forceinline__ uint4 bits2(double a, double b) {
    const unsigned long long x = (unsigned long long)__double_as_longlong(a), y = (unsigned long long)__double_as_longlong(b);
    return make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
}
// kind, prim, instance, material of a hit; tri_base: per accel, its mesh's first triangle in the triangle tables (a face number is the
// triangle index minus this)
__device__ __forceinline__ uint4 hit_id(const Best &b, const Shade &sh, const uint32_t *tri_base) {
    const uint32_t pk = b.ref >> 30, idx = b.ref & PRIM_INDEX_MASK;
    const uint32_t prim = pk == PK_TRIANGLE ? idx - tri_base[b.accel] : idx;
    return make_uint4(pk + 1u, prim, b.accel, (uint32_t)sh.mat); // lg_hit::kind: 1 sphere, 2 box, 3 triangle
}
__device__ __forceinline__ uint4 hit_id_none() { return make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu); } // kind 0, prim / instance ~0, material -1
// the record of a hit resolved by shade_frame: of Shade it reads praw, ng and ns, and mat through `id` (hit_id), nothing else
__device__ __forceinline__ void store_hit(uint4 *out, const Best &b, const Shade &sh, const uint4 id) {
    out[0] = bits2(b.t, sh.praw.x); out[1] = bits2(sh.praw.y, sh.praw.z);
    out[2] = bits2(sh.ng.x, sh.ng.y); out[3] = bits2(sh.ng.z, sh.ns.x); out[4] = bits2(sh.ns.y, sh.ns.z);
    out[5] = id;
}
__device__ __forceinline__ void store_hit_none(uint4 *out) {
    out[0] = bits2(INFINITY, 0.0); out[1] = bits2(0.0, 0.0); out[2] = bits2(0.0, 0.0);
    out[3] = bits2(0.0, 0.0); out[4] = bits2(0.0, 0.0);
    out[5] = hit_id_none();
}

} // namespace lg
