// lasgun_amd/csrc/k_query.hip -- ray queries (include/lasgun_hip.h, lg_intersect* / lg_occluded* / lg_camera_rays*): the caller's own rays
// through the render's walk (walk.h, walk<LDSS, FAST, PRUNE>), unchanged.
//
// One ray per lane, 64-ray tiles of the caller's array claimed by a persistent grid as the level-by-level traversal kernels claim theirs
// (kcommon.h: banded by XCD where the scene sits in LDS, one head word otherwise), a per-lane LDS stack, the scene image copied into LDS
// once per workgroup where the accel keeps it there.  A ray is 48 bytes in, read as three 16-byte loads; a closest hit is 96 bytes out
// (lg_hit), written as six 16-byte stores -- a wave writes 6 KiB in one piece; an occlusion answer is one byte.  Lanes past the last ray
// (n % 64) walk nothing and write nothing.  The prologue, the tile loop and the record writer are what tilewalk.h holds for the family's other
// tiled kernels; this file keeps its own text of them: over the shared header its rows measured slower than the parent's by more than
// its spread (profiles/tilewalk_account.md, profiles/tilewalk_ab.jsonl).
//
// PERM (lg_accel_set_query_order(1)): the tiles are cut from the SORTED order of the rays (k_sort.hip) -- slot s = tile * 64 + lane walks
// ray i = perm[s], read from rays[6i] and answered in hits[6i] / occluded[i]: no gathered copy of the rays, no scatter pass over the hits
// (either would move ~144 bytes a ray more).  perm is a permutation of 0 .. n-1, so every slot of the caller's arrays is written once.
#include "travform.h"

namespace lg {

struct QueryArgs {
    const double *rays;        // [n][6]: origin xyz, direction xyz (Ray3::new, ray.rs:28-33)
    unsigned long long n;
    uint4 *hits;               // closest hit: [n] lg_hit, 6 x uint4 each
    uint8_t *occluded;         // any-hit: [n]
    const uint32_t *tri_base;  // per accel: its mesh's first triangle in the triangle tables (a face number is the triangle index minus this)
    const uint32_t *perm;      // PERM forms only: [n], the ray walked in each slot
};

__device__ __forceinline__ uint4 bits2(double a, double b) {
    const unsigned long long x = (unsigned long long)__double_as_longlong(a), y = (unsigned long long)__double_as_longlong(b);
    return make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
}

// ANY = false: closest hit, resolved to world space as shading sees it (shade_frame), with the primitive's public identity;
// ANY = true: the shadow pass's any-hit walk, occluded = t < 1 (point.rs:49)
template <bool FAST, bool LDSS, bool PRUNE, bool ANY, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) query_kernel(const DParams P, const QueryArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ntiles = P.ntiles;
    if (ntiles == 0u) return; // (uniform: before the LDS copy and its barrier)
    uint32_t *stack = lds_stack + tid;
    constexpr uint32_t stride = LDSS ? LG_LDSS_BLOCK : LG_BLOCK;
    const uint4 *scn = nullptr;
    if (LDSS) {
        uint4 *dst = reinterpret_cast<uint4 *>(lds_stack + P.stack_depth * stride);
        copy_to_lds(dst, reinterpret_cast<const uint4 *>(P.lds_image), P.lds_image_n16, tid, stride);
        __syncthreads();
        scn = dst;
    }
    const uint4 *const arec = (LDSS || FAST) ? nullptr : load_accel_image(P, P.stack_depth * LG_BLOCK);
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    if (!wave_has_work(ntiles)) return;
    uint32_t band = LDSS ? xcc_id() : 0u, bands_left = TILE_HEADS;
    for (bool final = false; !final;) {
        uint32_t tile;
        if (LDSS) tile = claim_tile(P.tile_counter, ntiles, band, bands_left, final);
        else tile = claim_tile_single(P.tile_counter, ntiles, final);
        if (tile == NO_TILE) break;
        unsigned long long i = (unsigned long long)tile * 64ull + lane;
        const bool active = i < Q.n;
        if (PERM && active) i = Q.perm[i];
        Ray ray = ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0});
        if (active) {
            const double2 *r = reinterpret_cast<const double2 *>(Q.rays + 6ull * i);
            const double2 a = r[0], b = r[1], c = r[2];
            ray = ray_new(V3{a.x, a.y, b.x}, V3{b.y, c.x, c.y}); // Ray3::new: the direction as given
        }
        Best b;
        b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
        if (active) walk<LDSS, FAST, PRUNE>(P, ray, ANY, stack, stride, b, scn, cnt, arec);
        if (!active) continue;
        if (ANY) {
            Q.occluded[i] = b.t < 1.0 ? 1u : 0u; // point.rs:49
            continue;
        }
        uint4 *out = Q.hits + 6ull * i;
        if (b.ref == NO_HIT) {
            out[0] = bits2(INFINITY, 0.0); out[1] = bits2(0.0, 0.0); out[2] = bits2(0.0, 0.0);
            out[3] = bits2(0.0, 0.0); out[4] = bits2(0.0, 0.0);
            out[5] = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu); // kind 0, prim / instance ~0, material -1
            continue;
        }
        Shade sh;
        shade_frame(P, ray, b, sh);
        const uint32_t pk = b.ref >> 30, idx = b.ref & PRIM_INDEX_MASK;
        const uint32_t prim = pk == PK_TRIANGLE ? idx - Q.tri_base[b.accel] : idx;
        out[0] = bits2(b.t, sh.praw.x); out[1] = bits2(sh.praw.y, sh.praw.z);
        out[2] = bits2(sh.ng.x, sh.ng.y); out[3] = bits2(sh.ng.z, sh.ns.x); out[4] = bits2(sh.ns.y, sh.ns.z);
        out[5] = make_uint4(pk + 1u, prim, b.accel, (uint32_t)sh.mat); // lg_hit::kind: 1 sphere, 2 box, 3 triangle
    }
}

// Camera::sample for every sample of the pixels [x0, x1) x [y0, y1) (DParams' rectangle), row-major pixels, camera.rs sample order
__global__ void __launch_bounds__(LG_BLOCK) camera_rays_kernel(const DParams P, double *rays, unsigned long long n) {
    const uint32_t S = P.ss_root * P.ss_root, rw = P.x1 - P.x0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * LG_BLOCK) {
        const unsigned long long pix = i / S;
        const uint32_t s = (uint32_t)(i - pix * S);
        const uint32_t x = P.x0 + (uint32_t)(pix % rw), y = P.y0 + (uint32_t)(pix / rw);
        const Ray r = camera_ray(P, x, y, s);
        double2 *o = reinterpret_cast<double2 *>(rays + 6ull * i);
        o[0] = make_double2(r.o.x, r.o.y); o[1] = make_double2(r.o.z, r.d.x); o[2] = make_double2(r.d.y, r.d.z);
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's.  Variants: ANY x PERM
template <bool F, bool L, bool Z> struct QueryKernels {
    static constexpr int variants = 4;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(query_kernel<F, L, Z, false, false>), reinterpret_cast<const void *>(query_kernel<F, L, Z, true, false>),
                                   reinterpret_cast<const void *>(query_kernel<F, L, Z, false, true>), reinterpret_cast<const void *>(query_kernel<F, L, Z, true, true>)};
        return k[v];
    }
};
// occluded != nullptr: the any-hit variants; perm != nullptr: the PERM variants
hipError_t launch_query(const DParams &P, const double *rays, unsigned long long n, void *hits, uint8_t *occluded, const uint32_t *tri_base,
                        const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const QueryArgs Q{rays, n, reinterpret_cast<uint4 *>(hits), occluded, tri_base, perm};
    void *args[] = {const_cast<DParams *>(&P), const_cast<QueryArgs *>(&Q)};
    return trav_launch<QueryKernels>(P, fast, (occluded ? 1 : 0) + (perm ? 2 : 0), blocks, stack_depth, args, stream);
}
hipError_t launch_camera_rays(const DParams &P, double *rays, unsigned long long n, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, rays, n);
    return hipGetLastError();
}
hipError_t query_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<QueryKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t query_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<QueryKernels>(bytes, ldss); }

} // namespace lg
