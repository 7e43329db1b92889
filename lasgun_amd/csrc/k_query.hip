// lasgun_amd/csrc/k_query.hip -- ray queries (include/lasgun_hip.h, lg_intersect* / lg_occluded* / lg_camera_rays*): the caller's own rays
// through the render's walk (walk.h, walk<LDSS, FAST, PRUNE>), unchanged.
//
// One ray per lane, 64-ray tiles of the caller's array claimed by a persistent grid as the level-by-level traversal kernels claim theirs
// (kcommon.h: banded by XCD where the scene sits in LDS, one head word otherwise), a per-lane LDS stack, the scene image copied into LDS
// once per workgroup where the accel keeps it there.  A ray is 48 bytes in, read as three 16-byte loads; a closest hit is 96 bytes out
// (lg_hit), written as six 16-byte stores -- a wave writes 6 KiB in one piece; an occlusion answer is one byte.  Lanes past the last ray
// (n % 64) walk nothing and write nothing.
//
// PERM (lg_accel_set_query_order(1)): the tiles are cut from the SORTED order of the rays (k_sort.hip) -- slot s = tile * 64 + lane walks
// ray i = perm[s], read from rays[6i] and answered in hits[6i] / occluded[i]: no gathered copy of the rays, no scatter pass over the hits
// (either would move ~144 bytes a ray more).  perm is a permutation of 0 .. n-1, so every slot of the caller's arrays is written once.
#include "shade.h"

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

// ---- host-callable launchers (query.cpp).  The same (FAST, LDSS, PRUNE) forms as wf_trace_kernel, LDS sized as launch_wf_trace sizes it.
// perm != nullptr: the PERM forms
hipError_t launch_query(const DParams &P, const double *rays, unsigned long long n, void *hits, uint8_t *occluded, const uint32_t *tri_base,
                        const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const QueryArgs Q{rays, n, reinterpret_cast<uint4 *>(hits), occluded, tri_base, perm};
    const bool any = occluded != nullptr;
    const bool ldss = P.lds_image && !fast;
    const uint32_t block = ldss ? LG_LDSS_BLOCK : LG_BLOCK;
    const uint32_t depth = fast ? stack_depth : P.stack_depth;
    const size_t lds = (size_t)depth * block * sizeof(uint32_t) + (ldss ? (size_t)P.lds_image_n16 * 16u : (!fast && P.accel_image ? (size_t)P.accel_image_n16 * 16u : 0u));
#define LG_QP(F, L, Z, A) do { if (perm) hipLaunchKernelGGL((query_kernel<F, L, Z, A, true>), dim3(blocks), dim3(block), lds, stream, P, Q); \
                               else hipLaunchKernelGGL((query_kernel<F, L, Z, A, false>), dim3(blocks), dim3(block), lds, stream, P, Q); } while (0)
#define LG_Q(F, L, Z) do { if (any) LG_QP(F, L, Z, true); else LG_QP(F, L, Z, false); } while (0)
    if (fast) LG_Q(true, false, false);
    else if (P.prune) { if (ldss) LG_Q(false, true, true); else LG_Q(false, false, true); }
    else { if (ldss) LG_Q(false, true, false); else LG_Q(false, false, false); }
#undef LG_Q
#undef LG_QP
    return hipGetLastError();
}
hipError_t launch_camera_rays(const DParams &P, double *rays, unsigned long long n, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, rays, n);
    return hipGetLastError();
}
// workgroups per CU of the 256-lane forms (the smallest of closest and any-hit, as given and permuted)
template <bool FAST, bool PRUNE> static hipError_t query_occupancy_of(size_t lds, int *blocks_per_cu) {
    const void *fns[] = {reinterpret_cast<const void *>(query_kernel<FAST, false, PRUNE, false, false>), reinterpret_cast<const void *>(query_kernel<FAST, false, PRUNE, true, false>),
                         reinterpret_cast<const void *>(query_kernel<FAST, false, PRUNE, false, true>), reinterpret_cast<const void *>(query_kernel<FAST, false, PRUNE, true, true>)};
    int least = 0;
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; ++i) {
        int v = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, fns[i], LG_BLOCK, lds);
        if (e != hipSuccess) return e;
        if (i == 0 || v < least) least = v;
    }
    *blocks_per_cu = least;
    return hipSuccess;
}
hipError_t query_occupancy(uint32_t stack_depth, bool fast, bool prune, size_t extra_lds, int *blocks_per_cu) {
    const size_t lds = (size_t)stack_depth * LG_BLOCK * sizeof(uint32_t) + (fast ? 0u : extra_lds);
    if (fast) return query_occupancy_of<true, false>(lds, blocks_per_cu);
    if (prune) return query_occupancy_of<false, true>(lds, blocks_per_cu);
    return query_occupancy_of<false, false>(lds, blocks_per_cu);
}
// raise the dynamic-LDS limit of this file's traversal kernels to `bytes` (ldss: the LDS-resident-scene forms; otherwise the 256-lane forms)
template <bool FAST, bool LDSS, bool PRUNE> static hipError_t query_lds_limit_of(int bytes) {
    const void *fns[] = {reinterpret_cast<const void *>(query_kernel<FAST, LDSS, PRUNE, false, false>), reinterpret_cast<const void *>(query_kernel<FAST, LDSS, PRUNE, true, false>),
                         reinterpret_cast<const void *>(query_kernel<FAST, LDSS, PRUNE, false, true>), reinterpret_cast<const void *>(query_kernel<FAST, LDSS, PRUNE, true, true>)};
    for (const void *f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t query_set_lds_limit(size_t bytes, bool ldss) {
    hipError_t e;
    if (ldss) {
        e = query_lds_limit_of<false, true, false>((int)bytes);
        if (e == hipSuccess) e = query_lds_limit_of<false, true, true>((int)bytes);
        return e;
    }
    e = query_lds_limit_of<false, false, false>((int)bytes);
    if (e == hipSuccess) e = query_lds_limit_of<false, false, true>((int)bytes);
    if (e == hipSuccess) e = query_lds_limit_of<true, false, false>((int)bytes);
    return e;
}

} // namespace lg
