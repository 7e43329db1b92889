// lasgun_amd/csrc/k_attributes.hip -- hit attributes (include/lasgun_hip.h, lg_hit_attributes* / lg_hit_attributes_of*): where on the primitive
// a ray's hit lies -- barycentrics, (u, v), the local point -- and the frame the render shades it in -- the BSDF's tangents, the geometric
// dpdu / dpdv --, as planes indexed by the ray.  What resolve_hit / triangle_full / sphere_full / cuboid_hit<true> compute for every shaded
// hit and drop; attr_resolve.h restates them with it kept.
//
// attr_kernel, the walking form: query_kernel's closest form (k_query.hip) -- its prologue, its tile claim (in this file's own text, not
// over tilewalk.h: over the shared header a row of this family measured slower, profiles/tilewalk_account.md), one ray per lane, 64-ray tiles
// of the caller's array, the grid sized in query.cpp (traversal_grid), the forms launched through travform.h, PERM as there, the record
// resolved by shade_frame and written as six 16-byte stores -- with the attribute planes behind it.  The walk is walk<LDSS, FAST, PRUNE>,
// unchanged.  The evaluation that fills the record has query_kernel's uses and no others; the planes come from a second evaluation of the
// hit behind an optimisation barrier (attr_planes_of): with the tangents live beside the record the compiler is free to form a component
// of ng or ns by another route -- the same number, but where the hit's geometry is NaN another NaN sign, and the record would no longer be
// lg_intersect's bit for bit (k_layers.hip, layer_next_origin, met this first).
//
// attr_of_kernel, the _of form: no walk, no LDS: a grid-stride loop over the records, each checked by attr_record_ok (attributes_host.h,
// the function the host check runs) before anything is read through it, then resolved for its ray.
//
// Every element of every plane asked for is written by exactly one lane: no atomics, no pre-fill.  Lanes past the last ray walk nothing
// and write nothing.
#include "attr_resolve.h"
#include "attributes_host.h"
#include "travform.h"

namespace lg {

struct AttrArgs {
    const double *rays;        // [n][6]: origin xyz, direction xyz, as for lg_intersect
    unsigned long long n;
    uint4 *hits;               // [n] lg_hit, 6 x uint4 each; may be nullptr (as every plane); the _of form: nullptr
    uint32_t *flags;           // [n]
    double *bary;              // [n][3]
    double *uv;                // [n][2]
    double *local;             // [n][3]
    double *frame;             // [n][6]
    double *dp;                // [n][6]
    const uint32_t *tri_base;  // walking form: per accel, its mesh's first triangle in the triangle tables (k_query.hip)
    const uint32_t *perm;      // PERM forms only: [n], the ray walked in each slot
    const uint4 *records;      // _of form: [n] lg_hit, of which the last 16 bytes (kind, prim, instance, material) are read
    const uint32_t *counts;    // _of form: the counts table (attributes_host.h)
};

__device__ __forceinline__ uint4 attr_bits2(double a, double b) {
    const unsigned long long x = (unsigned long long)__double_as_longlong(a), y = (unsigned long long)__double_as_longlong(b);
    return make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
}
__device__ __forceinline__ double attr_opaque(double x) {
    asm volatile("" : "+v"(x));
    return x;
}
// the planes of ray i behind the record: flags, then what is asked for of `at`
__device__ __forceinline__ void attr_store(const AttrArgs &Q, unsigned long long i, uint32_t flags, const HitAttr &at) {
    if (Q.flags) Q.flags[i] = flags;
    if (Q.bary) { double *o = Q.bary + 3ull * i; o[0] = at.b0; o[1] = at.b1; o[2] = at.b2; }
    if (Q.uv) { double *o = Q.uv + 2ull * i; o[0] = at.u; o[1] = at.v; }
    if (Q.local) { double *o = Q.local + 3ull * i; o[0] = at.local.x; o[1] = at.local.y; o[2] = at.local.z; }
    if (Q.frame) { double *o = Q.frame + 6ull * i; o[0] = at.ss.x; o[1] = at.ss.y; o[2] = at.ss.z; o[3] = at.ts.x; o[4] = at.ts.y; o[5] = at.ts.z; }
    if (Q.dp) { double *o = Q.dp + 6ull * i; o[0] = at.gu.x; o[1] = at.gu.y; o[2] = at.gu.z; o[3] = at.gv.x; o[4] = at.gv.y; o[5] = at.gv.z; }
}
// The planes of the hit `b` of ray `r`, from an evaluation of their own: the ray goes through the barrier, so nothing of it is shared with
// the evaluation that filled the record.  (The walk accepted the primitive by the very tests attr_resolve repeats; were one to disagree,
// the planes would be zeros, never an unset register.)
__device__ __forceinline__ HitAttr attr_planes_of(const DParams &P, const Ray &r, const Best &b) {
    const Ray ray = ray_new(V3{attr_opaque(r.o.x), attr_opaque(r.o.y), attr_opaque(r.o.z)}, V3{attr_opaque(r.d.x), attr_opaque(r.d.y), attr_opaque(r.d.z)});
    HitAttr at;
    if (!attr_resolve(P, ray, b.ref >> 30, b.ref & PRIM_INDEX_MASK, b.accel, at)) at = attr_zero();
    return at;
}

template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) attr_kernel(const DParams P, const AttrArgs Q) {
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
        if (active) walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
        if (!active) continue;
        if (b.ref == NO_HIT) {
            if (Q.hits) {
                uint4 *out = Q.hits + 6ull * i;
                out[0] = attr_bits2(INFINITY, 0.0); out[1] = attr_bits2(0.0, 0.0); out[2] = attr_bits2(0.0, 0.0);
                out[3] = attr_bits2(0.0, 0.0); out[4] = attr_bits2(0.0, 0.0);
                out[5] = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu); // kind 0, prim / instance ~0, material -1
            }
            attr_store(Q, i, 0u, attr_zero());
            continue;
        }
        if (Q.hits) { // the record: query_kernel's evaluation, its uses alone
            Shade sh;
            shade_frame(P, ray, b, sh);
            const uint32_t pk = b.ref >> 30, idx = b.ref & PRIM_INDEX_MASK;
            const uint32_t prim = pk == PK_TRIANGLE ? idx - Q.tri_base[b.accel] : idx;
            uint4 *out = Q.hits + 6ull * i;
            out[0] = attr_bits2(b.t, sh.praw.x); out[1] = attr_bits2(sh.praw.y, sh.praw.z);
            out[2] = attr_bits2(sh.ng.x, sh.ng.y); out[3] = attr_bits2(sh.ng.z, sh.ns.x); out[4] = attr_bits2(sh.ns.y, sh.ns.z);
            out[5] = make_uint4(pk + 1u, prim, b.accel, (uint32_t)sh.mat); // lg_hit::kind: 1 sphere, 2 box, 3 triangle
        }
        attr_store(Q, i, ATTR_HIT, attr_planes_of(P, ray, b));
    }
}

// The _of form: record i names (kind, prim, instance); checked, then resolved for ray i.  One record per lane, grid-stride.
__global__ void __launch_bounds__(LG_BLOCK) attr_of_kernel(const DParams P, const AttrArgs Q) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; i < Q.n; i += (unsigned long long)gridDim.x * LG_BLOCK) {
        const uint4 id = Q.records[6ull * i + 5ull]; // kind, prim, instance, material
        uint32_t flags = 0u;
        HitAttr at = attr_zero();
        if (id.x != 0u) {
            if (!attr_record_ok(Q.counts, id.x, id.y, id.z)) flags = ATTR_BAD_RECORD;
            else {
                const double2 *r = reinterpret_cast<const double2 *>(Q.rays + 6ull * i);
                const double2 a = r[0], b = r[1], c = r[2];
                const Ray ray = ray_new(V3{a.x, a.y, b.x}, V3{b.y, c.x, c.y}); // Ray3::new: the direction as given
                const uint32_t pk = id.x - 1u;
                const uint32_t idx = pk == PK_TRIANGLE ? attr_triangle_index(Q.counts, id.y, id.z) : id.y;
                HitAttr got;
                if (attr_resolve(P, ray, pk, idx, id.z, got)) { flags = ATTR_HIT; at = got; }
                else flags = ATTR_NO_HIT;
            }
        }
        attr_store(Q, i, flags, at);
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's.  Variants: as given, permuted
template <bool F, bool L, bool Z> struct AttrKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(attr_kernel<F, L, Z, false>), reinterpret_cast<const void *>(attr_kernel<F, L, Z, true>)};
        return k[v];
    }
};
// perm != nullptr: the PERM variant; every plane may be nullptr
hipError_t launch_attributes(const DParams &P, const double *rays, unsigned long long n, void *hits, uint32_t *flags, double *bary, double *uv, double *local,
                             double *frame, double *dp, const uint32_t *tri_base, const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth,
                             hipStream_t stream) {
    const AttrArgs Q{rays, n, reinterpret_cast<uint4 *>(hits), flags, bary, uv, local, frame, dp, tri_base, perm, nullptr, nullptr};
    void *args[] = {const_cast<DParams *>(&P), const_cast<AttrArgs *>(&Q)};
    return trav_launch<AttrKernels>(P, fast, perm ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t launch_attr_of(const DParams &P, const double *rays, const void *records, unsigned long long n, const uint32_t *counts, uint32_t *flags, double *bary,
                          double *uv, double *local, double *frame, double *dp, uint32_t blocks, hipStream_t stream) {
    const AttrArgs Q{rays, n, nullptr, flags, bary, uv, local, frame, dp, nullptr, nullptr, reinterpret_cast<const uint4 *>(records), counts};
    hipLaunchKernelGGL(attr_of_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t attributes_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<AttrKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t attributes_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<AttrKernels>(bytes, ldss); }

} // namespace lg
