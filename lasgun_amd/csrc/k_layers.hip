// lasgun_amd/csrc/k_layers.hip -- hit layers (include/lasgun_hip.h, lg_hit_layers*): the first max_layers surfaces along each of the caller's
// rays in one launch.  Layer j of ray i is what lg_intersect returns for segment j; segment 0 is the ray as given, segment j+1 starts at
// layer j's p - ng * 2^-36 -- shade_frame's pm (shade.h), the origin the render gives a glass hit's transmitted ray -- and keeps the
// direction's bits.  The ray stays in registers between the walks; only the planes asked for are written.
//
// The kernel's prologue, tile cursor and record writer are tilewalk.h's, its work item query_kernel's (k_query.hip): one ray per lane, 64-ray
// tiles of the caller's array, the grid sized in query.cpp (traversal_grid), the forms launched through travform.h, PERM as there.  The walk is closest hit:
// walk<LDSS, FAST, PRUNE>(.., any = false, ..), unchanged, with a fresh Best per segment, and a hit is resolved as query_kernel resolves
// it (shade_frame, the face number through tri_base; layer_next_origin says why pm is evaluated apart).  What lives across the walks
// besides the ray: T (the running parameter), inside (t_1 + t_3 + ..) and count -- 5 VGPRs; nothing is parked in memory.  Lanes are not
// re-packed when rays end: a wave walks while any of its lanes is alive, a lane that missed writes the miss values of the layers its wave
// still walks, and the layers no lane of the wave reached are filled after the loop.
//
// Out, layer-major: element (j, i) at j * n + i.  hits: the 96-byte lg_hit as six 16-byte stores; id: its last 16 bytes as one store;
// along: one 8-byte store; count and inside: once per ray, after the loop.  Every element of every plane asked for is written by exactly
// one lane: no atomics, no pre-fill.  Lanes past the last ray (n % 64) walk nothing and write nothing.
#include "travform.h"
#include "tilewalk.h"

namespace lg {

struct LayersArgs {
    const double *rays;        // [n][6]: origin xyz, direction xyz, as for lg_intersect
    unsigned long long n;
    uint32_t max_layers;       // K >= 1
    uint4 *hits;               // [K][n] lg_hit, 6 x uint4 each; may be nullptr (as every output)
    double *along;             // [K][n]
    uint4 *id;                 // [K][n]: kind, prim, instance, material
    uint32_t *count;           // [n]
    double *inside;            // [n]
    const uint32_t *tri_base;  // per accel: its mesh's first triangle in the triangle tables (k_query.hip)
    const uint32_t *perm;      // PERM forms only: [n], the ray walked in each slot
};

// the planes of a layer behind a ray's last one, at element e: lg_intersect's miss record, its id words, +INF
__device__ __forceinline__ void layer_store_miss(const LayersArgs &Q, unsigned long long e) {
    if (Q.hits) store_hit_none(Q.hits + 6ull * e);
    if (Q.id) Q.id[e] = hit_id_none();
    if (Q.along) Q.along[e] = INFINITY;
}

// The origin of the segment behind a hit: shade_frame's pm, from an evaluation of its own behind an optimisation barrier.  With pm live in
// the evaluation that fills the record, the compiler forms some components of ng as -(-ng) (pm = p - ng * err wants -ng): the same number,
// but where the hit's geometry is NaN (an origin at 1e300, a quadratic that overflowed) the other NaN sign -- and the record would no
// longer be lg_intersect's bit for bit.  So the record's evaluation has query_kernel's uses and no others (store_hit, tilewalk.h), and pm
// comes from this one.
__device__ __forceinline__ V3 layer_next_origin(const DParams &P, const Ray &r, const Best &b) {
    const Ray ray = ray_opaque(r);
    Shade sh;
    shade_frame(P, ray, b, sh);
    return sh.pm;
}

template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) layers_kernel(const DParams P, const LayersArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t lane = threadIdx.x & 63u;
    TileWalk<FAST, LDSS> tw;
    if (!tw.begin(P)) return;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    const uint32_t K = Q.max_layers;
    for (bool final = false; !final;) {
        const uint32_t tile = tw.next(P, final);
        if (tile == NO_TILE) break;
        unsigned long long i = (unsigned long long)tile * 64ull + lane;
        const bool active = i < Q.n;
        if (PERM && active) i = Q.perm[i];
        Ray ray = idle_ray();
        if (active) ray = load_ray(Q.rays, i);
        // ---- the layer loop: segment j of every lane still alive, while the wave has one (j is uniform)
        bool alive = active;
        double T = 0.0, inside = 0.0;
        uint32_t count = 0u, j = 0u;
        for (; j < K && wave_any(alive); ++j) {
            const unsigned long long e = (unsigned long long)j * Q.n + i;
            if (alive) {
                Best b = fresh_best();
                walk<LDSS, FAST, PRUNE>(P, ray, false, tw.stack, tw.stride, b, tw.scn, cnt, tw.arec);
                if (b.ref == NO_HIT) {
                    layer_store_miss(Q, e);
                    alive = false; // a miss: the ray is finished
                } else {
                    Shade sh;
                    shade_frame(P, ray, b, sh);
                    const uint4 id = hit_id(b, sh, Q.tri_base);
                    if (Q.hits) store_hit(Q.hits + 6ull * e, b, sh, id);
                    if (Q.id) Q.id[e] = id;
                    // T_0 = t_0, T_j = T_{j-1} + t_j: the 2^-36 steps are not added.  A NaN stays (here and in inside): which of two NaNs a
                    // sum returns is the operand order's, and that is the compiler's
                    T = j == 0u ? b.t : (T != T ? T : T + b.t);
                    if (Q.along) Q.along[e] = T;
                    if (j & 1u) inside = inside != inside ? inside : inside + b.t; // t_1 + t_3 + ..., from +0.0
                    ++count;
                    ray = ray_new(layer_next_origin(P, ray, b), ray.d); // the next segment: p - ng * 2^-36, the direction's bits kept
                }
            } else if (active) layer_store_miss(Q, e); // a ray that ended below j, in a wave that walks on
        }
        if (!active) continue;
        for (uint32_t m = j; m < K; ++m) layer_store_miss(Q, (unsigned long long)m * Q.n + i); // the layers no lane of the wave reached
        if (Q.count) Q.count[i] = count;
        if (Q.inside) Q.inside[i] = inside;
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's.  Variants: as given, permuted
template <bool F, bool L, bool Z> struct LayersKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(layers_kernel<F, L, Z, false>), reinterpret_cast<const void *>(layers_kernel<F, L, Z, true>)};
        return k[v];
    }
};
// perm != nullptr: the PERM variant; every output may be nullptr
hipError_t launch_hit_layers(const DParams &P, const double *rays, unsigned long long n, uint32_t max_layers, void *hits, double *along, void *id, uint32_t *count,
                             double *inside, const uint32_t *tri_base, const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const LayersArgs Q{rays, n, max_layers, reinterpret_cast<uint4 *>(hits), along, reinterpret_cast<uint4 *>(id), count, inside, tri_base, perm};
    void *args[] = {const_cast<DParams *>(&P), const_cast<LayersArgs *>(&Q)};
    return trav_launch<LayersKernels>(P, fast, perm ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t hit_layers_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<LayersKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t hit_layers_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<LayersKernels>(bytes, ldss); }

} // namespace lg
