// lasgun_amd/csrc/k_paths.hip -- ray paths (include/lasgun_hip.h, lg_trace_paths*): each of the caller's rays followed through up to
// max_bounces vertices in one launch.  Vertex j of ray i is what lg_intersect returns for segment j; segment 0 is the ray as given; at a
// vertex the rule of the hit's material (the caller's table, read per lane) ends the path or forms segment j+1 -- mirrored, straight on or
// refracted, bounce.h's arithmetic.  The ray stays in registers between the walks; only the planes asked for are written.
//
// The kernel is layers_kernel's shape (k_layers.hip) with a direction update: tilewalk.h's prologue, tile cursor and record writer, and the
// same wave-uniform loop over the unchanged walk<LDSS, FAST, PRUNE>(.., any = false, ..) with a fresh Best per segment; the grid sized in
// query.cpp (traversal_grid), the forms launched through travform.h, PERM as there.  A hit is resolved as query_kernel resolves it (shade_frame, the face number through
// tri_base); what the next ray needs (p, ng, ns) comes from a second evaluation behind an optimisation barrier (path_vertex says why).
// What lives across the walks besides the ray: T (the running parameter), gain, count, medium and end -- 7 VGPRs; nothing is parked in
// memory.  Lanes are not re-packed when paths end: a wave walks while any of its lanes is alive, a lane whose path has ended writes the
// miss values of the vertices its wave still walks, and the vertices no lane of the wave reached are filled after the loop.  A path's ray is
// not touched once it has ended, and a path alive after the loop was cut: either way `last` is the ray in the registers.
//
// Out, vertex-major: element (j, i) at j * n + i.  hits: the 96-byte lg_hit as six 16-byte stores; id: its last 16 bytes as one store;
// point: three 8-byte stores; along: one; count, end, gain, last and medium: once per ray, after the loop.  Every element of every plane
// asked for is written by exactly one lane: no atomics, no pre-fill.  Lanes past the last ray (n % 64) walk nothing and write nothing.
#include "travform.h"
#include "tilewalk.h"
#include "bounce.h"

namespace lg {

struct PathRule { // lg_path_rule
    uint32_t action, reserved;
    double ior, gain;
};
static_assert(sizeof(PathRule) == 24, "lg_path_rule: 24 bytes");

constexpr uint32_t PATH_END_CUT = 0u, PATH_END_ESCAPED = 1u, PATH_END_ABSORBED = 2u, PATH_END_DEGENERATE = 3u; // LG_PATH_END_*

struct PathsArgs {
    const double *rays;           // [n][6]: origin xyz, direction xyz, as for lg_intersect
    unsigned long long n;
    uint32_t max_bounces;         // K >= 1
    uint32_t n_rules;             // the table's entries: a material outside 0 .. n_rules-1 absorbs
    const PathRule *rules;        // [n_rules], device memory (staged by query.cpp)
    uint32_t use_ns;              // 0: N = lg_hit::ng; 1: N = lg_hit::ns
    const uint32_t *start_medium; // [n], bit 0; nullptr: every ray starts outside
    uint4 *hits;                  // [K][n] lg_hit, 6 x uint4 each; may be nullptr (as every output)
    double *point;                // [K][n][3]
    uint4 *id;                    // [K][n]: kind, prim, instance, material
    double *along;                // [K][n]
    uint32_t *count, *end;        // [n]
    double *gain;                 // [n]
    double *last;                 // [n][6]
    uint32_t *medium;             // [n]
    const uint32_t *tri_base;     // per accel: its mesh's first triangle in the triangle tables (k_query.hip)
    const uint32_t *perm;         // PERM forms only: [n], the ray walked in each slot
};

// the planes of a vertex behind a path's last one, at element e: lg_intersect's miss record, its id words, +0s, +INF
__device__ __forceinline__ void path_store_miss(const PathsArgs &Q, unsigned long long e) {
    if (Q.hits) store_hit_none(Q.hits + 6ull * e);
    if (Q.point) { double *pt = Q.point + 3ull * e; pt[0] = 0.0; pt[1] = 0.0; pt[2] = 0.0; }
    if (Q.id) Q.id[e] = hit_id_none();
    if (Q.along) Q.along[e] = INFINITY;
}

// What the next ray is formed from -- the segment's direction and the vertex's p, ng and ns --, from an evaluation of shade_frame of its
// own behind an optimisation barrier.  With these live in the evaluation that fills the record, the compiler is free to form components of
// ng or ns as -(-x) (the bounce wants -N and p - ng * 2^-36): the same number, but where the hit's geometry is NaN the other NaN sign --
// and the record would no longer be lg_intersect's bit for bit (k_layers.hip, layer_next_origin, met this).  So the record's evaluation
// has query_kernel's uses and no others, and the bounce reads this one.
struct PathVertex {
    V3 d, p, ng, ns;
};
__device__ __forceinline__ PathVertex path_vertex(const DParams &P, const Ray &r, const Best &b) {
    const Ray ray = ray_opaque(r);
    Shade sh;
    shade_frame(P, ray, b, sh);
    return PathVertex{ray.d, sh.praw, sh.ng, sh.ns};
}

template <bool FAST, bool LDSS, bool PRUNE, bool PERM>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) paths_kernel(const DParams P, const PathsArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t lane = threadIdx.x & 63u;
    TileWalk<FAST, LDSS> tw;
    if (!tw.begin(P)) return;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    const uint32_t K = Q.max_bounces;
    for (bool final = false; !final;) {
        const uint32_t tile = tw.next(P, final);
        if (tile == NO_TILE) break;
        unsigned long long i = (unsigned long long)tile * 64ull + lane;
        const bool active = i < Q.n;
        if (PERM && active) i = Q.perm[i];
        Ray ray = idle_ray();
        uint32_t medium = 0u;
        if (active) {
            ray = load_ray(Q.rays, i);
            if (Q.start_medium) medium = Q.start_medium[i] & 1u;
        }
        // ---- the bounce loop: segment j of every lane still alive, while the wave has one (j is uniform)
        bool alive = active;
        double T = 0.0, gain = 1.0;
        uint32_t count = 0u, end = PATH_END_CUT, j = 0u;
        for (; j < K && wave_any(alive); ++j) {
            const unsigned long long e = (unsigned long long)j * Q.n + i;
            if (alive) {
                Best b = fresh_best();
                walk<LDSS, FAST, PRUNE>(P, ray, false, tw.stack, tw.stride, b, tw.scn, cnt, tw.arec);
                if (b.ref == NO_HIT) {
                    path_store_miss(Q, e);
                    end = PATH_END_ESCAPED; // a segment missed: the ray in the registers is that segment
                    alive = false;
                } else {
                    Shade sh;
                    shade_frame(P, ray, b, sh);
                    const uint4 id = hit_id(b, sh, Q.tri_base);
                    if (Q.hits) store_hit(Q.hits + 6ull * e, b, sh, id);
                    if (Q.id) Q.id[e] = id;
                    if (Q.point) { double *pt = Q.point + 3ull * e; pt[0] = sh.praw.x; pt[1] = sh.praw.y; pt[2] = sh.praw.z; } // (the record's own p)
                    // T_0 = t_0, T_j = T_{j-1} + t_j: the 2^-36 steps are not added.  A NaN stays (here and in gain): which of two NaNs an
                    // operation returns is the operand order's, and that is the compiler's
                    T = j == 0u ? b.t : (T != T ? T : T + b.t);
                    if (Q.along) Q.along[e] = T;
                    ++count;
                    const PathVertex v = path_vertex(P, ray, b);
                    uint32_t action = PATH_ABSORB; // a material outside the table absorbs
                    double ior = 1.0, rgain = 1.0;
                    if ((uint32_t)sh.mat < Q.n_rules) {
                        const PathRule *r = Q.rules + (uint32_t)sh.mat;
                        action = r->action; ior = r->ior; rgain = r->gain;
                    }
                    if (action == PATH_ABSORB) {
                        end = PATH_END_ABSORBED;
                        alive = false;
                    } else {
                        gain = gain != gain ? gain : gain * rgain;
                        const Bounce nb = bounce_next(action, ior, v.d, v.p, v.ng, Q.use_ns ? v.ns : v.ng, medium);
                        medium = nb.medium;
                        if (!bounce_finite(nb)) {
                            end = PATH_END_DEGENERATE; // the ray in the registers stays the segment that found this vertex
                            alive = false;
                        } else ray = ray_new(nb.o, nb.d);
                    }
                }
            } else if (active) path_store_miss(Q, e); // a path that ended below j, in a wave that walks on
        }
        if (!active) continue;
        for (uint32_t m = j; m < K; ++m) path_store_miss(Q, (unsigned long long)m * Q.n + i); // the vertices no lane of the wave reached
        if (Q.count) Q.count[i] = count;
        if (Q.end) Q.end[i] = end; // (alive here: cut after K vertices, end as initialised)
        if (Q.gain) Q.gain[i] = gain;
        if (Q.last) {
            double *l = Q.last + 6ull * i;
            l[0] = ray.o.x; l[1] = ray.o.y; l[2] = ray.o.z; l[3] = ray.d.x; l[4] = ray.d.y; l[5] = ray.d.z;
        }
        if (Q.medium) Q.medium[i] = medium;
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's.  Variants: as given, permuted
template <bool F, bool L, bool Z> struct PathsKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(paths_kernel<F, L, Z, false>), reinterpret_cast<const void *>(paths_kernel<F, L, Z, true>)};
        return k[v];
    }
};
// perm != nullptr: the PERM variant; every output may be nullptr; rules: n_rules lg_path_rule records in device memory
hipError_t launch_trace_paths(const DParams &P, const double *rays, unsigned long long n, uint32_t max_bounces, const void *rules, uint32_t n_rules, bool use_ns,
                              const uint32_t *start_medium, void *hits, double *point, void *id, double *along, uint32_t *count, uint32_t *end, double *gain, double *last,
                              uint32_t *medium, const uint32_t *tri_base, const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const PathsArgs Q{rays, n, max_bounces, n_rules, reinterpret_cast<const PathRule *>(rules), use_ns ? 1u : 0u, start_medium, reinterpret_cast<uint4 *>(hits), point,
                      reinterpret_cast<uint4 *>(id), along, count, end, gain, last, medium, tri_base, perm};
    void *args[] = {const_cast<DParams *>(&P), const_cast<PathsArgs *>(&Q)};
    return trav_launch<PathsKernels>(P, fast, perm ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t trace_paths_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<PathsKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t trace_paths_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<PathsKernels>(bytes, ldss); }

} // namespace lg
