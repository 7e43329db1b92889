// lasgun_amd/csrc/k_scan.hip -- range scans (include/lasgun_hip.h, lg_range_scan*): the first hits along K shared beams from N sensor poses.
// Ray (i, k) has the origin origins[i] as given and the direction beams[k] as given, or, with frames, the pose's 3 x 3 matrix applied to
// the beam -- d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z, f64, in this order, nothing fused (-ffp-contract=off) -- and is never
// written out as a ray; what comes back is not lg_hit records but only the planes asked for.
//
// The kernel's prologue and tile loop are those of tilewalk.h, which the tiled kernels of the query family share, in this file's own text:
// over the shared header rows of this family measured slower than the parent's by more than its spread (profiles/tilewalk_account.md).
// The grid is sized in query.cpp (traversal_grid) and the forms are launched through travform.h.  The walk is closest hit: walk<LDSS, FAST, PRUNE>(.., any = false, ..), unchanged, and the hit is resolved
// as query_kernel resolves it (shade_frame, the face number through tri_base) -- but only where point, normal or id is asked for: range,
// hits and nearest need b.t and b.ref alone.  What differs is the work item, and there are two (POSE):
//   beam lanes (POSE = false): a tile is one POSE x 64 consecutive BEAMS, tile = pose * beam_tiles + beam_block.  The origin and the frame
//     are the same address in every lane; lane l owns beam 64 bb + l.  The rays of a wave share an origin, like a camera's.
//   pose lanes (POSE = true): a tile is 64 consecutive POSES x 8 consecutive BEAMS, tile = pose_block * beam_tiles + beam_block -- the
//     direction sets' work item (k_directions.hip).  Lane l owns pose 64 pb + l, reads its origin and frame once, then loops j = 0 .. 7
//     over the beams 8 bb + j, the same address in every lane: without frames every trip walks 64 parallel rays.
//
// Out, element (i, k) at i * n_beams + k: range one f32; point and normal three f32 at a 12-byte pitch, written as three 4-byte stores (a
// 16-byte store would reach into the neighbouring element); id one 16-byte store.  The reductions go into buffers pre-filled on the same
// stream ahead of the launch (query.cpp: hits with 0, nearest with +INF's pattern 0x7F800000): an integer atomicAdd of the number of hits
// and an integer atomicMin of the smallest f32 range read as uint32 -- patterns at or above +INF's (an overflowed range, a NaN, anything
// negative) never win.  Beam lanes reduce across the wave first and issue one atomic each per tile, by lane 0; pose lanes issue one each
// per lane and tile; an atomic with nothing to add is skipped.  Integer sums and minima do not depend on the order the tiles finish in.
// Lanes behind n_poses or n_beams walk nothing and store nothing.
#include "travform.h"

namespace lg {

struct ScanArgs {
    const double *origins;         // [n_poses][3]
    const double *frames;          // [n_poses][9], row-major 3 x 3; nullptr: the beams are the directions
    const double *beams;           // [n_beams][3]
    unsigned long long n_poses, n_beams;
    float *range;                  // [n_poses * n_beams], may be nullptr (as every output)
    float *point;                  // [n_poses * n_beams][3]
    float *normal;                 // [n_poses * n_beams][3]
    uint4 *id;                     // [n_poses * n_beams]: kind, prim, instance, material
    uint32_t *hits;                // [n_poses], zeroed before the launch
    uint32_t *nearest;             // [n_poses], filled with 0x7F800000 before the launch
    const uint32_t *tri_base;      // per accel: its mesh's first triangle in the triangle tables (k_query.hip)
    uint32_t beam_tiles;           // tiles per pose (ceil(n_beams / 64)) or per block of 64 poses (ceil(n_beams / 8))
};

constexpr uint32_t SCAN_INF_BITS = 0x7F800000u; // +INF as f32: the pre-fill of nearest, and the least pattern that cannot win

// the direction of ray (pose, beam): the beam's bits, or the frame applied in the header's order
__device__ __forceinline__ V3 scan_direction(const double *M, const V3 &b) {
    if (!M) return b;
    return V3{(M[0] * b.x + M[1] * b.y) + M[2] * b.z, (M[3] * b.x + M[4] * b.y) + M[5] * b.z, (M[6] * b.x + M[7] * b.y) + M[8] * b.z};
}

// one walked pair's planes at element e; returns the f32 range's pattern if the pair is a hit, SCAN_INF_BITS otherwise
__device__ __forceinline__ uint32_t scan_store(const DParams &P, const ScanArgs &Q, const Ray &ray, const Best &b, unsigned long long e) {
    const bool hit = b.ref != NO_HIT;
    const float r = hit ? (float)b.t : INFINITY;
    if (Q.range) Q.range[e] = r;
    if (Q.point || Q.normal || Q.id) { // (uniform)
        float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
        uint4 id = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu); // kind 0, prim / instance ~0, material -1: lg_hit's miss
        if (hit) {
            Shade sh;
            shade_frame(P, ray, b, sh);
            const uint32_t pk = b.ref >> 30, idx = b.ref & PRIM_INDEX_MASK;
            p[0] = (float)sh.praw.x; p[1] = (float)sh.praw.y; p[2] = (float)sh.praw.z;
            n[0] = (float)sh.ng.x; n[1] = (float)sh.ng.y; n[2] = (float)sh.ng.z;
            id = make_uint4(pk + 1u, pk == PK_TRIANGLE ? idx - Q.tri_base[b.accel] : idx, b.accel, (uint32_t)sh.mat);
        }
        if (Q.point) { float *o = Q.point + 3ull * e; o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
        if (Q.normal) { float *o = Q.normal + 3ull * e; o[0] = n[0]; o[1] = n[1]; o[2] = n[2]; }
        if (Q.id) Q.id[e] = id;
    }
    return hit ? __float_as_uint(r) : SCAN_INF_BITS;
}

template <bool FAST, bool LDSS, bool PRUNE, bool POSE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) scan_kernel(const DParams P, const ScanArgs Q) {
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
        const uint32_t hi = tile / Q.beam_tiles, bb = tile - hi * Q.beam_tiles;
        if (!POSE) {
            // ---- beam lanes: pose `hi`, beam 64 bb + lane
            const unsigned long long pose = hi, k = 64ull * bb + lane;
            const bool active = k < Q.n_beams;
            const double *po = Q.origins + 3ull * pose; // the same address in every lane
            Ray ray = ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0});
            Best b;
            b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
            uint32_t bits = SCAN_INF_BITS;
            if (active) {
                const double *bk = Q.beams + 3ull * k;
                ray = ray_new(V3{po[0], po[1], po[2]}, scan_direction(Q.frames ? Q.frames + 9ull * pose : nullptr, V3{bk[0], bk[1], bk[2]}));
                walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
                bits = scan_store(P, Q, ray, b, pose * Q.n_beams + k);
            }
            if (Q.hits || Q.nearest) { // (uniform; every lane of the wave is here)
                const uint32_t nhit = (uint32_t)__popcll(__ballot(active && b.ref != NO_HIT));
                for (int off = 32; off > 0; off >>= 1) bits = min(bits, (uint32_t)__shfl_xor((int)bits, off));
                if (lane == 0u) {
                    if (Q.hits && nhit) atomicAdd(Q.hits + pose, nhit);
                    if (Q.nearest && bits < SCAN_INF_BITS) atomicMin(Q.nearest + pose, bits);
                }
            }
        } else {
            // ---- pose lanes: pose 64 hi + lane, beams 8 bb .. 8 bb + 7
            const unsigned long long pose = 64ull * hi + lane;
            const bool active = pose < Q.n_poses;
            V3 o{0.0, 0.0, 0.0};
            double M[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
            if (active) {
                const double *po = Q.origins + 3ull * pose;
                o = V3{po[0], po[1], po[2]};
                if (Q.frames) {
                    const double *pm = Q.frames + 9ull * pose;
                    for (int c = 0; c < 9; ++c) M[c] = pm[c];
                }
            }
            uint32_t nhit = 0u, bits = SCAN_INF_BITS;
            for (uint32_t j = 0u; j < 8u; ++j) {
                const unsigned long long k = 8ull * bb + j;
                if (k >= Q.n_beams) break; // (uniform)
                if (!active) continue;
                const double *bk = Q.beams + 3ull * k; // the same address in every lane
                const Ray ray = ray_new(o, scan_direction(Q.frames ? M : nullptr, V3{bk[0], bk[1], bk[2]}));
                Best b;
                b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
                walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
                bits = min(bits, scan_store(P, Q, ray, b, pose * Q.n_beams + k));
                nhit += b.ref != NO_HIT ? 1u : 0u;
            }
            if (!active) continue;
            if (Q.hits && nhit) atomicAdd(Q.hits + pose, nhit);
            if (Q.nearest && bits < SCAN_INF_BITS) atomicMin(Q.nearest + pose, bits);
        }
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's.  Variants: beam lanes, pose lanes
template <bool F, bool L, bool Z> struct ScanKernels {
    static constexpr int variants = 2;
    static const void *kernel(int v) {
        const void *k[variants] = {reinterpret_cast<const void *>(scan_kernel<F, L, Z, false>), reinterpret_cast<const void *>(scan_kernel<F, L, Z, true>)};
        return k[v];
    }
};
hipError_t launch_range_scan(const DParams &P, const double *origins, const double *frames, unsigned long long n_poses, const double *beams,
                             unsigned long long n_beams, bool pose_lanes, float *range, float *point, float *normal, void *id, uint32_t *hits, uint32_t *nearest,
                             const uint32_t *tri_base, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const unsigned long long per = pose_lanes ? 8ull : 64ull;
    const ScanArgs Q{origins, frames, beams, n_poses, n_beams, range, point, normal, reinterpret_cast<uint4 *>(id), hits, nearest, tri_base,
                     (uint32_t)((n_beams + per - 1ull) / per)};
    void *args[] = {const_cast<DParams *>(&P), const_cast<ScanArgs *>(&Q)};
    return trav_launch<ScanKernels>(P, fast, pose_lanes ? 1 : 0, blocks, stack_depth, args, stream);
}
hipError_t range_scan_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<ScanKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t range_scan_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<ScanKernels>(bytes, ldss); }

} // namespace lg
