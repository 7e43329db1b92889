// lasgun_amd/csrc/k_directions.hip -- direction sets (include/lasgun_hip.h, lg_open_directions*): which of K shared directions are open above
// each of N points.  Pair (i, k) is the ray (points[i], dirs[k]), both as given: no arithmetic makes it, and nothing is written out as rays.
//
// The kernel's prologue and tile cursor are tilewalk.h's; the grid is sized in query.cpp (traversal_grid) and the forms are
// launched through travform.h.  The walk is any-hit: walk<LDSS, FAST, PRUNE>(.., any = true, ..), unchanged.  What differs is the work
// item, and it is not k_visibility.hip's 8 x 8 block: a tile is 64 consecutive POINTS x 8 consecutive DIRECTIONS, one byte of each of 64
// rows.  tile = point_block * dir_bytes + dir_byte: consecutive tiles keep their points and step through the directions.  Lane l owns
// point 64 pb + l, reads it and its normal once, then loops j = 0 .. 7 over the directions 8 db + j -- the same address in every lane
// -- so in every trip the wave walks PARALLEL rays from 64 neighbouring points, the shape of a shadow pass under a
// directional light.  A lane whose direction is not above its horizon (s = (n.x d.x + n.y d.y) + n.z d.z, s > 0.0; every pair when there
// are no normals) sits the trip out: the pair is not walked.
//
// Out: the lane's own byte at bits[point * row_bytes + db] -- every used byte written exactly once, padding bits 0 because the trips with
// k >= n_dirs set nothing; no ballot, no atomics -- and two integer atomicAdds a lane and tile into count buffers zeroed on the same stream
// ahead of the launch (query.cpp): the byte's popcount to open[point], the trips it was above in to above[point]; a zero is skipped.  A
// wave's adds are 64 consecutive words; integer sums do not depend on the order the tiles finish in.  Lanes behind n_points walk nothing
// and store nothing.
#include "travform.h"
#include "tilewalk.h"

namespace lg {

struct DirectionArgs {
    const double *points;          // [n_points][3]
    const double *normals;         // [n_points][3], nullptr: every pair is above
    const double *dirs;            // [n_dirs][3]
    unsigned long long n_points, n_dirs;
    uint8_t *bits;                 // [n_points][row_bytes], may be nullptr
    unsigned long long row_bytes;
    uint32_t *open;                // [n_points], zeroed before the launch; may be nullptr
    uint32_t *above;               // [n_points], zeroed before the launch; may be nullptr
    uint32_t dir_bytes;            // ceil(n_dirs / 8): tiles per block of 64 points (ntiles = ceil(n_points / 64) * dir_bytes, DParams)
};

template <bool FAST, bool LDSS, bool PRUNE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) directions_kernel(const DParams P, const DirectionArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t lane = threadIdx.x & 63u;
    TileWalk<FAST, LDSS> tw;
    if (!tw.begin(P)) return;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    for (bool final = false; !final;) {
        const uint32_t tile = tw.next(P, final);
        if (tile == NO_TILE) break;
        const uint32_t pb = tile / Q.dir_bytes, db = tile - pb * Q.dir_bytes;
        const unsigned long long point = 64ull * pb + lane;
        const bool active = point < Q.n_points;
        V3 o{0.0, 0.0, 0.0}, n{0.0, 0.0, 0.0};
        if (active) {
            const double *p = Q.points + 3ull * point;
            o = V3{p[0], p[1], p[2]};
            if (Q.normals) {
                const double *q = Q.normals + 3ull * point;
                n = V3{q[0], q[1], q[2]};
            }
        }
        uint32_t byte = 0u, nabove = 0u;
        for (uint32_t j = 0u; j < 8u; ++j) {
            const unsigned long long k = 8ull * db + j;
            if (k >= Q.n_dirs) break; // (uniform)
            const double *dk = Q.dirs + 3ull * k; // the same address in every lane
            const V3 d{dk[0], dk[1], dk[2]};
            bool up = active;
            if (Q.normals) up = active && (n.x * d.x + n.y * d.y) + n.z * d.z > 0.0; // (a NaN sum, a zero and a perpendicular direction: not above)
            Best b = fresh_best();
            if (up) {
                const Ray ray = ray_new(o, d); // origin and direction as given
                walk<LDSS, FAST, PRUNE>(P, ray, true, tw.stack, tw.stride, b, tw.scn, cnt, tw.arec);
                nabove += 1u;
                if (!(b.t < 1.0)) byte |= 1u << j; // open: lg_occluded's test (point.rs:49) answers 0
            }
        }
        if (!active) continue;
        if (Q.bits) Q.bits[point * Q.row_bytes + db] = (uint8_t)byte;
        if (Q.open && byte) atomicAdd(Q.open + point, (uint32_t)__builtin_popcount(byte));
        if (Q.above && nabove) atomicAdd(Q.above + point, nabove);
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's
template <bool F, bool L, bool Z> struct DirectionKernels {
    static constexpr int variants = 1;
    static const void *kernel(int) { return reinterpret_cast<const void *>(directions_kernel<F, L, Z>); }
};
hipError_t launch_open_directions(const DParams &P, const double *points, const double *normals, unsigned long long n_points, const double *dirs,
                                  unsigned long long n_dirs, uint8_t *bits, unsigned long long row_bytes, uint32_t *open, uint32_t *above, bool fast,
                                  uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const DirectionArgs Q{points, normals, dirs, n_points, n_dirs, bits, row_bytes, open, above, (uint32_t)((n_dirs + 7ull) / 8ull)};
    void *args[] = {const_cast<DParams *>(&P), const_cast<DirectionArgs *>(&Q)};
    return trav_launch<DirectionKernels>(P, fast, 0, blocks, stack_depth, args, stream);
}
hipError_t open_directions_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<DirectionKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t open_directions_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<DirectionKernels>(bytes, ldss); }

} // namespace lg
