// lasgun_amd/csrc/k_visibility.hip -- visibility matrices (include/lasgun_hip.h, lg_visibility*): occlusion between two point sets, the
// segments made in registers as the render's shadow pass makes its own (k_wavefront.hip: hit point and light position), the answer bit-packed.
//
// The kernel's prologue and tile cursor are tilewalk.h's; the grid is sized in query.cpp (traversal_grid) and the forms are
// launched through travform.h.  The walk is any-hit: walk<LDSS, FAST, PRUNE>(.., any = true, ..), unchanged.  What differs is the work
// item: an 8 x 8 BLOCK of the matrix.  Lane l of the wave that claimed block (ti, tj) walks the segment from[8 ti + (l >> 3)] ->
// to[8 tj + (l & 7)]: a wave reads 8 + 8 points (384 bytes) where lg_occluded reads 64 rays (3 KiB), and its 64 segments share 8 origins
// and 8 targets.  Blocks are numbered row-major (tile = ti * tiles_j + tj): consecutive tiles keep their origins and step through the
// targets.  Lanes outside the matrix walk nothing and vote 0.
//
// One ballot of the verdict per wave; in each of the block's 8 rows the lane with (l & 7) == 0 takes its row's byte out of the mask and
// stores it at bits[row * row_bytes + tj] -- every used byte is written exactly once, padding bits 0 (the lanes behind n_to voted 0), no
// atomics and no pre-clear -- and adds the byte's popcount to blocked[row] (zeroed on the same stream ahead of the launch, query.cpp;
// integer addition: the counts do not depend on the order the blocks finish in).
#include "travform.h"
#include "tilewalk.h"

namespace lg {

struct VisibilityArgs {
    const double *from;            // [n_from][3]
    const double *to;              // [n_to][3]
    unsigned long long n_from, n_to;
    uint8_t *bits;                 // [n_from][row_bytes], may be nullptr
    unsigned long long row_bytes;
    uint32_t *blocked;             // [n_from], zeroed before the launch; may be nullptr
    uint32_t tiles_j;              // ceil(n_to / 8): blocks per row of blocks (ntiles = ceil(n_from / 8) * tiles_j, DParams)
};

template <bool FAST, bool LDSS, bool PRUNE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) visibility_kernel(const DParams P, const VisibilityArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t lane = threadIdx.x & 63u;
    TileWalk<FAST, LDSS> tw;
    if (!tw.begin(P)) return;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    for (bool final = false; !final;) {
        const uint32_t tile = tw.next(P, final);
        if (tile == NO_TILE) break;
        const uint32_t ti = tile / Q.tiles_j, tj = tile - ti * Q.tiles_j;
        const unsigned long long row = 8ull * ti + (lane >> 3), col = 8ull * tj + (lane & 7u);
        const bool active = row < Q.n_from && col < Q.n_to;
        Best b = fresh_best();
        if (active) {
            const double *f = Q.from + 3ull * row, *t = Q.to + 3ull * col;
            const V3 o{f[0], f[1], f[2]};
            const Ray ray = ray_new(o, V3{t[0] - o.x, t[1] - o.y, t[2] - o.z}); // the segment from -> to: three subtractions, direction as it comes out
            walk<LDSS, FAST, PRUNE>(P, ray, true, tw.stack, tw.stride, b, tw.scn, cnt, tw.arec);
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(active && b.t < 1.0); // point.rs:49
        if ((lane & 7u) != 0u || row >= Q.n_from) continue;
        const uint32_t byte = (uint32_t)(mask >> (lane & 56u)) & 0xFFu;
        if (Q.bits) Q.bits[row * Q.row_bytes + tj] = (uint8_t)byte;
        if (Q.blocked && byte) atomicAdd(Q.blocked + row, (uint32_t)__builtin_popcount(byte));
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's
template <bool F, bool L, bool Z> struct VisibilityKernels {
    static constexpr int variants = 1;
    static const void *kernel(int) { return reinterpret_cast<const void *>(visibility_kernel<F, L, Z>); }
};
hipError_t launch_visibility(const DParams &P, const double *from, unsigned long long n_from, const double *to, unsigned long long n_to, uint8_t *bits,
                             unsigned long long row_bytes, uint32_t *blocked, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const VisibilityArgs Q{from, to, n_from, n_to, bits, row_bytes, blocked, (uint32_t)((n_to + 7ull) / 8ull)};
    void *args[] = {const_cast<DParams *>(&P), const_cast<VisibilityArgs *>(&Q)};
    return trav_launch<VisibilityKernels>(P, fast, 0, blocks, stack_depth, args, stream);
}
hipError_t visibility_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<VisibilityKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t visibility_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<VisibilityKernels>(bytes, ldss); }

} // namespace lg
