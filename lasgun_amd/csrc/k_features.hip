// lasgun_amd/csrc/k_features.hip -- feature buffers (include/lasgun_hip.h, lg_capture_features*): depth, normal, albedo, coverage and ids of
// the primary hits of the scene's own camera, the rays made in registers as the render makes them (camera_ray) and never written anywhere.
//
// The kernel's prologue, tile cursor and id word are tilewalk.h's; the grid is sized in query.cpp (traversal_grid) and the forms are
// launched through travform.h.  The walk is closest hit: walk<LDSS, FAST, PRUNE>(.., any = false, ..), unchanged.  What differs is the work
// item: a tile is an 8 x 8 block of the rectangle (pixel_of, mode 0, as the render's tiles) and a lane is one PIXEL.  The lane loops over
// the pixel's samples s = 0 .. S-1, so the whole wave walks sample s together (64 neighbouring rays, as a render's wave) and each pixel's
// sums come out in sample order with no cross-lane step: seven f64 accumulators, a hit count and sample 0's identity stay in registers
// across the walks.
//
// Out: only the planes asked for.  depth and coverage are one f32 a pixel (a tile row is 32 contiguous bytes); normal and albedo are
// three f32 at a 12-byte pitch, written as three 4-byte stores -- a 16-byte store would reach into the neighbouring pixel, which may lie
// outside the rectangle and is never touched (a tile row's 8 lanes still cover 96 contiguous bytes); id is one 16-byte store.  At most
// 48 bytes a pixel, whatever S is.  Lanes outside the rectangle walk nothing and write nothing.
#include "travform.h"
#include "tilewalk.h"

namespace lg {

struct FeatureArgs {
    float *depth;               // [pixels]
    float *normal;              // [pixels][3]
    float *albedo;              // [pixels][3]
    float *coverage;            // [pixels]
    uint4 *id;                  // [pixels]: kind, prim, instance, material
    const double *material_rgb; // [nmat][3], read only where albedo is asked for
    uint32_t nmat;
    const uint32_t *tri_base;   // per accel: its mesh's first triangle in the triangle tables (k_query.hip)
};

template <bool FAST, bool LDSS, bool PRUNE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) features_kernel(const DParams P, const FeatureArgs Q) {
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t lane = threadIdx.x & 63u;
    TileWalk<FAST, LDSS> tw;
    if (!tw.begin(P)) return;
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    const uint32_t S = P.ss_root * P.ss_root;
    for (bool final = false; !final;) {
        const uint32_t tile = tw.next(P, final);
        if (tile == NO_TILE) break;
        const Pixel px = pixel_of(P, tile, lane);
        double tsum = 0.0;
        V3 nsum{0.0, 0.0, 0.0}, asum{0.0, 0.0, 0.0};
        uint32_t nhit = 0u;
        uint4 id0 = hit_id_none(); // lg_hit's miss
        for (uint32_t s = 0u; s < S; ++s) {
            Ray ray = idle_ray();
            if (px.active) ray = camera_ray(P, px.x, px.y, s);
            Best b = fresh_best();
            if (px.active) walk<LDSS, FAST, PRUNE>(P, ray, false, tw.stack, tw.stride, b, tw.scn, cnt, tw.arec);
            if (!px.active || b.ref == NO_HIT) continue;
            Shade sh;
            shade_frame(P, ray, b, sh);
            nhit += 1u;
            tsum = tsum + b.t;
            nsum = nsum + sh.ns;
            if (Q.albedo && (uint32_t)sh.mat < Q.nmat) { // (an index outside the table, a negative one included, adds nothing)
                const double *c = Q.material_rgb + 3ull * (uint32_t)sh.mat;
                asum = asum + V3{c[0], c[1], c[2]};
            }
            if (s == 0u) id0 = hit_id(b, sh, Q.tri_base);
        }
        if (!px.active) continue;
        const double inv = 1.0 / (double)S;
        const unsigned long long pix = px.pix;
        if (Q.depth) Q.depth[pix] = nhit ? (float)(tsum * (1.0 / (double)nhit)) : INFINITY;
        if (Q.normal) {
            float *o = Q.normal + 3ull * pix;
            o[0] = (float)(nsum.x * inv); o[1] = (float)(nsum.y * inv); o[2] = (float)(nsum.z * inv);
        }
        if (Q.albedo) {
            float *o = Q.albedo + 3ull * pix;
            o[0] = (float)(asum.x * inv); o[1] = (float)(asum.y * inv); o[2] = (float)(asum.z * inv);
        }
        if (Q.coverage) Q.coverage[pix] = (float)((double)nhit * inv);
        if (Q.id) Q.id[pix] = id0;
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's
template <bool F, bool L, bool Z> struct FeatureKernels {
    static constexpr int variants = 1;
    static const void *kernel(int) { return reinterpret_cast<const void *>(features_kernel<F, L, Z>); }
};
hipError_t launch_features(const DParams &P, float *depth, float *normal, float *albedo, float *coverage, void *id, const double *material_rgb, uint32_t nmat,
                           const uint32_t *tri_base, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const FeatureArgs Q{depth, normal, albedo, coverage, reinterpret_cast<uint4 *>(id), material_rgb, nmat, tri_base};
    void *args[] = {const_cast<DParams *>(&P), const_cast<FeatureArgs *>(&Q)};
    return trav_launch<FeatureKernels>(P, fast, 0, blocks, stack_depth, args, stream);
}
hipError_t features_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) { return trav_occupancy<FeatureKernels>(P, fast, stack_depth, blocks_per_cu); }
hipError_t features_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<FeatureKernels>(bytes, ldss); }

} // namespace lg
