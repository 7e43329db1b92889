// lasgun_amd/csrc/k_view_features.hip -- view features (include/lasgun_hip.h, lg_capture_view_features*): depth, normal, albedo, coverage,
// ids and the world-space hit point of the primary hits of K cameras over one accel, into K whole films' planes in one launch.  It is
// features_kernel (k_features.hip) with the camera a row of a table (DView; view_ray.h, as k_views.hip reads it) instead of eight fields of
// DParams, and one more accumulator triple.
//
// The prologue, the tile claim, the LDS image and the stacks are features_kernel's as they stood before tilewalk.h, in this file's own text
// (over the shared header this family's rows measured slower than the parent's by more than its spread, profiles/tilewalk_account.md); the grid is sized in query.cpp (traversal_grid) and the
// forms are launched through travform.h.  The walk is closest hit: walk<LDSS, FAST, PRUNE>(.., any = false, ..), unchanged.  A tile is
// global pixel tile G = v * tiles_per_view + t of view_pixel -- an 8 x 8 tile of film v -- and a lane is one PIXEL, looping over its samples
// s = 0 .. S-1: the wave walks sample s together, and each pixel's sums come out in sample order with no cross-lane step.  v is the same in
// every lane of a tile: the view's 16 doubles are read ONCE per tile through a wave-uniform index from the constant address space, scalar
// loads into SGPRs, and kept across the S walks -- not reloaded per sample and not held in 30 vector registers.  Ten f64 accumulators, a hit
// count and sample 0's identity stay in registers across the walks.
//
// Out: only the planes asked for, film v's pixel (x, y) at v * w * h + y * w + x.  depth and coverage are one f32 a pixel; normal, albedo
// and point are three f32 at a 12-byte pitch, written as three 4-byte stores (a 16-byte store would reach into the neighbouring pixel, or
// past the last film's end); id is one 16-byte store.  At most 60 bytes a pixel, whatever S is, each written by its own lane alone.
// Lanes beyond a film's edge walk nothing and write nothing.
#include "travform.h"
#include "view_ray.h"

namespace lg {

struct ViewFeatureArgs {
    float *depth;               // [n_views * w * h]
    float *normal;              // [n_views * w * h][3]
    float *albedo;              // [n_views * w * h][3]
    float *coverage;            // [n_views * w * h]
    uint4 *id;                  // [n_views * w * h]: kind, prim, instance, material
    float *point;               // [n_views * w * h][3]
    const double *material_rgb; // [nmat][3], read only where albedo is asked for
    uint32_t nmat;
    const uint32_t *tri_base;   // per accel: its mesh's first triangle in the triangle tables (k_query.hip)
};

template <bool FAST, bool LDSS, bool PRUNE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) view_features_kernel(const DParams P, const ViewArgs V, const ViewFeatureArgs Q) {
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
    const uint32_t S = P.ss_root * P.ss_root;
    uint32_t band = LDSS ? xcc_id() : 0u, bands_left = TILE_HEADS;
    for (bool final = false; !final;) {
        uint32_t tile;
        if (LDSS) tile = claim_tile(P.tile_counter, ntiles, band, bands_left, final);
        else tile = claim_tile_single(P.tile_counter, ntiles, final);
        if (tile == NO_TILE) break;
        // (the claimed tile is the same in every lane, and so is the view made from it and the kernel's arguments: said once more for the compiler)
        const uint32_t G = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile);
        const ViewPixel px = view_pixel(V, G, lane);
        const DView view = view_load(V, px.v); // G < n_views * tiles_per_view: a row of the table, whatever the lane's pixel is
        double tsum = 0.0;
        V3 nsum{0.0, 0.0, 0.0}, asum{0.0, 0.0, 0.0}, psum{0.0, 0.0, 0.0};
        uint32_t nhit = 0u;
        uint4 id0 = make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu); // kind 0, prim / instance ~0, material -1: lg_hit's miss
        for (uint32_t s = 0u; s < S; ++s) {
            Ray ray = ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0});
            if (px.active) ray = view_ray(P, view, px.x, px.y, s);
            Best b;
            b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
            if (px.active) walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
            if (!px.active || b.ref == NO_HIT) continue;
            Shade sh;
            shade_frame(P, ray, b, sh);
            nhit += 1u;
            tsum = tsum + b.t;
            nsum = nsum + sh.ns;
            psum = psum + sh.praw; // lg_hit::p (k_query.hip)
            if (Q.albedo && (uint32_t)sh.mat < Q.nmat) { // (an index outside the table, a negative one included, adds nothing)
                const double *c = Q.material_rgb + 3ull * (uint32_t)sh.mat;
                asum = asum + V3{c[0], c[1], c[2]};
            }
            if (s == 0u) {
                const uint32_t pk = b.ref >> 30, idx = b.ref & PRIM_INDEX_MASK;
                id0 = make_uint4(pk + 1u, pk == PK_TRIANGLE ? idx - Q.tri_base[b.accel] : idx, b.accel, (uint32_t)sh.mat);
            }
        }
        if (!px.active) continue;
        const double inv = 1.0 / (double)S, inv_hit = 1.0 / (double)nhit; // (inv_hit is read only where nhit != 0)
        const unsigned long long pix = px.pix;
        if (Q.depth) Q.depth[pix] = nhit ? (float)(tsum * inv_hit) : INFINITY;
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
        if (Q.point) {
            float *o = Q.point + 3ull * pix;
            o[0] = nhit ? (float)(psum.x * inv_hit) : 0.0f; o[1] = nhit ? (float)(psum.y * inv_hit) : 0.0f; o[2] = nhit ? (float)(psum.z * inv_hit) : 0.0f;
        }
    }
}

// ---- host-callable launchers (query.cpp): the forms and their three operations are travform.h's
template <bool F, bool L, bool Z> struct ViewFeatureKernels {
    static constexpr int variants = 1;
    static const void *kernel(int) { return reinterpret_cast<const void *>(view_features_kernel<F, L, Z>); }
};
hipError_t launch_view_features(const DParams &P, const ViewArgs &V, float *depth, float *normal, float *albedo, float *coverage, void *id, float *point,
                                const double *material_rgb, uint32_t nmat, const uint32_t *tri_base, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    const ViewFeatureArgs Q{depth, normal, albedo, coverage, reinterpret_cast<uint4 *>(id), point, material_rgb, nmat, tri_base};
    void *args[] = {const_cast<DParams *>(&P), const_cast<ViewArgs *>(&V), const_cast<ViewFeatureArgs *>(&Q)};
    return trav_launch<ViewFeatureKernels>(P, fast, 0, blocks, stack_depth, args, stream);
}
hipError_t view_features_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) {
    return trav_occupancy<ViewFeatureKernels>(P, fast, stack_depth, blocks_per_cu);
}
hipError_t view_features_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<ViewFeatureKernels>(bytes, ldss); }

} // namespace lg
