// lasgun_amd/csrc/k_views.hip -- view batches (include/lasgun_hip.h, lg_capture_views*): one accel seen from K cameras into K films of one
// size, LEVEL 0 of the level-by-level pipeline (k_wavefront.hip) a fourth time.  k_radiance.hip is level 0 for rays the caller wrote out and
// k_gather.hip for rays made from two tables; here the rays are the render's own -- camera_ray()'s expression (shade.h, Camera::sample) --
// over a camera that is a row of a table (DView) instead of eight fields of DParams.  The three passes are level0.h's bodies over ViewSource,
// which says the three things a source says -- read it side by side with wf_trace_kernel's L0 branch:
//   * the work tile -> (view, pixel, sample) mapping (view_pixel).  Work tile vt of a chunk is pixel tile vt / ss_par of the chunk at sample
//     vt % ss_par, the render's samples side by side (shade.h, l0_tile); pixel tile t of the chunk is global pixel tile
//     G = base_tile + t = v * tiles_per_view + tile-of-film-v, an 8 x 8 tile of film v as pixel_of's mode 0 cuts it (tx = tile % tiles_x; lane l
//     is pixel (8 tx + (l & 7), 8 ty + (l >> 3))).  v is the same in every lane of the closest pass: the view's 16 doubles are read through a
//     wave-uniform index from the constant address space, scalar loads, not 30 more vector registers in kernels that sit at their register
//     budget;
//   * the ray: view_ray -- camera_ray()'s expression word for word over the view's fields, ss_distance as the host made it
//     (1.0 / (double)samples_root).  A hit's lanes in the shade pass come from any tile, so the record is read per lane there;
//   * the finish: one sample a pixel -> (0 + li) * 1.0 as one 4-byte store and / or three doubles at the pixel of film v (film_store); several
//     -> the sample's li parked at the work item's slot of the chunk's `accum`, as finish_pixel does under ss_par, and view_resolve_kernel
//     sums a pixel's samples in their order per chunk (wf_resolve_kernel's arithmetic: chunks hold whole pixel tiles x S).  Every pixel of
//     every film is written exactly once, however the chunks are cut.
// Levels >= 1 and every shadow pass are the render's own kernels.  camera_ray()'s expression is repeated in view_ray, not shared with the
// render: k_wavefront.hip is not touched.
// view_pixel, view_load and view_ray are view_ray.h's: k_view_features.hip maps the same tiles to the same pixels and makes the same rays.
#include "wflevel.h"
#include "travform.h"
#include "view_ray.h"
#include "level0.h"

namespace lg {

// The source: the item is a pixel of film v at one sample.  finish is integrate() (integrate.rs:16-20): one sample a pixel -> Color::zero() +
// li, * 1 / 1, written (film_store); several side by side -> this sample's li parked at work item j until the resolve pass (shade.h,
// finish_pixel under ss_par)
struct ViewSource {
    const ViewArgs &Q;
    struct Item { ViewPixel px; uint32_t sample; };
    __device__ __forceinline__ bool work_item(const DParams &P, unsigned long long j, Item &it) const {
        const uint32_t ptile = l0_tile(P, (uint32_t)(j >> 6), it.sample);
        it.px = view_pixel(Q, (uint32_t)Q.base_tile + ptile, (uint32_t)(j & 63u));
        return it.px.active;
    }
    __device__ __forceinline__ bool tile_item(const DParams &P, uint32_t tile, uint32_t lane, Item &it) const {
        const uint32_t ptile = l0_tile(P, tile, it.sample);
        // (the claimed tile is the same in every lane, and so is everything made from it and the kernel's arguments: said once more for the compiler)
        const uint32_t G = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)Q.base_tile + ptile));
        it.px = view_pixel(Q, G, lane);
        return it.px.active;
    }
    __device__ __forceinline__ Ray ray(const DParams &P, const Item &it) const { return view_ray(P, view_load(Q, it.px.v), it.px.x, it.px.y, it.sample); }
    __device__ __forceinline__ void finish(const DParams &P, const Item &it, unsigned long long j, V3 value) const {
        if (P.ss_par > 1u) {
            P.accum[j] = value.x; P.accum[P.n_items + j] = value.y; P.accum[2 * P.n_items + j] = value.z;
            return;
        }
        film_store(Q, it.px.pix, l0_finished(value));
    }
};

// W1, W3 and W4 of level 0
template <bool FAST, bool LDSS, bool PRUNE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) view_closest_kernel(const DParams P, const ViewArgs Q) {
    l0_closest_body<FAST, LDSS, PRUNE>(P, ViewSource{Q});
}
template <int KIND> __global__ void __launch_bounds__(LG_BLOCK, 3) view_shade_kernel(const DParams P, const ViewArgs Q) { l0_shade_body<KIND>(P, ViewSource{Q}); }
__global__ void __launch_bounds__(LG_BLOCK) view_combine_kernel(const DParams P, const ViewArgs Q) { l0_combine_body(P, ViewSource{Q}); }

// W5 (several samples a pixel): a pixel's samples summed in their order from zero, * 1 / S, quantised (integrate.rs:16-20, img.rs:46-67) --
// wf_resolve_kernel over the chunk's pixel tiles.  P.ntiles = the chunk's PIXEL tiles; the parked li() of pixel tile t, sample s, lane l
// sits at accum[(t * ss_par + s) * 64 + l].
__global__ void __launch_bounds__(LG_BLOCK) view_resolve_kernel(const DParams P, const ViewArgs Q) {
    const unsigned long long n_pix = (unsigned long long)P.ntiles * 64ull;
    const uint32_t S = P.ss_par;
    const double weight = 1. / (double)(P.ss_root * P.ss_root);
    for (unsigned long long q = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; q < n_pix; q += (unsigned long long)gridDim.x * LG_BLOCK) {
        const uint32_t t = (uint32_t)(q >> 6), l = (uint32_t)(q & 63u);
        const ViewPixel px = view_pixel(Q, (uint32_t)Q.base_tile + t, l);
        if (!px.active) continue;
        V3 color = vzero();
        for (uint32_t sidx = 0; sidx < S; ++sidx) {
            const unsigned long long i = ((unsigned long long)t * S + sidx) * 64ull + l;
            color = color + V3{P.accum[i], P.accum[P.n_items + i], P.accum[2 * P.n_items + i]};
        }
        film_store(Q, px.pix, color * weight);
    }
}

// ---- host-callable launchers (launch.cpp, enqueue_view_batch).  The closest pass: the forms and their operations are travform.h's.
template <bool F, bool L, bool Z> struct ViewKernels {
    static constexpr int variants = 1;
    static const void *kernel(int) { return reinterpret_cast<const void *>(view_closest_kernel<F, L, Z>); }
};
hipError_t launch_view_closest(const DParams &P, const ViewArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream) {
    void *args[] = {const_cast<DParams *>(&P), const_cast<ViewArgs *>(&Q)};
    return trav_launch<ViewKernels>(P, fast, 0, blocks, stack_depth, args, stream);
}
hipError_t launch_view_shade(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream) {
    return l0_launch<ViewArgs>(P.wf_levels == 1u ? view_shade_kernel<0> : view_shade_kernel<1>, P, Q, blocks, stream);
}
hipError_t launch_view_combine(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream) { return l0_launch<ViewArgs>(view_combine_kernel, P, Q, blocks, stream); }
hipError_t launch_view_resolve(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(view_resolve_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t view_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<ViewKernels>(bytes, ldss); }

} // namespace lg
