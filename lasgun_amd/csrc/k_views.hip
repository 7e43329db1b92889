// lasgun_amd/csrc/k_views.hip -- view batches (include/lasgun_hip.h, lg_capture_views*): one accel seen from K cameras into K films of one
// size, LEVEL 0 of the level-by-level pipeline (k_wavefront.hip) a fourth time.  k_radiance.hip is level 0 for rays the caller wrote out and
// k_gather.hip for rays made from two tables; here the rays are the render's own -- camera_ray()'s expression (shade.h, Camera::sample) --
// over a camera that is a row of a table (DView) instead of eight fields of DParams.  The three passes are k_radiance.hip's film forms (and
// rq_closest_body.h) with exactly three things replaced -- read them side by side with wf_trace_kernel's L0 branch:
//   * "slot base + i is active while < n" by the work tile -> (view, pixel, sample) mapping (view_pixel).  Work tile vt of a chunk is pixel
//     tile vt / ss_par of the chunk at sample vt % ss_par, the render's samples side by side (shade.h, l0_tile); pixel tile t of the chunk is
//     global pixel tile G = base_tile + t = v * tiles_per_view + tile-of-film-v, an 8 x 8 tile of film v as pixel_of's mode 0 cuts it
//     (tx = tile % tiles_x; lane l is pixel (8 tx + (l & 7), 8 ty + (l >> 3))).  v is the same in every lane of the closest pass: the view's
//     16 doubles are read through a wave-uniform index from the constant address space, scalar loads, not 30 more vector registers in
//     kernels that sit at their register budget;
//   * rq_load_ray by view_ray -- camera_ray()'s expression word for word over the view's fields, ss_distance as the host made it
//     (1.0 / (double)samples_root) --, in the closest pass and again in the shade pass (wo depends on it; the same expression gives the same
//     bits; a hit's lanes there come from any tile, so the record is read per lane);
//   * rq_finish by view_finish: one sample a pixel -> (0 + li) * 1.0 as one 4-byte store and / or three doubles at the pixel of film v
//     (film_store's arithmetic); several -> the sample's li parked at the work item's slot of the chunk's `accum`, as finish_pixel does under
//     ss_par, and view_resolve_kernel sums a pixel's samples in their order per chunk (wf_resolve_kernel's arithmetic: chunks hold whole
//     pixel tiles x S).  Every pixel of every film is written exactly once, however the chunks are cut.
// The walk, the hit queue, the parked frame, wave_append and every f64 expression are kept as they are there; levels >= 1 and every shadow
// pass are the render's own kernels.  The bodies and camera_ray()'s expression are repeated, not shared: the render's, radiance and film
// kernels compile to exactly what they were before this file existed (profiles/r17_kernel_resources_diff.txt).
// view_pixel, view_load and view_ray are view_ray.h's: k_view_features.hip maps the same tiles to the same pixels and makes the same rays.
#include "wflevel.h"
#include "travform.h"
#include "view_ray.h"

namespace lg {

// the film word / radiance triple of a finished pixel of film v (k_radiance.hip, film_store)
__device__ __forceinline__ void view_store(const ViewArgs &Q, unsigned long long pix, V3 color) {
    if (Q.rgba) Q.rgba[pix] = to_byte(color.x) | (to_byte(color.y) << 8) | (to_byte(color.z) << 16) | (255u << 24);
    if (Q.rgb) {
        double *o = Q.rgb + 3ull * pix;
        o[0] = color.x; o[1] = color.y; o[2] = color.z;
    }
}
// integrate() (integrate.rs:16-20): one sample a pixel -> Color::zero() + li, * 1 / 1, written; several side by side -> this sample's li
// parked at work item `widx` until the resolve pass (shade.h, finish_pixel under ss_par)
__device__ __forceinline__ void view_finish(const DParams &P, const ViewArgs &Q, const ViewPixel &px, unsigned long long widx, V3 value) {
    if (P.ss_par > 1u) {
        P.accum[widx] = value.x; P.accum[P.n_items + widx] = value.y; P.accum[2 * P.n_items + widx] = value.z;
        return;
    }
    view_store(Q, px.pix, (vzero() + value) * 1.0);
}

// W1 of level 0: rq_closest_body.h with the three replacements
template <bool FAST, bool LDSS, bool PRUNE>
__global__ void __launch_bounds__(LDSS ? LG_LDSS_BLOCK : LG_BLOCK, LG_TRAV_WAVES_PER_SIMD) view_closest_kernel(const DParams P, const ViewArgs Q) {
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
        __syncthreads(); // the only workgroup-wide step; every wave reaches it before pulling tiles
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
        const unsigned long long i = (unsigned long long)tile * 64ull + lane; // the chunk's work item: index of level 0's arrays
        uint32_t sample;
        const uint32_t ptile = l0_tile(P, tile, sample);
        // (the claimed tile is the same in every lane, and so is everything made from it and the kernel's arguments: said once more for the compiler)
        const uint32_t G = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)Q.base_tile + ptile));
        const ViewPixel px = view_pixel(Q, G, lane);
        const bool active = px.active;
        Ray ray = ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0});
        if (active) ray = view_ray(P, view_load(Q, px.v), px.x, px.y, sample);
        Best b;
        b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
        if (active) walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
        const bool hit = active && b.ref != NO_HIT;
        // ---- this wave's slots in the level's hit queue (wflevel.h: dense where most lanes hit, appended otherwise)
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        const uint32_t nhit = (uint32_t)__builtin_popcountll(mask);
        unsigned long long h = i;
        if (nhit < WF_FULL_MIN) {
            P.wf_hq[i] = WF_NONE; // (every lane stands for slot i of the dense part, a pixel or a lane beyond the film's edge: the chunk's arrays hold whole tiles)
            if (nhit != 0u) {
                uint32_t base_v = 0u;
                if (lane == 0u) base_v = atomicAdd(P.wf_counts + P.wf_levels, nhit);
                h = P.wf_hit_cap + (uint32_t)__builtin_amdgcn_readfirstlane((int)base_v) + lanes_below(mask);
            }
        } else if (!hit) P.wf_hq[i] = WF_NONE; // a hole of a dense block
        if (hit) {
            P.wf_hq[h] = (uint32_t)i; // a bare index below 2^31, as in rq_closest_body.h: the chunks come from the same ChunkPlan
            Shade sh;
            shade_frame(P, ray, b, sh);
            const unsigned long long n = P.wf_hit_stride;
            double *f = P.frame + h;
            f[0 * n] = sh.praw.x; f[1 * n] = sh.praw.y; f[2 * n] = sh.praw.z;
            f[3 * n] = sh.ng.x; f[4 * n] = sh.ng.y; f[5 * n] = sh.ng.z;
            f[6 * n] = sh.ns.x; f[7 * n] = sh.ns.y; f[8 * n] = sh.ns.z;
            f[9 * n] = sh.ss.x; f[10 * n] = sh.ss.y; f[11 * n] = sh.ss.z;
            f[12 * n] = (double)sh.mat;
        } else if (active) { // integrate.rs:26-28
            const V3 value = background(P, normalize(ray.d));
            if (P.wf_levels == 1u) view_finish(P, Q, px, i, value);
            else {
                const unsigned long long n = P.wf_cap;
                P.wf_out[i] = value.x; P.wf_out[n + i] = value.y; P.wf_out[2 * n + i] = value.z;
                P.wf_child[i] = WF_MISS;
            }
        }
    }
}

// W3 of level 0: rq_shade_body with the ray made again from the hit's work item
template <int KIND>
__global__ void __launch_bounds__(LG_BLOCK, 3) view_shade_kernel(const DParams P, const ViewArgs Q) {
    const HitSlots hs = hit_slots(P, 0u, 64u);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long t = (unsigned long long)blockIdx.x * (LG_BLOCK / 64u) + wave;
    if (t >= hs.tiles) return; // (whole waves stay together: the appends of KIND 1 are wave-wide)
    unsigned long long h = 0;
    const bool valid = hit_of(P, hs, (uint32_t)t, lane, h);
    unsigned long long j = 0;
    ViewPixel px;
    px.active = false; px.pix = 0ull;
    bool has_r = false, has_t = false;
    Sample sr, st;
    Shade sh;
    V3 output = vzero();
    if (valid) {
        j = P.wf_hq[h];
        uint32_t sample;
        const uint32_t ptile = l0_tile(P, (uint32_t)(j >> 6), sample);
        px = view_pixel(Q, (uint32_t)Q.base_tile + ptile, (uint32_t)(j & 63u)); // (a hit's item is active)
        const Ray ray = view_ray(P, view_load(Q, px.v), px.x, px.y, sample);
        const unsigned long long n = P.wf_hit_stride;
        const double *f = P.frame + h;
        V3 p{f[0 * n], f[1 * n], f[2 * n]};
        sh.ng = V3{f[3 * n], f[4 * n], f[5 * n]};
        sh.ns = V3{f[6 * n], f[7 * n], f[8 * n]};
        sh.ss = V3{f[9 * n], f[10 * n], f[11 * n]};
        sh.mat = (int32_t)f[12 * n];
        sh.wo = -normalize(ray.d);
        const double err = 2.220446049250313e-16 * 65536.0;
        V3 p_err = sh.ng * err;
        sh.praw = p; sh.p = p + p_err; sh.pm = p - p_err;
        sh.ts = cross(sh.ns, sh.ss);
        const DMaterial m = P.materials[sh.mat];
        const uint32_t vis = P.nlights ? P.vis[h] : 0u;
        output = shade_lights(P, m, sh, vis); // integrate.rs:47-67
        if (KIND == 1 && (m.kind == MAT_GLASS || m.kind == MAT_MIRROR)) { // depth < max recursion (integrate.rs:69-77)
            if (sample_specular_transmission(m, sh, st))
                has_t = !(st.pdf <= 0.0 || veq(st.spectrum, vzero()) || fabs(dot(st.wi, sh.ns)) == 0.0);
            if (sample_specular_reflection(m, sh, sr))
                has_r = !(sr.pdf <= 0.0 || veq(sr.spectrum, vzero()) || dot(sr.wi, sh.ns) <= 0.0);
        }
    }
    if (KIND == 0) { // integrate.rs:79 with no children
        if (valid) view_finish(P, Q, px, j, output + vzero() + vzero());
        return;
    }
    // children: consecutive slots of level 1's ray queue per wavefront and kind
    const uint32_t cr = wave_append(P.wf_counts + 1u, has_r);
    const uint32_t ct = wave_append(P.wf_counts + 1u, has_t);
    if (!valid) return;
    const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
    P.wf_out[j] = output.x; P.wf_out[n + j] = output.y; P.wf_out[2 * n + j] = output.z;
    P.wf_child[j] = has_r ? cr : WF_NONE;
    P.wf_child[n + j] = has_t ? ct : WF_NONE;
    double *sp = P.wf_spec + j;
    if (has_r) {
        sp[0 * n] = sr.spectrum.x; sp[1 * n] = sr.spectrum.y; sp[2 * n] = sr.spectrum.z;
        const V3 wr = -1.0 * sh.wo + 2.0 * dot(sh.wo, sh.ns) * sh.ns; // bxdf::util::reflect (integrate.rs:100)
        double *q = P.wf_q_next + cr;
        q[0 * nn] = sh.p.x; q[1 * nn] = sh.p.y; q[2 * nn] = sh.p.z; q[3 * nn] = wr.x; q[4 * nn] = wr.y; q[5 * nn] = wr.z;
    }
    if (has_t) {
        sp[3 * n] = st.spectrum.x; sp[4 * n] = st.spectrum.y; sp[5 * n] = st.spectrum.z;
        sp[6 * n] = fabs(dot(st.wi, sh.ns)); sp[7 * n] = st.pdf;
        double *q = P.wf_q_next + ct;
        q[0 * nn] = sh.pm.x; q[1 * nn] = sh.pm.y; q[2 * nn] = sh.pm.z; q[3 * nn] = st.wi.x; q[4 * nn] = st.wi.y; q[5 * nn] = st.wi.z;
    }
}

// W4 of level 0: rq_combine_body over the chunk's work items
__global__ void __launch_bounds__(LG_BLOCK) view_combine_kernel(const DParams P, const ViewArgs Q) {
    const unsigned long long n_work = (unsigned long long)P.ntiles * 64ull;
    const unsigned long long n = P.wf_cap, nn = P.wf_cap_next;
    for (unsigned long long j = (unsigned long long)blockIdx.x * LG_BLOCK + threadIdx.x; j < n_work; j += (unsigned long long)gridDim.x * LG_BLOCK) {
        uint32_t sample;
        const uint32_t ptile = l0_tile(P, (uint32_t)(j >> 6), sample);
        const ViewPixel px = view_pixel(Q, (uint32_t)Q.base_tile + ptile, (uint32_t)(j & 63u));
        if (!px.active) continue;
        V3 value{P.wf_out[j], P.wf_out[n + j], P.wf_out[2 * n + j]};
        const uint32_t c0 = P.wf_child[j];
        if (c0 != WF_MISS) {
            const uint32_t c1 = P.wf_child[n + j];
            const double *sp = P.wf_spec + j;
            V3 reflected = vzero(), refracted = vzero();
            if (c0 != WF_NONE) {
                const V3 l{P.wf_out_next[c0], P.wf_out_next[nn + c0], P.wf_out_next[2 * nn + c0]};
                reflected = mul_ew(V3{sp[0 * n], sp[1 * n], sp[2 * n]}, l); // integrate.rs:103
            }
            if (c1 != WF_NONE) {
                const V3 l{P.wf_out_next[c1], P.wf_out_next[nn + c1], P.wf_out_next[2 * nn + c1]};
                refracted = mul_ew(V3{sp[3 * n], sp[4 * n], sp[5 * n]}, l) * sp[6 * n] / sp[7 * n]; // integrate.rs:129
            }
            value = value + reflected + refracted; // integrate.rs:79
        }
        view_finish(P, Q, px, j, value);
    }
}

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
        view_store(Q, px.pix, color * weight);
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
    if (P.wf_levels == 1u) hipLaunchKernelGGL((view_shade_kernel<0>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    else hipLaunchKernelGGL((view_shade_kernel<1>), dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t launch_view_combine(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(view_combine_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t launch_view_resolve(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(view_resolve_kernel, dim3(blocks), dim3(LG_BLOCK), 0, stream, P, Q);
    return hipGetLastError();
}
hipError_t view_set_lds_limit(size_t bytes, bool ldss) { return trav_set_lds_limit<ViewKernels>(bytes, ldss); }

} // namespace lg
