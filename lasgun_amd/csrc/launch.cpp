// lasgun_amd/csrc/launch.cpp -- one render enqueued on a stream (internal.h): the launch contexts, the three kernel organisations
// (level by level, queue, megakernel), the fitted rule and the measured choice between them (tune.cpp does the measuring), and the
// addressing modes of capture_subset (strided subsets, batches, lattice tiling).
#include "internal.h"
#include "choice.h"
#include "packet_host.h"
#include "fused_host.h"
#include "tri_frames_host.h"

// The launch context of `stream` (at most MAX_LAUNCH_CTXS are kept; the least recently used one is recycled after a
// device-wide synchronise).  Caller holds a.mtx and has made the accel's device current.
lg_accel::LaunchCtx &ctx_for(const lg_accel &a, hipStream_t stream) {
    for (auto &c : a.ctxs)
        if (c->key == stream) { c->last_use = ++a.ctx_clock; return *c; }
    lg_accel::LaunchCtx *c = nullptr;
    if (a.ctxs.size() < MAX_LAUNCH_CTXS) {
        a.ctxs.emplace_back(new lg_accel::LaunchCtx());
        c = a.ctxs.back().get();
        c->tile_counter.alloc(TILE_COUNTER_WORDS);
        HIP_TRY(hipMemset(c->tile_counter.p, 0, TILE_COUNTER_WORDS * sizeof(uint32_t)));
    } else {
        c = a.ctxs[0].get();
        for (auto &x : a.ctxs) if (x->last_use < c->last_use) c = x.get();
        HIP_TRY(hipDeviceSynchronize()); // nothing may still be using the recycled buffers
    }
    c->key = stream;
    c->last_use = ++a.ctx_clock;
    return *c;
}

// The queue organisation's error word: a wave that gave up waiting for work that never came (a scheduler bug) must fail a call, not
// leave a half-rendered film behind.  The word is sticky -- the device only ever sets it -- and is cleared here, once reported.
// Looked at after every synchronise of the accel's stream, at the head of every enqueue and in lg_accel_synchronize: a launch on a
// CALLER's stream that stalled is reported by the first of those that follows its end.  Caller holds a.mtx.
void check_queue_error(const lg_accel &a) {
    if (!a.q_err) return;
    volatile uint32_t *w = a.q_err;
    if (*w == 0u) return;
    *w = 0u;
    throw Error("queue organisation: a wave gave up waiting for work (scheduler stalled); the film is incomplete");
}
void sync_checked(const lg_accel &a) {
    HIP_TRY(hipStreamSynchronize(a.stream));
    check_queue_error(a);
}

// ------------------------------------------------------------------------------------------
DParams base_params(const lg_accel &a, uint32_t w, uint32_t h) {
    const Scene &s = *a.scene;
    DParams P{};
    P.nodes = a.nodes.p; P.nodes4 = a.nodes4.p; P.primref = a.primref.p; P.spheres = a.spheres.p; P.sphere_mat = a.sphere_mat.p;
    P.cuboids = a.cuboids.p; P.cuboid_mat = a.cuboid_mat.p; P.tri_v = a.tri_v.p; P.tri_n = a.tri_n.p; P.tri_t = a.tri_t.p;
    P.vpos = a.vpos.p; P.vnorm = a.vnorm.p; P.vtex = a.vtex.p; P.leaf_soup = a.leaf_soup.p; P.chunks = a.chunks.p; P.strips = a.strips.p; P.sphere_ref_leaf = a.sphere_ref_leaf.p; P.cuboid_ref_leaf = a.cuboid_ref_leaf.p;
    P.tri_ref_leaf = a.tri_ref_leaf.p; P.accel_ref_leaf = a.accel_ref_leaf.p; P.accels = a.accels.p; P.materials = a.materials.p;
    P.lights = a.lights.p;
    P.nlights = (uint32_t)a.flat.lights.size();
    P.recursion = s.recursion;
    P.default_material = a.flat.default_material;
    P.stack_depth = a.stack_depth;
    {   // LASGUN_ACCEL_LDS=0 (A/B): the accel records from the DAccel table in L2
        static const bool accel_lds = env_on("LASGUN_ACCEL_LDS");
        P.accel_image = a.accel_image_n16 && accel_lds ? a.accel_image.p : nullptr; P.accel_image_n16 = a.accel_image_n16;
    }
    {   // LASGUN_PRUNE=0|1 replaces the scene-dependent DEFAULT (prune_env); lg_accel_set_prune still wins
        P.prune = prune_effective(a) ? 1u : 0u;
    }
    {   // LASGUN_SHADOW_SKIP=0 / lg_accel_set_shadow_skip(0) (A/B, tests): every hit's shadow rays are walked.  The flag's argument (shade.h,
        // light_irrelevant) needs PI * intensity finite for every light; the visibility word holds 32 lights.
        static const bool skip_env = env_on("LASGUN_SHADOW_SKIP");
        bool ok = skip_env && a.shadow_skip && !a.flat.lights.empty() && a.flat.lights.size() <= 32;
        for (const DLight &L : a.flat.lights)
            for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(PI * L.intensity[k]);
        P.shadow_skip = ok ? 1u : 0u;
    }
    {   // LASGUN_LEVEL_DOOR=0..3 / lg_accel_set_level_door (A/B, tests): which shortcuts the exact walk takes where it enters a nested accel --
        // bit 0 the probe at the door, bit 1 a lone mesh and its group as one level.  Same results with every mask.
        static const uint32_t door_env = [] { const char *e = std::getenv("LASGUN_LEVEL_DOOR"); return e && e[0] >= '0' && e[0] <= '3' && !e[1] ? (uint32_t)(e[0] - '0') : 3u; }();
        P.level_door = door_env & a.level_door;
    }
    P.cam_origin = s.camera.origin; P.cam_view = s.camera.view; P.cam_up = s.camera.up; P.cam_aux = s.camera.aux;
    P.image_plane_height = s.camera.image_plane_height;
    P.pixel_separation = s.camera.pixel_separation;
    P.ss_distance = s.camera.ss_distance;
    P.ss_root = s.camera.ss_root;
    {   // LASGUN_SLAB_SIGNS=0: the reference's slab formula as written in every node step (A/B, tests)
        static const bool signs = env_on("LASGUN_SLAB_SIGNS");
        P.boxes_finite = a.flat.boxes_finite && signs ? 1u : 0u;
    }
    P.ah_omax = a.flat.ah_omax; P.ah_dmin = a.flat.ah_dmin; P.ah_dmax = a.flat.ah_dmax;
    P.bg_inner = s.bg_inner; P.bg_outer = s.bg_outer; P.bg_scale = s.bg_scale;
    P.ambient = s.ambient;
    P.w = w; P.h = h;
    P.winv = 1. / (double)w; P.hinv = 1. / (double)h; P.aspect = (double)w / (double)h; // film.rs:40-42
    return P;
}

// the accel's internal streams (bands of a big wavefront launch, bands of a whole-film capture).  Caller holds a.mtx.
void ensure_aux_streams(const lg_accel &a, unsigned n) {
    while (a.aux_streams.size() < n) {
        hipStream_t st = g_streams.take(a.device); hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        a.aux_streams.push_back(st); a.aux_done.push_back(ev);
    }
    if (!a.aux_fork) HIP_TRY(hipEventCreateWithFlags(&a.aux_fork, hipEventDisableTiming));
}

// the LDS-resident scene into a launch's parameters: the kernels then run in their 1024-lane forms and read the tables from LDS
void set_lds_scene(const lg_accel &a, DParams &P) {
    P.lds_image = a.lds_image.p; P.lds_image_n16 = a.lds_image_n16;
    P.lds_node_off = a.lds_node_off; P.lds_prim_off = a.lds_prim_off; P.lds_soup_off = a.lds_soup_off; P.lds_accel_off = a.lds_accel_off;
    // ... which holds pair records in place of the node records when lds_pairs says so (dscene.h; never for a pruned launch: lds_resident)
    const bool pairs = a.lds_pairs;
    P.lds_pairs = pairs ? 1u : 0u;
    a.last_node_pairs = pairs ? 1 : 0;
    for (size_t i = 0; i < L0_REL_MAX_ACCELS; ++i) {
        const bool have = pairs && a.pair_rel.size() <= L0_REL_MAX_ACCELS && i < a.pair_rel.size();
        P.pair_rel[i].root_off = have ? a.pair_rel[i][0] : 0u; P.pair_rel[i].pair_off = have ? a.pair_rel[i][1] : 0u; P.pair_rel[i].pair_n = have ? a.pair_rel[i][2] : 0u;
        P.pair_rel[i].pad = 0u;
    }
}

// ---- the two organisations that keep every recursion level's rays in arrays of their own (k_wavefront.hip, k_queue.hip) -------------
static uint32_t levels_of(const lg_accel &a, const DParams &P) { return (a.flat.has_specular && P.recursion > 0) ? P.recursion + 1u : 1u; }
constexpr size_t WF_FULL_MIN_HOST = 48; // == WF_FULL_MIN of k_wavefront.hip
constexpr uint32_t MEGA_SPLIT = 4;      // the parts a small launch's tiles are handed out in where the measured choice found that faster (enqueue_mega, enqueue_queue)
// the parts a launch's tiles are handed out in -- lg_accel_set_tile_parts, or the measured choice's candidate (`split`) -- and DParams::split_shift for them
static std::pair<uint32_t, uint32_t> tile_parts(const lg_accel &a, bool split) {
    const uint32_t parts = a.tile_parts >= 1 ? (uint32_t)a.tile_parts : split ? MEGA_SPLIT : 1u;
    return {parts, parts == 8u ? 3u : parts == 4u ? 2u : parts == 2u ? 1u : 0u};
}

// A profiled span of a stream: two HIP events around what is enqueued on it between the span's declaration and end(), which hands the pair
// over (lg_profile_read* reads and destroys it).  Profiling off: no HIP call.  An enqueue that throws in between: the events are destroyed.
struct Span {
    struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } e0, e1;
    hipStream_t s;
    Span(const lg_accel &a, hipStream_t stream) : s(stream) { if (a.profiling) { HIP_TRY(hipEventCreate(&e0.e)); HIP_TRY(hipEventCreate(&e1.e)); HIP_TRY(hipEventRecord(e0.e, s)); } }
    void end(std::vector<std::pair<hipEvent_t, hipEvent_t>> &into) { if (e0.e) { HIP_TRY(hipEventRecord(e1.e, s)); into.emplace_back(e0.e, e1.e); e0.e = e1.e = nullptr; } }
};
// ... around ONE kernel on its launch stream
template <class F> static void timed(const lg_accel &a, int kind, hipStream_t s, F &&launch) {
    Span span(a, s);
    HIP_TRY(launch());
    span.end(a.kind_events[kind]);
}

// A chunk's level arrays, carved from a launch context's wf_mem
struct LevelArrays {
    std::vector<double *> q, out, spec;
    std::vector<uint32_t *> child;
    double *accum = nullptr;
};
// The chunks a launch of either organisation is cut into.  Queue capacities are worst case (level d holds at most 2^d rays per level-0
// work item of the chunk), so nothing can overflow, and the chunk is sized to the memory budget of a launch context.
struct ChunkPlan {
    bool queue;                    // the queue organisation's constants, else the level-by-level pipeline's
    uint32_t levels, nsamples, S;  // S: level-0 work items per pixel
    size_t per_item = 0;           // bytes per level-0 work item
    size_t *budget;                // a.queue_budget / a.wf_budget
    unsigned long long chunk_tiles = 0;

    // `extra`: the organisation's own bytes per level-0 work item beside the level arrays
    ChunkPlan(const lg_accel &a, const DParams &P0, bool queue_org, uint32_t S_, size_t extra)
        : queue(queue_org), levels(levels_of(a, P0)), nsamples(P0.ss_root * P0.ss_root), S(S_), budget(queue_org ? &a.queue_budget : &a.wf_budget) {
        per_item = (nsamples > 1 ? 3 * 8 : 0) + extra;
        for (uint32_t d = 0; d < levels; ++d) {
            size_t b = 0;                                 // per ray of level d
            if (d >= 1) b += 6 * 8;                       // ray queue
            if (levels > 1) b += 3 * 8;                   // output / li
            if (d + 1 < levels) b += 8 * 8 + 2 * 4;       // children's weights and indices
            per_item += b << d;
        }
        if (*budget == 0) *budget = budget_from_free_memory();
        chunk_tiles = *budget / (per_item * S * 64);
        const unsigned long long cap_limit = ((queue ? 0xFFFFFF00ull : 0x7FFFFFF0ull) >> (levels - 1)) / (64ull * S); // ray indices are 32-bit (level by level, a render and a radiance query alike: 31, WF_SKIP sits above them -- rq_closest_body.h and level0.h's closest body store bare indices and rely on it)
        if (chunk_tiles > cap_limit) chunk_tiles = cap_limit;
        if (chunk_tiles < 1) chunk_tiles = 1;
        if (chunk_tiles > P0.ntiles) chunk_tiles = P0.ntiles;
        if (queue && chunk_tiles < P0.ntiles && P0.mode == 0u && P0.tiles_x != 0u && chunk_tiles >= (unsigned long long)P0.tiles_x * 32ull)
            chunk_tiles -= chunk_tiles % ((unsigned long long)P0.tiles_x * 32ull); // whole rows of 32 x 32-tile blocks: the block order applies to every chunk
    }
    // Per launch CONTEXT, and an accel keeps up to MAX_LAUNCH_CTXS of them plus the band contexts (a caller with four frames in flight uses
    // five): a sixteenth of the free memory, at most 8 GiB each (the headline frame needs 3.3 GB and stays one chunk).  The queue
    // organisation with a recursive scene: up to a quarter (at most 48 GiB), so that a 4096^2 frame is one launch.  An allocation that
    // fails anyway halves the chunk (fit).
    size_t budget_from_free_memory() const {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const bool deep = queue && levels > 1;
        size_t b = deep ? free_b / 4 : free_b / 16;
        const char *env = std::getenv(queue ? "LASGUN_QUEUE_BUDGET_MB" : "LASGUN_WF_BUDGET_MB");
        if (env && std::atoll(env) > 0) {
            b = (size_t)std::atoll(env) << 20;
            if (queue) return b; // (as given: tests cut small films into many chunks with it)
        } else if (b > (deep ? (48ull << 30) : (8ull << 30))) b = deep ? (48ull << 30) : (8ull << 30);
        return b < (64ull << 20) ? (64ull << 20) : b;
    }
    unsigned long long n0() const { return chunk_tiles * 64ull * S; } // level 0's work items per chunk
    size_t need() const { return (size_t)n0() * per_item + 4096 * ((queue ? 4 : 3) * levels + 4); } // (+ the carve's alignment)

    // Runs `alloc` (the organisation's allocations for a chunk); memory that is not there (other contexts, other accels, other processes):
    // halve the chunk and run it again
    template <class F> void fit(F &&alloc) {
        for (;;) {
            try { alloc(); return; }
            catch (const Error &e) {
                if (std::string(e.what()).find("hipMalloc") == std::string::npos || chunk_tiles <= 1) throw;
                (void)hipGetLastError(); // (the failed allocation's error must not be what the next launch reports)
                chunk_tiles = (chunk_tiles + 1) / 2;
                *budget = std::max<size_t>(*budget / 2, 64ull << 20); // (later launches start from what fitted)
                if (std::getenv("LASGUN_DEBUG")) std::fprintf(stderr, "[lasgun] %s: %s -- chunks of %llu tiles instead\n", queue ? "queue" : "wavefront", e.what(), chunk_tiles);
            }
        }
    }
    // One chunk's level arrays in `mem` (256-byte aligned): each level's rays, output, children's weights and indices; then whatever `mid`
    // takes; then the sample accumulator
    template <class F> LevelArrays carve(uint8_t *mem, F &&mid) const {
        LevelArrays k;
        k.q.assign(levels, nullptr); k.out.assign(levels, nullptr); k.spec.assign(levels, nullptr); k.child.assign(levels, nullptr);
        uint8_t *cur = mem;
        auto take = [&](size_t bytes) { uint8_t *p = cur; cur += (bytes + 255) & ~(size_t)255; return p; };
        for (uint32_t d = 0; d < levels; ++d) {
            const size_t cap = (size_t)n0() << d;
            if (d >= 1) k.q[d] = (double *)take(cap * 6 * 8);
            if (levels > 1) k.out[d] = (double *)take(cap * 3 * 8);
            if (d + 1 < levels) { k.spec[d] = (double *)take(cap * 8 * 8); k.child[d] = (uint32_t *)take(cap * 2 * 4); }
        }
        mid(take);
        k.accum = nsamples > 1 ? (double *)take((size_t)n0() * 3 * 8) : nullptr;
        return k;
    }
};

// The passes of a chain of the level-by-level pipeline that are not the render's own, bound to the kernel arguments `q` of whoever makes level
// 0's rays (level0.h's sources: a radiance query's or a ray film's rays, k_radiance.hip; a radiance gather's, k_gather.hip; a view batch's,
// k_views.hip; light groups, k_light_groups.hip): level 0's three passes, the levels below are the render's.  `resolve`: what the source
// enqueues behind a chunk's chain (a view batch of several samples a pixel; P.ntiles = the chunk's pixel tiles).  `lg`, light groups: the shade
// and combine passes of every level below are the source's too (every_level), they carry lg->n_groups planes, with a spread pass at the
// deepest level; `xout` then holds each level's planes 1 .. G-1 (WfChunk::xout) and level() tells lg which the next launches work on.
// Nothing bound: the scene's own camera (k_wavefront.hip) -- a render.
struct Level0 {
    typedef hipError_t (*Closest)(const DParams &, const void *, bool, uint32_t, uint32_t, hipStream_t);
    typedef hipError_t (*Flat)(const DParams &, const void *, uint32_t, hipStream_t);
    const void *q = nullptr;
    Closest closest_ = nullptr;
    Flat shade_ = nullptr, combine_ = nullptr, resolve_ = nullptr;
    // level 0's shadow pass, where the lights are the call's and not the scene's (lit scatter, k_lit.hip): with own_shadow the render's
    // shadow pass is not launched at level 0 whatever lights the scene has, and shadow_ (nullptr: a call without lights) is launched in its
    // place over the hit tiles x vis_words work tiles
    bool own_shadow = false;
    Closest shadow_ = nullptr;
    uint32_t vis_words = 1;
    GroupArgs *lg = nullptr;
    const std::vector<double *> *xout = nullptr;
    bool own() const { return q != nullptr; }
    bool every_level() const { return lg != nullptr; }
    void level(uint32_t d) const {
        if (!lg) return;
        lg->xout = (*xout)[d];
        lg->xout_next = d + 1 < xout->size() ? (*xout)[d + 1] : nullptr;
    }
    hipError_t spread(const DParams &P, uint32_t blocks, hipStream_t s) const { return launch_lg_spread(P, *lg, blocks, s); }
    hipError_t closest(const DParams &P, bool fast, uint32_t blocks, uint32_t depth, hipStream_t s) const { return closest_(P, q, fast, blocks, depth, s); }
    hipError_t shadow(const DParams &P, bool fast, uint32_t blocks, uint32_t depth, hipStream_t s) const { return shadow_(P, q, fast, blocks, depth, s); }
    hipError_t shade(const DParams &P, uint32_t blocks, hipStream_t s) const { return shade_(P, q, blocks, s); }
    hipError_t combine(const DParams &P, uint32_t blocks, hipStream_t s) const { return combine_(P, q, blocks, s); }
    hipError_t resolve(const DParams &P, uint32_t blocks, hipStream_t s) const { return resolve_(P, q, blocks, s); }
};
// ... bound to a family's launchers (internal.h) and to its arguments, which live until the chunk's chain is enqueued
template <class ARGS> using L0Closest = hipError_t (*)(const DParams &, const ARGS &, bool, uint32_t, uint32_t, hipStream_t);
template <class ARGS> using L0Flat = hipError_t (*)(const DParams &, const ARGS &, uint32_t, hipStream_t);
template <class ARGS, L0Closest<ARGS> F> static hipError_t l0_closest(const DParams &P, const void *q, bool fast, uint32_t blocks, uint32_t depth, hipStream_t s) {
    return F(P, *static_cast<const ARGS *>(q), fast, blocks, depth, s);
}
template <class ARGS, L0Flat<ARGS> F> static hipError_t l0_flat(const DParams &P, const void *q, uint32_t blocks, hipStream_t s) { return F(P, *static_cast<const ARGS *>(q), blocks, s); }
template <class ARGS, L0Closest<ARGS> CLOSEST, L0Flat<ARGS> SHADE, L0Flat<ARGS> COMBINE> static Level0 bind_level0(const ARGS &Q) {
    Level0 l0;
    l0.q = &Q;
    l0.closest_ = l0_closest<ARGS, CLOSEST>;
    l0.shade_ = l0_flat<ARGS, SHADE>;
    l0.combine_ = l0_flat<ARGS, COMBINE>;
    return l0;
}
// Bottom-up after a sample's levels: li of level d's rays from their children's (integrate.rs:79, 103, 129), shared by both organisations
static void combine_levels(const lg_accel &a, DParams &P, const LevelArrays &K, const ChunkPlan &plan, hipStream_t s, const Level0 &l0 = Level0()) {
    const unsigned long long n0 = plan.n0();
    const uint32_t flat_blocks0 = (uint32_t)(((unsigned long long)P.ntiles * 64ull + 255ull) / 256ull), flat_cap = a.cus * 16u; // (level 0: one thread per work item)
    for (uint32_t d = plan.levels - 1; d-- > 0;) {
        P.wf_level = d;
        P.wf_cap = n0 << d; P.wf_cap_next = n0 << (d + 1);
        P.wf_out = K.out[d]; P.wf_spec = K.spec[d]; P.wf_child = K.child[d]; P.wf_out_next = K.out[d + 1];
        l0.level(d);
        if (l0.own() && (d == 0 || l0.every_level())) timed(a, 1, s, [&] { return l0.combine(P, d == 0 ? flat_blocks0 : flat_cap, s); });
        else timed(a, 1, s, [&] { return launch_wf_combine(P, d == 0 ? flat_blocks0 : flat_cap, s); });
    }
}
// ... and a pixel's samples summed in their order (k_wavefront.hip, wf_resolve_kernel)
static void resolve_samples(const lg_accel &a, const DParams &P, uint32_t pixel_tiles, hipStream_t s) {
    DParams R = P;
    R.ntiles = pixel_tiles;
    timed(a, 1, s, [&] { return launch_wf_resolve(R, (uint32_t)(((unsigned long long)pixel_tiles * 64ull + 255ull) / 256ull), s); });
}

// The gate of the level-0 closest pass's origin-relative form (k_wavefront.hip, l0_rewrite).  Wrong means wrong pixels, so every
// condition is stated: the plain exact walk over the LDS-resident scene with finite, ordered boxes; an accel whose records the form may
// rewrite (lg_accel::l0_rel); rays that camera_ray() makes from THIS launch's parameters, all from one origin that is the same bits in every
// lane (host.cpp, l0_relative_camera), and the same again in every accel's local space (l0_relative_origins).  LASGUN_L0_RELATIVE=0 /
// lg_accel_set_l0_relative(0): the absolute form, the parent's code path.  Fills P.l0_rel_n / P.l0_rel; false leaves P.l0_rel_n = 0.
static bool l0_relative(const lg_accel &a, DParams &P) {
    static const bool env = env_on("LASGUN_L0_RELATIVE");
    P.l0_rel_n = 0u;
    if (!env || !a.l0_relative || a.fast || P.prune || !P.lds_image || !P.boxes_finite || P.wf_level != 0u) return false;
    if (a.l0_rel.empty() || a.l0_rel.size() != a.flat.accels.size() || a.l0_rel.size() > L0_REL_MAX_ACCELS) return false;
    if (!l0_relative_camera(P.cam_origin, P.cam_up, P.cam_aux, P.pixel_separation)) return false;
    std::vector<V3> local;
    if (!l0_relative_origins(a.flat, P.cam_origin, local)) return false;
    for (size_t i = 0; i < a.l0_rel.size(); ++i) {
        P.l0_rel[i] = a.l0_rel[i];
        P.l0_rel[i].o[0] = local[i].x; P.l0_rel[i].o[1] = local[i].y; P.l0_rel[i].o[2] = local[i].z;
    }
    P.l0_rel_n = (uint32_t)a.l0_rel.size();
    return true;
}

// The gate of the packet form of level 0's closest pass (packet.h; the predicate is packet_host.h's).  Wrong means wrong
// pixels: the launch takes the pair form today, it is the camera's level 0 of the level-by-level pipeline, and every nested accel is one
// root record entered from the root accel.  LASGUN_PACKET_WALK=0 / lg_accel_set_packet_walk(0): the per-lane walk, the parent's kernel.
static uint32_t packet_walk(const lg_accel &a, const DParams &P, bool camera_level0) {
    static const bool env = env_on("LASGUN_PACKET_WALK");
    if (packet_launch_gate(wf_takes_pairs(P, a.fast), camera_level0, a.packet_walk && env) != PACKET_OK) return 0u;
    if (a.packet_scene < 0)
        a.packet_scene = (int)packet_scene_gate(a.flat.accels.data(), a.flat.accels.size(), a.flat.nodes.data(), a.flat.nodes.size(), a.flat.primref.data(),
                                                a.flat.primref.size(), a.stack_depth);
    return a.packet_scene == (int)PACKET_OK ? 1u : 0u;
}

// The gate of the fused form of the camera's level 0 (k_wavefront.hip, FUSED; the predicate is fused_host.h's).  Wrong means
// wrong pixels: the chain is the scene camera's own, level 0 is its only level, the scene has exactly one light, and this level's closest
// launch takes the packet form (P.packet, set just before) and its shadow launch the pair form.  LASGUN_FUSED_SHADE=0 /
// lg_accel_set_fused_shade(0): the three kernels, the parent's code path.
static uint32_t fused_shade(const lg_accel &a, const DParams &P, bool camera_level0, uint32_t levels) {
    static const bool env = env_on("LASGUN_FUSED_SHADE");
    FusedAsk q;
    q.switched_on = a.fused_shade && env;
    q.camera_level0 = camera_level0;
    q.levels = levels;
    q.nlights = (unsigned long)P.nlights;
    q.packet_closest = P.packet != 0u;
    q.pair_shadow = wf_takes_pairs(P, a.fast);
    return fused_shade_gate(q) == FUSED_OK ? 1u : 0u;
}

// The gate of the frame table in the fused packet closest launch (shade.h, shade_frame_tri; the predicate is
// tri_frames_host.h's): that launch alone, when the accel holds a table.  Sets P.tri_frames / tri_frame_base / tri_base, or leaves them
// null.  LASGUN_TRI_FRAMES=0 / lg_accel_set_tri_frames(0): every hit takes shade_frame's text, the parent's code path.
static bool tri_frames(const lg_accel &a, DParams &P) {
    static const bool env = env_on("LASGUN_TRI_FRAMES");
    P.tri_frames = nullptr; P.tri_frame_base = nullptr; P.tri_base = nullptr;
    if (!tri_frames_launch_gate(a.tri_frames_on && env, P.fused != 0u && P.packet != 0u && P.wf_level == 0u, a.tri_frame_records)) return false;
    if (!a.tri_frames.p || !a.tri_frame_base.p || !a.accel_tri_base.p || a.tri_frames.n != a.tri_frame_records) return false;
    P.tri_frames = a.tri_frames.p; P.tri_frame_base = a.tri_frame_base.p; P.tri_base = a.accel_tri_base.p;
    return true;
}

// ---- the level-by-level pipeline (k_wavefront.hip), shared by a render (enqueue_wavefront) and a radiance query (enqueue_radiance) ----
// A chunk's arrays in a launch context: the level arrays, and beside them the hit queue, frame and visibility of the widest level (dense
// part + appended part), the queue counts and a block of tile heads per launch
struct WfChunk {
    const ChunkPlan &plan;
    uint32_t levels, nlaunch;
    static constexpr uint32_t CL = TILE_COUNTER_WORDS; // the queue counts (3 per level) in the first block, then a block of tile heads per launch (one head per XCD, each on a line of its own)
    LevelArrays L;
    uint32_t *hq = nullptr, *vis = nullptr, *counters = nullptr;
    double *frame = nullptr;
    uint32_t groups;             // light groups (Level0::lg): planes of li per ray of every level; 1 for every other chain
    std::vector<double *> xout;  // ... planes 1 .. groups-1 of each level, where there are any (plane 0 is L.out)
    uint32_t vis_words;          // visibility words per hit slot (lit scatter, Level0::vis_words: > 1 with more than 32 lights in the call); 1 for every other chain
    WfChunk(const ChunkPlan &p, uint32_t groups_ = 1, uint32_t vis_words_ = 1) : plan(p), levels(p.levels), nlaunch(4 * p.levels), groups(groups_), vis_words(vis_words_) {}
    // ChunkPlan's `extra`: the hit queue, frame and visibility of the widest level (4 * (vis_words - 1) bytes more per hit slot); and 3 * 8 * (groups - 1) bytes per ray of each level of a recursive scene
    static size_t extra_per_item(uint32_t levels, uint32_t groups = 1, uint32_t vis_words = 1) {
        return ((size_t)(4 + STASH_DOUBLES * 8 + 4 * (size_t)vis_words) << (levels - 1)) * 7 / 4 + (levels > 1 ? (size_t)3 * 8 * (groups - 1) * (((size_t)1 << levels) - 1) : 0);
    }
    size_t hit_cap() const { return (size_t)plan.n0() << (levels - 1); }
    size_t hit_len() const { return hit_cap() + hit_cap() / 64 * (WF_FULL_MIN_HOST - 1); } // appended part: fewer than WF_FULL_MIN hits per block of 64 rays
    void carve(lg_accel::LaunchCtx &cx) { // this context's arrays for one chunk, grown if they have to be
        grow(cx.wf_mem, plan.need());
        grow(cx.wf_counters, CL * (1 + nlaunch));
        L = plan.carve(cx.wf_mem.p, [&](auto &take) {
            hq = (uint32_t *)take(hit_len() * 4);
            frame = (double *)take(hit_len() * STASH_DOUBLES * 8);
            vis = (uint32_t *)take(hit_len() * 4 * vis_words);
            xout.assign(levels, nullptr);
            for (uint32_t d = 0; levels > 1 && groups > 1 && d < levels; ++d) xout[d] = (double *)take(((size_t)plan.n0() << d) * 3 * 8 * (groups - 1));
        });
        counters = cx.wf_counters.p;
    }
    // what every launch of the chunk is told (P.ntiles = level 0's work tiles is the caller's)
    void params(const lg_accel &a, DParams &P) const {
        P.n_items = plan.n0(); // stride of the sample accumulator
        P.accum = L.accum;
        P.wf_levels = levels;
        P.wf_counts = counters;
        P.wf_hit_cap = hit_cap(); P.wf_hit_stride = hit_len(); P.wf_hq = hq; P.frame = frame; P.vis = vis;
        if (lds_resident(a)) set_lds_scene(a, P);
    }
    // One chain of launches on `ls`: the counters cleared, levels 0 .. L-1 top-down (closest, shadow, shade), the combine passes
    // bottom-up.  `l0`: whose forms level 0's three passes take (Level0; none: the camera's).
    void run(const lg_accel &a, DParams &P, hipStream_t ls, const Level0 &l0 = Level0()) const {
        const bool ldss = P.lds_image != nullptr;
        const uint32_t depth = a.fast ? a.stack_depth_fast1 : a.stack_depth;
        const uint32_t trace_cap = ldss ? a.ldss_blocks : (a.fast ? a.wf_blocks_fast : a.wf_blocks), flat_cap = a.cus * 16u;
        const uint32_t trace_blocks0 = ldss ? trace_cap : std::min(trace_cap, (P.ntiles + 3u) / 4u);
        // level-0 shade: one wave per dense tile and per tile the appended hits can fill (< WF_FULL_MIN of every 64 rays)
        const uint32_t shade_blocks0 = (uint32_t)(((unsigned long long)P.ntiles + ((unsigned long long)P.ntiles * (WF_FULL_MIN_HOST - 1) + 63ull) / 64ull + 3ull) / 4ull);
        const unsigned long long n0 = plan.n0();
        HIP_TRY(hipMemsetAsync(counters, 0, CL * (1 + nlaunch) * sizeof(uint32_t), ls));
        uint32_t launch_no = 0;
        auto level_params = [&](uint32_t d) {
            P.wf_level = d;
            P.wf_cap = n0 << d; P.wf_cap_next = n0 << (d + 1);
            P.wf_q = L.q[d]; P.wf_out = L.out[d]; P.wf_spec = L.spec[d]; P.wf_child = L.child[d];
            P.wf_q_next = d + 1 < levels ? L.q[d + 1] : nullptr;
            P.wf_out_next = d + 1 < levels ? L.out[d + 1] : nullptr;
            P.tile_counter = counters + CL * (1 + launch_no++);
            l0.level(d);
        };
        for (uint32_t d = 0; d < levels; ++d) {
            // (deeper levels: the number of rays is only known on the device; grids are sized for a full level 0, which
            // every deeper level may exceed only in waves, never in work per wave)
            const uint32_t tb = d == 0 ? trace_blocks0 : trace_cap, fb = d == 0 ? shade_blocks0 : flat_cap;
            const bool own0 = d == 0 && l0.own();
            level_params(d);
            P.packet = packet_walk(a, P, d == 0 && !own0); // (the camera's level 0 alone; every other launch of the chain: 0)
            if (d == 0) a.last_packet_walk = (int)P.packet;
            P.fused = d == 0 ? fused_shade(a, P, !own0 && !l0.every_level(), levels) : 0u; // (the camera's level 0 of a chain of one level: its closest and shadow launches shade, no shade pass follows)
            if (d == 0) { a.last_fused_shade = (int)P.fused; a.last_tri_frames = 0; }
            if (own0) timed(a, 0, ls, [&] { return l0.closest(P, a.fast, tb, depth, ls); });
            else {
                if (d == 0) a.last_l0_relative = l0_relative(a, P) ? 1 : 0; // (the camera's level 0: the form is chosen per launch, from this launch's camera)
                if (d == 0) a.last_tri_frames = tri_frames(a, P) ? 1 : 0;   // (the fused packet closest launch alone reads the frame table)
                timed(a, 0, ls, [&] { return launch_wf_trace(P, a.fast, false, tb, depth, ls); });
                P.l0_rel_n = 0u;
                P.tri_frames = nullptr; P.tri_frame_base = nullptr; P.tri_base = nullptr;
            }
            if (own0 && l0.own_shadow) { // (the call's lights: hit tiles x visibility words work tiles)
                if (l0.shadow_) {
                    // hs.tiles * W in 32 bits: a chunk holds fewer than 2^31 rays (ChunkPlan, cap_limit), so fewer than 2^25 * 7 / 4 hit tiles, and W <= 32
                    if (((unsigned long long)P.ntiles * 7ull / 4ull + 1ull) * l0.vis_words > 0xFFFFFFFFull) throw Error("level 0's shadow pass: hit tiles x visibility words do not fit 32 bits");
                    const uint32_t sb = ldss ? trace_cap : (uint32_t)std::min<unsigned long long>(trace_cap, ((unsigned long long)P.ntiles * l0.vis_words + 3ull) / 4ull);
                    level_params(d);
                    timed(a, 2, ls, [&] { return l0.shadow(P, a.fast, sb, depth, ls); });
                }
            } else
            if (P.nlights > 0) {
                level_params(d);
                timed(a, 2, ls, [&] { return launch_wf_trace(P, a.fast, true, tb, depth, ls); });
            }
            level_params(d);
            // (light groups, the deepest level of a recursive scene: the closest pass left a miss's background in plane 0 alone)
            if (l0.every_level() && d >= 1 && d + 1 == levels) timed(a, 1, ls, [&] { return l0.spread(P, flat_cap, ls); });
            if (own0 || l0.every_level()) timed(a, 3, ls, [&] { return l0.shade(P, fb, ls); });
            else if (!P.fused) timed(a, 3, ls, [&] { return launch_wf_shade(P, fb, ls); });
        }
        P.packet = 0u; P.fused = 0u;
        combine_levels(a, P, L, plan, ls, l0);
    }
};

// A render: per chunk of the film and per supersample, one chain (WfChunk::run).
static void enqueue_wavefront(const lg_accel &a, DParams &P0, lg_accel::LaunchCtx &c, hipStream_t stream) {
    const uint32_t levels = levels_of(a, P0);
    const uint32_t nsamples = P0.ss_root * P0.ss_root;
    // A supersampled launch runs its samples SIDE BY SIDE (DParams::ss_par): level 0 holds pixels x samples work items, one chain of
    // launches per chunk instead of one per sample, and a resolve pass sums each pixel's samples in their order.  The levels of a 9-sample
    // frame are nine times as wide -- a 512^2 film of glass fills the machine at its deep levels, which one sample at a time does not.
    // lg_accel_set_sample_order(1): one chain per sample, summed as they come.
    const uint32_t S = nsamples > 1 && a.sample_order != 1 ? nsamples : 1u; // level-0 work items per pixel
    // beside the level arrays: the hit queue, frame and visibility of the widest level, dense part + appended part
    ChunkPlan plan(a, P0, false, S, WfChunk::extra_per_item(levels));
    // Bands on internal streams: opt-in (lg_accel_set_wf_split, or LASGUN_WF_SPLIT=n as the default), launches of 2 Mpixel and
    // more.  Measured: one headline frame at a time 7.79 -> 7.50 ms with 4 bands, but 7.20 -> 7.46 ms
    // when the caller already keeps four frames in flight -- which is why it is not the default.
    static const unsigned split_env = [] { const char *e = std::getenv("LASGUN_WF_SPLIT"); return e && std::atoi(e) > 0 ? (unsigned)std::atoi(e) : 1u; }();
    const unsigned want = a.wf_split ? a.wf_split : split_env;
    // (at most MAX_WF_BANDS bands: their contexts and the callers' streams share the accel's MAX_LAUNCH_CTXS slots, and a
    // context that has to be recycled costs a device-wide synchronise)
    const unsigned split = (unsigned long long)P0.ntiles * 64ull >= (1ull << 21) ? std::min(want, MAX_WF_BANDS) : 1u;
    if (split > 1) plan.chunk_tiles = std::min<unsigned long long>(plan.chunk_tiles, (P0.ntiles + split - 1) / split);
    const unsigned long long nchunks = (P0.ntiles + plan.chunk_tiles - 1) / plan.chunk_tiles;
    const unsigned nstreams = split > 1 && nchunks > 1 ? (unsigned)std::min<unsigned long long>(split, nchunks) : 0u; // 0: everything on the caller's stream
    if (nstreams) ensure_aux_streams(a, nstreams);
    std::vector<WfChunk> carved;
    std::vector<hipStream_t> lanes;
    plan.fit([&] {
        carved.clear(); lanes.clear();
        if (nstreams) for (unsigned j = 0; j < nstreams; ++j) { lanes.push_back(a.aux_streams[j]); carved.emplace_back(plan); carved.back().carve(ctx_for(a, a.aux_streams[j])); }
        else { lanes.push_back(stream); carved.emplace_back(plan); carved.back().carve(c); }
    });
    const unsigned long long chunk_tiles = plan.chunk_tiles;
    if (nstreams) {
        HIP_TRY(hipEventRecord(a.aux_fork, stream)); // the bands start after whatever the caller's stream holds (a film clear, the previous frame's copy)
        for (unsigned j = 0; j < nstreams; ++j) HIP_TRY(hipStreamWaitEvent(a.aux_streams[j], a.aux_fork, 0));
    }

    const bool ldss = lds_resident(a);
    Span span(a, stream);
    if (std::getenv("LASGUN_DEBUG"))
        std::fprintf(stderr, "[lasgun] wavefront: levels %u, %llu tiles in chunks of %llu on %u stream(s) (%.1f MiB per context), trace grid %u x %u, stack %u, max_blocks %u\n", levels,
                     (unsigned long long)P0.ntiles, chunk_tiles, nstreams ? nstreams : 1u, plan.need() / 1048576.0, ldss ? a.ldss_blocks : (a.fast ? a.wf_blocks_fast : a.wf_blocks),
                     ldss ? 1024u : 256u, a.fast ? a.stack_depth_fast1 : a.stack_depth, a.max_blocks);
    // (A small frame's chain replayed as a HIP graph was measured in round 6 and retired: on this runtime a graph launch costs more than
    // the stream launches it replaces -- the README sphere at 512^2 0.086 -> 0.093 ms, Cornell plastic 0.119 -> 0.129 ms, every longer
    // chain within +-2 %; profiles/r06_small_frames.jsonl.)
    unsigned long long chunk_no = 0;
    for (unsigned long long t0 = 0; t0 < P0.ntiles; t0 += chunk_tiles, ++chunk_no) {
        const WfChunk &K = carved[chunk_no % carved.size()];
        const hipStream_t ls = lanes[chunk_no % lanes.size()]; // the stream of this chunk
        DParams P = P0;
        P.tile0 = (uint32_t)t0;
        const uint32_t pixel_tiles = (uint32_t)std::min<unsigned long long>(chunk_tiles, P0.ntiles - t0);
        P.ntiles = pixel_tiles * S; // level 0's work tiles
        P.ss_par = S;
        K.params(a, P);
#ifdef LG_STAMPS
        P.stats = a.stats.p;
        P.stamp_counts = reinterpret_cast<unsigned long long *>(a.stats.p + 1);
#endif
        for (uint32_t sidx = 0; sidx < nsamples / S; ++sidx) {
            P.sample_index = sidx;
            K.run(a, P, ls);
        }
        if (S > 1) resolve_samples(a, P, pixel_tiles, ls);
    }
    for (unsigned j = 0; j < nstreams; ++j) { // join: the caller's stream continues when every band is done
        HIP_TRY(hipEventRecord(a.aux_done[j], a.aux_streams[j]));
        HIP_TRY(hipStreamWaitEvent(stream, a.aux_done[j], 0));
    }
    span.end(a.events);
}

// A radiance query (query.cpp, lg_radiance*): li() of `n` caller-supplied rays through the same chain, on the caller's stream alone (no
// bands).  Level 0's work items are the query's SLOTS, 64 to a tile, cut into chunks of consecutive slots by the same plan -- with a
// permutation (lg_accel_set_query_order(1)) slot s is ray perm[s], so the chunks are cut from the sorted order.  One sample per ray,
// whatever the scene's camera supersamples; always this organisation, whatever lg_accel_set_streaming says: nothing is measured or
// remembered for it.  Caller holds a.mtx, has made the accel's device current and has checked the buffers and that the scene can go
// level by level (radiance_possible).
// A call is its SHAPE (Level0Call) and a per-chunk callback `bind(t0)`: told the chunk's first tile, it sets where the chunk starts in its
// kernel arguments (base / base_tile) and returns the passes bound to them (Level0).  The sources:
// rays (lg_radiance*, and with `film` lg_capture_rays* of one sample per pixel slot: ray r is pixel slot r and level 0 finishes it into the film
// (FilmArgs) instead of radiance[] -- the same chunks, the same launches with the film forms of the three level-0 kernels);
// a gather (lg_radiance_gather*): there is no ray array -- level 0's work items are the gather's tiles, whose rays its own forms of the three
// kernels make from two tables (k_gather.hip) and finish into its li;
// views (lg_capture_views*): there is no ray array either -- level 0's work items are the batch's global pixel tiles x S samples side by side,
// as a render's (enqueue_wavefront): the film size and samples_root go into the chunk's DParams, a chunk holds whole pixel tiles x S, and with
// S > 1 each chunk's parked samples are resolved behind its chain (Level0::resolve: k_views.hip, view_resolve_kernel; a combine pass, kind 1, as
// the render's resolve is).
// `tail`: what is enqueued behind the chunks inside the profiled span (a film's or a gather's resolve pass).
struct Level0Call {
    uint32_t tiles = 0;                // level 0's tiles of 64 work items (views: pixel tiles, x samples_root^2 work tiles each)
    uint32_t w = 1, h = 1;             // the film size the chunks' DParams are made for (views alone)
    uint32_t samples_root = 1;         // (the scene's camera may be supersampled; a query is not, and a view batch has its own samples_root)
    uint32_t planes = 1;               // planes of li per ray of every level (light groups alone: > 1)
    bool one_level = false;            // the chain is level 0 alone whatever depth the scene has (surface scatter: no children are followed, no combine)
    uint32_t vis_words = 1;            // visibility words per hit slot (lit scatter alone: > 1 with more than 32 lights in the call)
    const char *label = "";            // what LASGUN_DEBUG calls the query ...
    std::string note;                  // ... and how it ends its line (a query's rays: the order they are walked in)
};
template <class BIND>
static void enqueue_level0_query(const lg_accel &a, const Level0Call &call, BIND &&bind, lg_accel::LaunchCtx &c, hipStream_t stream, const std::function<void()> &tail = nullptr) {
    DParams P0 = base_params(a, call.w, call.h);
    P0.ss_root = call.samples_root;
    const uint32_t S = P0.ss_root * P0.ss_root; // level-0 work items per pixel
    P0.ntiles = call.tiles;
    if (call.one_level) P0.recursion = 0; // (levels_of: 1 -- the plan, the carve and P.wf_levels all follow from it; no level-by-level kernel reads P.recursion)
    const uint32_t levels = levels_of(a, P0);
    ChunkPlan plan(a, P0, false, S, WfChunk::extra_per_item(levels, call.planes, call.vis_words));
    WfChunk K(plan, call.planes, call.vis_words);
    plan.fit([&] { K.carve(c); });
    const unsigned long long chunk_tiles = plan.chunk_tiles;
    Span span(a, stream);
    if (std::getenv("LASGUN_DEBUG"))
        std::fprintf(stderr, "[lasgun] %s: levels %u, %llu tiles in chunks of %llu (%.1f MiB), %s\n", call.label, levels, (unsigned long long)P0.ntiles,
                     chunk_tiles, plan.need() / 1048576.0, call.note.c_str());
    for (unsigned long long t0 = 0; t0 < P0.ntiles; t0 += chunk_tiles) {
        DParams P = P0;
        P.tile0 = (uint32_t)t0;
        const uint32_t chunk = (uint32_t)std::min<unsigned long long>(chunk_tiles, P0.ntiles - t0);
        P.ntiles = chunk * S; // level 0's work tiles (at most the call's: 32 bits, views_host.h)
        P.ss_par = S;
        K.params(a, P);
        Level0 l0 = bind(t0);
        l0.xout = &K.xout; // (light groups: where the chunk carved planes 1 .. G-1 of each level)
        K.run(a, P, stream, l0);
        if (l0.resolve_) {
            DParams R = P;
            R.ntiles = chunk;
            timed(a, 1, stream, [&] { return l0.resolve(R, (uint32_t)(((unsigned long long)chunk * 64ull + 255ull) / 256ull), stream); });
        }
    }
    if (tail) tail();
    span.end(a.events);
}
// The rays of a radiance query, a ray film (`film`) or light groups (`groups`) as level 0's source: work item i of the chunk at tile t0 is
// slot 64 t0 + i of the query
static void enqueue_ray_query(const lg_accel &a, const double *rays, size_t n, double *radiance, const FilmArgs *film, const DLightGroup *groups, uint32_t n_groups,
                              const uint32_t *perm, const char *label, lg_accel::LaunchCtx &c, hipStream_t stream, const std::function<void()> &tail = nullptr) {
    Level0Call call;
    call.tiles = (uint32_t)((n + 63) / 64);
    call.label = label;
    call.note = perm ? "sorted order" : "as given";
    const RadianceArgs Q{rays, radiance, perm, (unsigned long long)n, 0ull};
    if (groups) {
        call.planes = n_groups;
        call.note += ", " + std::to_string(n_groups) + " groups";
        GroupArgs GA;
        std::memset(&GA, 0, sizeof GA);
        static_cast<RadianceArgs &>(GA) = Q;
        GA.n_groups = n_groups;
        std::memcpy(GA.groups, groups, n_groups * sizeof(DLightGroup));
        enqueue_level0_query(a, call, [&](unsigned long long t0) {
            GA.base = t0 * 64ull;
            Level0 l0 = bind_level0<GroupArgs, launch_lg_closest, launch_lg_shade, launch_lg_combine>(GA);
            l0.lg = &GA;
            return l0;
        }, c, stream, tail);
    } else if (film) {
        FilmArgs F = *film;
        static_cast<RadianceArgs &>(F) = Q;
        enqueue_level0_query(a, call, [&](unsigned long long t0) {
            F.base = t0 * 64ull;
            return bind_level0<FilmArgs, launch_rf_closest, launch_rf_shade, launch_rf_combine>(F);
        }, c, stream, tail);
    } else {
        RadianceArgs R = Q;
        enqueue_level0_query(a, call, [&](unsigned long long t0) {
            R.base = t0 * 64ull;
            return bind_level0<RadianceArgs, launch_rq_closest, launch_rq_shade, launch_rq_combine>(R);
        }, c, stream, tail);
    }
}
void enqueue_radiance(const lg_accel &a, const double *rays, size_t n, double *radiance, const uint32_t *perm, lg_accel::LaunchCtx &c, hipStream_t stream) {
    enqueue_ray_query(a, rays, n, radiance, nullptr, nullptr, 0, perm, "radiance query", c, stream);
}
// Light groups (query.cpp, lg_radiance_groups*; the call checked there and in light_groups_host.h): the same query with n_groups planes of li
// per ray at every level -- the chunk carries planes 1 .. G-1 beside the level arrays, and the chain takes the shade and combine passes of
// every level, and a spread pass at the deepest, from k_light_groups.hip (Level0::lg).  The walks are the radiance query's.
void enqueue_radiance_groups(const lg_accel &a, const double *rays, size_t n, const DLightGroup *groups, uint32_t n_groups, double *radiance, const uint32_t *perm,
                             lg_accel::LaunchCtx &c, hipStream_t stream) {
    enqueue_ray_query(a, rays, n, radiance, nullptr, groups, n_groups, perm, "radiance groups", c, stream);
}
// Surface scatter (query.cpp, lg_scatter*; the call checked there and in scatter_host.h): the same rays as level 0's source of a chain of ONE
// level (Level0Call::one_level) whatever the scene's depth -- the closest pass and, in the shade pass's place, the emit pass are
// k_scatter.hip's, the shadow pass between them is the render's.  The chunks are the pipeline's own: a chunk parks the hit queue, the frame
// and the visibility words of its rays; the planes are the caller's, indexed by the ray.  With one level there is no combine pass to bind.
void enqueue_scatter(const lg_accel &a, const double *rays, size_t n, ScatterArgs Q, const uint32_t *perm, lg_accel::LaunchCtx &c, hipStream_t stream) {
    Level0Call call;
    call.tiles = (uint32_t)((n + 63) / 64);
    call.label = "surface scatter";
    call.note = perm ? "sorted order" : "as given";
    call.one_level = true;
    static_cast<RadianceArgs &>(Q) = RadianceArgs{rays, nullptr, perm, (unsigned long long)n, 0ull};
    Q.tri_base = a.accel_tri_base.p;
    enqueue_level0_query(a, call, [&](unsigned long long t0) {
        Q.base = t0 * 64ull;
        Level0 l0;
        l0.q = &Q;
        l0.closest_ = l0_closest<ScatterArgs, launch_scatter_closest>;
        l0.shade_ = l0_flat<ScatterArgs, launch_scatter_emit>;
        return l0;
    }, c, stream);
}
// Lit scatter (query.cpp, lg_scatter_lit*; the call checked there and in lit_host.h): surface scatter's chain with all three passes
// k_lit.hip's -- the shadow pass between the closest and the emit pass walks the CALL's lights (Level0::own_shadow: the render's shadow pass
// is not launched, whatever lights the scene has; a call without lights launches none).  Q.lights is device memory: a per-ray table is the
// caller's, a shared one is staged here from the host array `shared` (which may be freed on return).  A chunk parks Q.vis_words visibility
// words per hit slot.
void enqueue_scatter_lit(const lg_accel &a, const double *rays, size_t n, LitArgs Q, const DLight *shared, const uint32_t *perm, lg_accel::LaunchCtx &c, hipStream_t stream) {
    try {
        if (!Q.per_ray && Q.n_lights) Q.lights = static_cast<const DLight *>(stage_rule_table(shared, (size_t)Q.n_lights * sizeof(DLight), c, stream));
        Level0Call call;
        call.tiles = (uint32_t)((n + 63) / 64);
        call.label = "lit scatter";
        call.note = std::string(perm ? "sorted order" : "as given") + ", " + std::to_string(Q.n_lights) + (Q.per_ray ? " lights per ray" : " shared lights") + (Q.skip ? ", skip" : "");
        call.one_level = true;
        call.vis_words = std::max(1u, Q.vis_words);
        static_cast<RadianceArgs &>(Q) = RadianceArgs{rays, nullptr, perm, (unsigned long long)n, 0ull};
        Q.tri_base = a.accel_tri_base.p;
        enqueue_level0_query(a, call, [&](unsigned long long t0) {
            Q.base = t0 * 64ull;
            Level0 l0;
            l0.q = &Q;
            l0.closest_ = l0_closest<LitArgs, launch_lit_closest>;
            l0.shade_ = l0_flat<LitArgs, launch_lit_emit>;
            l0.own_shadow = true;
            if (Q.n_lights) l0.shadow_ = l0_closest<LitArgs, launch_lit_shadow>;
            l0.vis_words = call.vis_words;
            return l0;
        }, c, stream);
        subsets_enqueued(a, stream);
    } catch (...) { subsets_abandoned(a, stream); throw; }
}
// A radiance gather (query.cpp, lg_radiance_gather*; the call checked there and in gather_host.h): batch after batch of g.batch_poses whole
// consecutive poses, each a level-0 query of its own over the batch's tiles -- its poses' rows of the tables, its own li -- with the
// reduction (k_gather.hip, gather_resolve_kernel; credited to lg_profile_read_kinds as a combine pass, kind 1, as a film's resolve is) as
// its tail where sums is asked for.  li is the caller's radiance plane (then the call is ONE batch) or the context's gather_li, which the
// next batch overwrites: the stream orders a batch's reduction ahead of the next batch's level 0.  Growing gather_li is the one step that
// is more than an enqueue (a device-wide synchronise first, as for the level arrays).  A sum never crosses a pose, so the batches cannot
// change a bit.
void enqueue_radiance_gather(const lg_accel &a, const GatherCall &g, lg_accel::LaunchCtx &c, hipStream_t stream) {
    const size_t batch_poses = std::min(g.batch_poses, g.n_poses);
    const size_t nbatches = (g.n_poses + batch_poses - 1) / batch_poses;
    if (!g.radiance) grow(c.gather_li, batch_poses * g.n_dirs * 3);
    for (size_t p0 = 0, batch = 0; p0 < g.n_poses; p0 += batch_poses, ++batch) {
        const size_t np = std::min(batch_poses, g.n_poses - p0);
        double *li = g.radiance ? g.radiance + 3 * (p0 * g.n_dirs) : c.gather_li.p;
        const uint32_t tiles_per = g.pose_lanes ? (uint32_t)g.n_dirs : (uint32_t)((g.n_dirs + 63) / 64);
        GatherArgs G{g.origins + 3 * p0, g.frames ? g.frames + 9 * p0 : nullptr, g.dirs, li, np, g.n_dirs, 0ull, tiles_per, g.pose_lanes ? 1u : 0u};
        Level0Call call;
        call.tiles = (uint32_t)((g.pose_lanes ? (np + 63) / 64 : np) * tiles_per); // (at most the call's tiles: 32 bits)
        call.label = "radiance gather";
        call.note = "batch " + std::to_string(batch + 1) + " of " + std::to_string(nbatches) + ", " + (g.pose_lanes ? "pose lanes" : "direction lanes");
        double *sums = g.sums ? g.sums + 3 * (p0 * g.n_weights) : nullptr;
        auto bind = [&](unsigned long long t0) {
            G.base_tile = t0;
            return bind_level0<GatherArgs, launch_gather_closest, launch_gather_shade, launch_gather_combine>(G);
        };
        enqueue_level0_query(a, call, bind, c, stream, [&] {
            if (!sums) return;
            const uint32_t blocks = (uint32_t)std::min<unsigned long long>(((unsigned long long)np * g.n_weights + 255ull) / 256ull, (unsigned long long)a.cus * 64ull);
            timed(a, 1, stream, [&] { return launch_gather_resolve(li, g.weights, sums, np, g.n_dirs, g.n_weights, blocks, stream); });
        });
    }
}
// A small host table on its way to the device for the launches a call enqueues next on `stream`: a buffer and pinned staging of its own in
// the stream's launch context, released once the event that subsets_enqueued() records behind those launches is through (a call that
// fails before that: subsets_abandoned()).  Tables whose launch is through go back to the pools here.
static lg_accel::LaunchCtx::KsTable &live_table(lg_accel::LaunchCtx &c) {
    for (size_t i = 0; i < c.ks_live.size();) {
        if (c.ks_live[i]->done && hipEventQuery(c.ks_live[i]->done) == hipSuccess) {
            (void)hipEventDestroy(c.ks_live[i]->done);
            c.ks_live.erase(c.ks_live.begin() + (long)i);
        } else ++i;
    }
    (void)hipGetLastError(); // (hipEventQuery's "not ready" is not an error of this call)
    c.ks_live.emplace_back(new lg_accel::LaunchCtx::KsTable());
    return *c.ks_live.back();
}
// The K view records of a call (lg_capture_views*, lg_capture_view_features*) from the caller's host array through pinned staging into a
// table of the call's own on the stream (live_table) -- so the call only enqueues and the caller's array may be freed when it returns.
// The caller ends with subsets_enqueued() behind its launches, or subsets_abandoned() where it fails before them.
const DView *stage_view_table(const DView *views, size_t n_views, lg_accel::LaunchCtx &c, hipStream_t stream) {
    static_assert(sizeof(DView) % sizeof(unsigned long long) == 0, "the table is staged as 64-bit words");
    const size_t bytes = n_views * sizeof(DView);
    lg_accel::LaunchCtx::KsTable &t = live_table(c);
    t.stage.need(bytes);
    std::memcpy(t.stage.p, views, bytes);
    t.buf.alloc(std::max<size_t>(bytes / sizeof(unsigned long long), 128));
    HIP_TRY(hipMemcpyAsync(t.buf.p, t.stage.p, bytes, hipMemcpyHostToDevice, stream));
    return reinterpret_cast<const DView *>(t.buf.p);
}
// ... and the rule table of a call (lg_trace_paths*), the same way: `bytes` of 64-bit words
const void *stage_rule_table(const void *rules, size_t bytes, lg_accel::LaunchCtx &c, hipStream_t stream) {
    lg_accel::LaunchCtx::KsTable &t = live_table(c);
    t.stage.need(std::max<size_t>(bytes, 8));
    std::memcpy(t.stage.p, rules, bytes);
    t.buf.alloc(std::max<size_t>(bytes / sizeof(unsigned long long), 128));
    if (bytes) HIP_TRY(hipMemcpyAsync(t.buf.p, t.stage.p, bytes, hipMemcpyHostToDevice, stream));
    return t.buf.p;
}
// A view batch (query.cpp, lg_capture_views*; the call checked there and in views_host.h): the table, then one level-0 query over the
// batch's pixel tiles.
void enqueue_view_batch(const lg_accel &a, const DView *views, ViewArgs V, uint32_t samples_root, lg_accel::LaunchCtx &c, hipStream_t stream) {
    try {
        V.views = stage_view_table(views, (size_t)V.n_views, c, stream);
        V.base_tile = 0;
        Level0Call call;
        call.tiles = (uint32_t)V.n_views * V.tiles_per_view; // (at most the call's work tiles: 32 bits)
        call.w = V.w; call.h = V.h;
        call.samples_root = samples_root;
        call.label = "view batch";
        call.note = std::to_string(V.n_views) + " views of " + std::to_string(V.tiles_per_view) + " tiles x " + std::to_string(samples_root * samples_root) + " samples";
        enqueue_level0_query(a, call, [&](unsigned long long t0) {
            V.base_tile = t0;
            Level0 l0 = bind_level0<ViewArgs, launch_view_closest, launch_view_shade, launch_view_combine>(V);
            if (samples_root > 1) l0.resolve_ = l0_flat<ViewArgs, launch_view_resolve>;
            return l0;
        }, c, stream);
        subsets_enqueued(a, stream);
    } catch (...) { subsets_abandoned(a, stream); throw; }
}
// A ray film (query.cpp, lg_capture_rays*): `slots` pixel slots of `samples` rays each, slot g's rays [g*samples, (g+1)*samples), into
// film.rgba / film.rgb at film.offsets[g] (or g).  One sample: the film forms of level 0 finish every ray where the radiance forms finish
// it, as its pixel.  Several: every ray's li is parked RAY-INDEXED in the context's film_li (24 bytes a ray; the radiance forms write it) --
// chunks are 64-ray tiles that a pixel's samples straddle (9 does not divide 64) and the sorted order scatters them, and neither
// matters to an array indexed by the ray --, then one resolve pass, a lane per slot, sums them in order (k_radiance.hip,
// rf_resolve_kernel; credited to lg_profile_read_kinds as a combine pass, kind 1, as the render's resolve is).  Growing film_li is the one
// step that is more than an enqueue (a device-wide synchronise first, as for the level arrays).
void enqueue_ray_film(const lg_accel &a, const double *rays, size_t slots, uint32_t samples, const FilmArgs &film, const uint32_t *perm, lg_accel::LaunchCtx &c,
                      hipStream_t stream) {
    const size_t n = slots * samples;
    if (samples == 1) { enqueue_ray_query(a, rays, n, nullptr, &film, nullptr, 0, perm, "ray film", c, stream); return; }
    grow(c.film_li, n * 3);
    const double *li = c.film_li.p;
    enqueue_ray_query(a, rays, n, c.film_li.p, nullptr, nullptr, 0, perm, "ray film", c, stream, [&] {
        const uint32_t blocks = (uint32_t)std::min<unsigned long long>(((unsigned long long)slots + 255ull) / 256ull, (unsigned long long)a.cus * 64ull);
        timed(a, 1, stream, [&] { return launch_rf_resolve(film, li, slots, samples, blocks, stream); });
    });
}

// The queue organisation (k_queue.hip): per chunk of the film and per supersample ONE persistent launch that runs every recursion
// level -- its waves pull 64-ray packets from per-level queues, deepest level first -- then the combine passes bottom-up, shared
// with the level-by-level pipeline.  A recursive scene may take a large share of the HBM for its worst-case capacities (a 4096^2
// frame at recursion 3: 26 GB of 288) and keeps ONE chunk in flight per launch context.
static void enqueue_queue(const lg_accel &a, DParams &P0, lg_accel::LaunchCtx &c, bool split, hipStream_t stream) {
    const uint32_t levels = levels_of(a, P0);
    const uint32_t nsamples = P0.ss_root * P0.ss_root;
    // level 0's tiles in parts (enqueue_mega, DParams::split_shift): the children's packets are then as narrow as their parents -- a small
    // launch's recursion chains are walked by four times the waves, 16 lanes each
    const auto [parts, split_shift] = tile_parts(a, split);
    const uint32_t S = (nsamples > 1 && a.sample_order != 1 ? nsamples : 1u) * parts; // samples side by side (enqueue_wavefront) x parts: level-0 tiles per pixel tile
    // (+ 1 byte per level-0 work item, as the organisation was first written: nothing is carved for it.  It stands in for the packets'
    // ready words, which live in wf_counters -- 4 bytes per 64-ray packet of the levels >= 1, 7/8 of a byte per item at four levels.)
    ChunkPlan plan(a, P0, true, S, 1);
    // level 0's work items: units of consecutive 8x8 tiles whose specular children the wave compacts into packets of its own.  Default
    // 1 (measured, config 4 / 4m in ms: 1 tile 39.0 / 16.4, 2: 40.0 / 17.0, 4: 41.0 / 18.5, 8: 44.6 / 22.2, 16: 51.7 / 31.6 -- a mesh tile is a
    // millisecond of work, so longer units lengthen the launch's tail by more than fuller packets save); LASGUN_QUEUE_UNIT: A/B
    static const uint32_t unit_tiles = [] { const char *e = std::getenv("LASGUN_QUEUE_UNIT"); const int v = e ? std::atoi(e) : 0; return v >= 1 && v <= 64 ? (uint32_t)v : 1u; }();
    // LASGUN_QUEUE_ORDER=1 (A/B): 32 x 32-tile blocks in Morton order, claimed XCD by XCD -- measured no better than row order with one
    // claim counter (config 4 / 4m / 5: 39.4 / 16.7 / 63.7 against 38.4 / 16.0 / 64.8 ms): which tiles are in flight together does not
    // move these kernels, as round 3 found for the other organisations
    static const bool order_blocks = [] { const char *e = std::getenv("LASGUN_QUEUE_ORDER"); return e && e[0] == '1'; }();
    const bool ldss = lds_resident(a); // (never in fast mode: org_possible rules the queue organisation out there, wherever one is picked)
    const uint32_t blocks_cap = ldss ? a.ldss_blocks : a.queue_blocks;
    const unsigned long long threads = (unsigned long long)blocks_cap * (ldss ? 1024ull : 256ull);
    // one word per packet of the levels >= 1, + slack per level
    auto nready = [&] { return (size_t)plan.chunk_tiles * S * ((1ull << levels) - 2ull) + (size_t)levels * QR_SLACK; };
    plan.fit([&] {
        grow(c.wf_mem, plan.need());
        grow(c.wf_counters, QC_WORDS + nready());
        if (P0.nlights > 0) grow(c.stash, (size_t)threads * STASH_DOUBLES);
    });
    const unsigned long long chunk_tiles = plan.chunk_tiles;
    const LevelArrays K = plan.carve(c.wf_mem.p, [](auto &) {});
    if (!a.q_err) a.q_err = g_err_words.take();
    Span span(a, stream);
    if (std::getenv("LASGUN_DEBUG"))
        std::fprintf(stderr, "[lasgun] queue: levels %u, %llu tiles in chunks of %llu (%.1f MiB), grid %u x %u, stack %u\n", levels,
                     (unsigned long long)P0.ntiles, chunk_tiles, plan.need() / 1048576.0, blocks_cap, ldss ? 1024u : 256u, a.stack_depth);
    for (unsigned long long t0 = 0; t0 < P0.ntiles; t0 += chunk_tiles) {
        DParams P = P0;
        P.tile0 = (uint32_t)t0;
        const uint32_t pixel_tiles = (uint32_t)std::min<unsigned long long>(chunk_tiles, P0.ntiles - t0);
        P.ntiles = pixel_tiles * S; // level 0's tiles
        P.ss_par = S / parts; P.split_shift = split_shift;
        P.n_items = plan.n0(); // SoA stride of level 0's arrays and of the sample accumulator
        P.accum = K.accum;
        P.wf_levels = levels;
        P.q_ctl = c.wf_counters.p; P.q_ready = c.wf_counters.p + QC_WORDS; P.q_err = a.q_err;
        P.q_unit_tiles = levels > 1 ? unit_tiles : 1u;
        // the tile sequence: rectangles whose chunk is whole tile rows go block by block, XCD by XCD (k_queue.hip, q_seq_tile)
        P.q_order = (order_blocks && !ldss && S == 1u && P.mode == 0u && P.tiles_x != 0u && t0 % P.tiles_x == 0u && P.ntiles % P.tiles_x == 0u) ? 1u : 0u;
        P.q_tiles_y = P.q_order ? P.ntiles / P.tiles_x : 0u;
        P.q_blocks_x = P.q_order ? (P.tiles_x + 31u) / 32u : 0u;
        P.q_seq_len = P.q_order ? P.q_blocks_x * ((P.q_tiles_y + 31u) / 32u) * 1024u : P.ntiles;
        P.q_units = (P.q_seq_len + P.q_unit_tiles - 1u) / P.q_unit_tiles;
        for (uint32_t d = 0; d < levels; ++d) { P.q_rays[d] = K.q[d]; P.q_out[d] = K.out[d]; P.q_spec[d] = K.spec[d]; P.q_child[d] = K.child[d]; }
        P.stash = c.stash.p; P.frame_threads = threads;
        if (ldss) set_lds_scene(a, P);
        const uint32_t blocks = ldss ? blocks_cap : std::min(blocks_cap, (P.q_units + 3u) / 4u);
        for (uint32_t sidx = 0; sidx < nsamples / (S / parts); ++sidx) {
            P.sample_index = sidx;
            HIP_TRY(hipMemsetAsync(c.wf_counters.p, 0, (QC_WORDS + (levels > 1 ? nready() : 0)) * sizeof(uint32_t), stream));
            timed(a, 4, stream, [&] { return launch_queue(P, blocks, stream); });
            combine_levels(a, P, K, plan, stream);
        }
        if (S / parts > 1) resolve_samples(a, P, pixel_tiles, stream);
    }
    span.end(a.events);
}

// ---- which organisation renders a launch -----------------------------------------------------------------
// what each organisation can take: the queue organisation the reference traversal with <= 32 lights and <= 8 recursion levels, the
// level-by-level pipeline any scene with <= 32 lights; neither the counting variant
static bool org_possible(const lg_accel &a, const DParams &P, bool stats, Org org) {
    if (org == ORG_QUEUE) return !stats && !a.fast && P.nlights <= 32 && levels_of(a, P) <= QC_MAX_LEVELS;
    if (org == ORG_WAVEFRONT) return !stats && P.nlights <= 32 && P.recursion < 20;
    return true;
}
// The FITTED rule of rounds 2-4 (primitive count, glass / mirror, pixels per launch, samples per pixel): what a launch gets when
// nothing has been measured for its kind -- LASGUN_AUTOTUNE=0, or the first candidate the measurement below starts from.
//   * queue organisation: glass / mirror over a big mesh (long uneven walks, sparse deep levels), launches of 2^16 pixels and more;
//   * level by level, for a scene resident in LDS (round 4, once a launch no longer ended in 75-90 us of failed tile claims): glass /
//     mirror frames up to 2^20 pixels (Cornell glass 0.41 against 0.81 ms at 512^2, 0.99 / 1.18 at 1024^2, 1.81 / 1.64 at 1536^2), and
//     frames from 2^18 pixels of few primitives at one sample per pixel (README sphere 2.2 / 3.5 ms at 4096^2); and wherever node and
//     sphere tests dominate (>= 512 spheres / boxes) from 2^21 pixels;
//   * the megakernel otherwise (supersampled frames of small scenes: its 768-lane form is ahead at every size).
static Org org_by_rule(const lg_accel &a, const DParams &P, bool stats) {
    const unsigned long long items = (unsigned long long)P.ntiles * 64ull;
    if (org_possible(a, P, stats, ORG_QUEUE) && a.streaming && a.queue_default && items >= a.queue_min_items) return ORG_QUEUE;
    const bool resident = lds_resident(a), specular = a.flat.has_specular && P.recursion > 0;
    // (level 0's work items: with a pixel's samples side by side -- round 5 -- a 9-sample frame is nine times as wide as its film;
    // profiles/r05_ss_par.jsonl: Cornell glass at 9 spp goes level by level at 256^2 and in the megakernel from 512^2, like its
    // one-sample frames of nine times the pixels; simple.rs at 16 spp level by level at every size)
    const unsigned long long work = items * (a.sample_order != 1 ? (unsigned long long)P.ss_root * P.ss_root : 1ull);
    const bool small_specular = resident && specular && work <= a.specular_small_items;
    const bool light_scene = resident && !specular && !a.streaming_pays && (P.ss_root == 1u || a.sample_order != 1) && work >= (1ull << 18);
    if (a.streaming && org_possible(a, P, stats, ORG_WAVEFRONT) && (small_specular || light_scene || (a.streaming_pays && work >= a.streaming_min_items)))
        return ORG_WAVEFRONT;
    return ORG_MEGA;
}

// the megakernel (k_mega.hip): the whole of li() per lane
// The megakernel with a pixel's samples SIDE BY SIDE (DParams::ss_par, enqueue_wavefront): the launch hands out (tile, sample) pairs,
// so that a wave's share is 1 / samples of what it was and the launch's tail with it; the samples are parked (24 bytes each) and summed
// in their order by the resolve pass.  Measured (tools/ss_probe.py, profiles/r05_ss_par.jsonl): 4- and 9-sample frames of 256^2 .. 1024^2
// 1.2 - 10 x faster (a 512^2 film is one tile per wave of the grid: nine samples in a row on each, or nine times the tiles); frames of
// 1024^2 and more of a cheap scene 30-50 % SLOWER (nine times the claims on one head word, 8 ns each).  So: possible while the parked
// samples fit 1 GiB, the rule below where nothing is measured, and one more thing the measured choice times.
constexpr unsigned long long SS_PAR_WAVES = 8; // the rule: side by side below this many pixel tiles per wave of the grid (9 of 12 scenes faster at 1024^2, none at 2048^2)
static bool mega_par_possible(const DParams &P, bool stats) {
    const unsigned long long nsamples = (unsigned long long)P.ss_root * P.ss_root;
    return nsamples > 1 && !stats && (unsigned long long)P.ntiles * 64ull * nsamples * 24ull <= (1ull << 30);
}
// the waves of the megakernel's grid (its LDS-resident form: one 1024- or 768-lane workgroup per CU)
static unsigned long long mega_grid_waves(const lg_accel &a) {
    return lds_resident(a) ? (unsigned long long)a.ldss_blocks * (a.mega_narrow ? 12u : 16u) : (unsigned long long)(a.fast ? a.max_blocks_fast : a.max_blocks) * 4ull;
}
static bool mega_par_by_rule(const lg_accel &a, const DParams &P, bool stats) {
    if (!mega_par_possible(P, stats) || a.sample_order == 1) return false;
    if (a.sample_order == 0) return true;
    return P.ntiles < SS_PAR_WAVES * mega_grid_waves(a);
}
// A SMALL launch may hand its tiles out in QUARTERS (DParams::split_shift: 16 lanes of a tile per wave, four times the waves at work): a frame of
// fewer tiles than the grid has waves is as slow as its slowest tile's recursion tree, and a quarter of a tile is a shorter tree walked by
// fewer diverging lanes.  Measured (tools/split_probe.py, profiles/r05_ab_split.jsonl): the kitchen sink at 512^2 2.40 -> 1.73 ms, the
// 100k-triangle metal torus at 256^2 2.23 -> 1.82; cheap scenes and frames of 1024^2 and more lose (idle lanes are then lost throughput).
// One more candidate of the measured choice; never by rule.
static bool mega_split_possible(const lg_accel &a, const DParams &P, bool stats) {
    const unsigned long long work = (unsigned long long)P.ntiles * (mega_par_by_rule(a, P, stats) ? (unsigned long long)P.ss_root * P.ss_root : 1ull);
    return !stats && P.ntiles >= 2u && work <= 4ull * mega_grid_waves(a);
}
static void enqueue_mega(const lg_accel &a, DParams &P, lg_accel::LaunchCtx &c, bool par, bool split, bool stats, hipStream_t stream) {
    const uint32_t nsamples = P.ss_root * P.ss_root;
    par = par && mega_par_possible(P, stats);
    if (par) {
        const size_t n_items = (size_t)P.ntiles * 64ull * nsamples, need = n_items * 3 * 8;
        grow(c.wf_mem, need);
        P.accum = reinterpret_cast<double *>(c.wf_mem.p); P.n_items = n_items; P.ss_par = nsamples; P.ntiles *= nsamples;
    }
    const auto [parts, shift] = tile_parts(a, split);
    if (parts > 1u && !stats && (unsigned long long)P.ntiles * parts < (1ull << 31)) { P.split_shift = shift; P.ntiles *= parts; }
    uint32_t cap = a.fast ? a.max_blocks_fast : a.max_blocks;
    uint32_t blocks = (P.ntiles + 3u) / 4u;
    if (blocks > cap) blocks = cap;
    uint32_t maxb = a.max_blocks > a.max_blocks_fast ? a.max_blocks : a.max_blocks_fast;
    if (!stats && lds_resident(a)) { // scene tables resident in LDS: one 1024-lane workgroup per CU
        set_lds_scene(a, P);
        P.mega_lanes = a.mega_narrow ? 768u : 1024u; // (k_mega.hip: three waves per SIMD and 168 registers where shading weighs more than walking)
        blocks = a.ldss_blocks;
    }
    if (maxb < a.ldss_blocks * 4u) maxb = a.ldss_blocks * 4u; // per-lane slots below: 1024 lanes per LDS-scene workgroup
    const unsigned long long threads = (unsigned long long)maxb * 256ull;
    if (a.flat.has_specular && P.recursion > 0) { // Whitted frames: one slot per resident lane and recursion level, only for glass / mirror scenes
        grow(c.frames, (size_t)threads * P.recursion * FRAME_DOUBLES);
        P.frames = c.frames.p;
        P.frame_threads = threads;
    }
    if (P.nlights > 0) { // shading frame parked across the shadow traversals
        grow(c.stash, (size_t)threads * STASH_DOUBLES);
        P.stash = c.stash.p;
        P.frame_threads = threads;
    }
    if (stats) {
        P.stats = a.stats.p;
        HIP_TRY(hipMemsetAsync(a.stats.p, 0, sizeof(DStats), stream));
    }
    HIP_TRY(hipMemsetAsync(c.tile_counter.p, 0, TILE_COUNTER_WORDS * sizeof(uint32_t), stream));
    Span span(a, stream);
#ifdef LG_QIDLE // diagnostic build: the waves' start / exit times of this launch (k_mega.hip), read by lg_debug_stats
    if (!stats) { P.stats = a.stats.p; HIP_TRY(hipMemsetAsync(a.stats.p, 0, sizeof(DStats), stream)); }
#endif
    HIP_TRY(launch_trace(P, stats, a.fast, blocks, a.fast ? a.stack_depth_fast1 : a.stack_depth, stream));
    if (par) {
        DParams R = P;
        R.ntiles = (P.ntiles >> P.split_shift) / nsamples; R.tile_rev = 0u; R.split_shift = 0u;
        HIP_TRY(launch_wf_resolve(R, (uint32_t)(((unsigned long long)R.ntiles * 64ull + 255ull) / 256ull), stream));
    }
    span.end(a.events);
}
static void enqueue_choice(const lg_accel &a, DParams P, lg_accel::LaunchCtx &c, Choice ch, bool stats, hipStream_t stream) { // (P by value: an organisation fills in its own fields)
    P.tile_counter = c.tile_counter.p;
    P.tile_rev = ch.org != ORG_WAVEFRONT ? (uint32_t)ch.dir : 0u; // (the level-by-level passes are short and alike: one direction)
    if (ch.org == ORG_QUEUE) enqueue_queue(a, P, c, ch.split, stream);
    else if (ch.org == ORG_WAVEFRONT) enqueue_wavefront(a, P, c, stream);
    else enqueue_mega(a, P, c, !ch.serial, ch.split, stats, stream);
}

// The MEASURED choice (round 5; the rule above was a fit to eight scenes and wrong by 6-22 % on the first scene that was not among
// them; round 6: the table and the race live in tune.cpp, this file supplies the kind, the candidates and how one is launched).
// Every organisation renders the same bytes, so which one runs is a question of time alone, and the answer is taken from the clock: the
// second API call that launches a KIND in the process (the first gets the rule's choice at no cost) -- the scene's shape (table sizes,
// materials, lights, recursion, samples per pixel, traversal mode, LDS residency), the device, the launch's size class (log2 of its pixels)
// and addressing mode -- renders the launch with every CANDIDATE that can take it (a warm-up pass, then three timed passes over the
// candidates in turn, HIP events on the caller's stream, the HOST WAITING -- the one place where a *_device entry point blocks; never on a
// stream that is being captured), keeps the fastest (the rule's own choice unless another beats it by 1 %) and remembers it for
// the process: capture() rebuilds its accel for every frame (lib.rs:64), so the memory is keyed by the scene's shape, not by the accel.
// A candidate that cannot run (no memory for its buffers) drops out of the race instead of failing the caller's render.
// A candidate is an organisation and, for the megakernel and the queue organisation, the DIRECTION the launch's tiles are claimed in:
// a launch ends with the recursion trees of its last tiles, and whether the film's top or its bottom should come last is the scene's
// and the camera's business -- simple.rs at 9 spp and the metal torus gain 6-9 % from the bottom up, the glass torus loses 3 %
// (profiles/r05_ab_tile_order.jsonl); which tile is rendered when never changes a pixel.  (The kind does not know the camera: a
// direction measured for one view is kept for the next.)  The launch itself is then enqueued as usual; what the measurement rendered
// into the caller's film are the same pixels.  Overridden by lg_accel_set_streaming(0 / 2 / 3) and lg_accel_set_tile_order
// (lg_accel_last_organisation says what a launch ran as); LASGUN_AUTOTUNE=0 keeps the rule and the middle-out direction;
// lg_tune_export / lg_tune_import / lg_tune_clear read, pin and forget choices.
namespace {
using TuneKey = lg::tune::Key;
// the direction a launch's tiles are claimed in when nothing is measured (choice.h: DIR_DEFAULT unless lg_accel_set_tile_order says otherwise)
static int dir_unmeasured(const lg_accel &a, Org org) { return org == ORG_WAVEFRONT ? 0 : a.tile_order >= 0 ? a.tile_order : DIR_DEFAULT; }
// LASGUN_AUTOTUNE (tune.cpp: mode()): 0 = never measure (the fitted rule), 1 (default) = measure a kind at the second API CALL that
// launches it, 2 = at the first.  A program that renders one frame and exits (every example of the reference) gets the rule's choice at no
// cost -- timing seven candidates three times over costs 30-50 frames' worth; whatever renders a kind twice (an animation, the progressive
// front end's hundred subsets, a benchmark) is measured from then on.  What counts is the CALL, not the launch: one lg_capture of a big
// film launches its kind four times (row bands), lg_multi_* once per share of a device (round 5 counted launches and measured inside
// the first frame: ADVICE r5).
bool autotune_enabled() { return lg::tune::mode() != 0; }
// Which API call is running: bumped when a call enters the library from outside (CallScope in guarded(), lg_capture, lg_multi_*:
// calls nested in it, on this thread or on the threads it starts, belong to it).
std::atomic<uint64_t> g_call_serial{1};
std::atomic<int> g_call_depth{0};
} // namespace
CallScope::CallScope() { if (g_call_depth.fetch_add(1) == 0) g_call_serial.fetch_add(1); }
CallScope::~CallScope() { g_call_depth.fetch_sub(1); }
extern "C" void lg_internal_call_scope(int enter) { // (multi.cpp: one lg_multi_capture* is one call, whatever its shares launch)
    if (enter) { if (g_call_depth.fetch_add(1) == 0) g_call_serial.fetch_add(1); }
    else g_call_depth.fetch_sub(1);
}
static TuneKey tune_key(const lg_accel &a, const DParams &P) {
    const FlatScene &f = a.flat;
    const unsigned long long items = (unsigned long long)P.ntiles * 64ull;
    uint64_t cls = 0;
    while ((items >> cls) > 1ull) ++cls;
    TuneKey k{};
    k.v[0] = f.nodes.size(); k.v[1] = f.primref.size(); k.v[2] = f.spheres.size(); k.v[3] = f.cuboids.size(); k.v[4] = f.tri_v.size();
    k.v[5] = f.accels.size(); k.v[6] = ((uint64_t)f.max_stack << 32) | (uint64_t)f.lights.size();
    k.v[7] = ((uint64_t)P.recursion << 32) | ((uint64_t)P.ss_root << 8) | (f.has_specular ? 1u : 0u);
    k.v[8] = ((uint64_t)P.prune << 2) | (a.fast ? 2u : 0u) | (a.lds_scene && a.ldss_blocks ? 1u : 0u);
    {   // what the primitives are made of decides how many rays have children: two scenes of one shape (config 4's glass torus, 4m's metal one) are two kinds
        uint64_t hsh = 1469598103934665603ull;
        auto mix = [&hsh](const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { hsh ^= b[i]; hsh *= 1099511628211ull; } };
        for (const DMaterial &m : f.materials) mix(&m.kind, sizeof m.kind);
        for (const DAccel &A : f.accels) { mix(&A.material, sizeof A.material); mix(&A.flags, sizeof A.flags); }
        if (!f.sphere_mat.empty()) mix(f.sphere_mat.data(), f.sphere_mat.size() * sizeof f.sphere_mat[0]);
        if (!f.cuboid_mat.empty()) mix(f.cuboid_mat.data(), f.cuboid_mat.size() * sizeof f.cuboid_mat[0]);
        k.v[9] = hsh ^ ((uint64_t)a.device << 56);
    }
    k.v[10] = cls;
    k.v[11] = (P.mode == 0u ? 0u : 1u) | (a.tile_order >= 0 ? 2u + (uint64_t)a.tile_order : 0u) | ((uint64_t)(a.sample_order + 1) << 4) | ((uint64_t)(a.tile_parts + 1) << 8); // (a forced direction is a kind of its own: only the organisations race)
    return k;
}
// a remembered choice (measured here, or pinned by lg_tune_import for a kind this build may see differently) that the launch cannot take
// falls back to the rule's
static Choice rule_choice(const lg_accel &a, const DParams &P) {
    const Org rule = org_by_rule(a, P, false);
    return Choice{rule, P.ntiles < 2u ? 0 : dir_unmeasured(a, rule), rule == ORG_MEGA && !mega_par_by_rule(a, P, false), false};
}
static bool choice_possible(const lg_accel &a, const DParams &P, Choice ch) {
    if (ch.org < ORG_MEGA || ch.org > ORG_QUEUE || !org_possible(a, P, false, ch.org)) return false;
    if (ch.split && !mega_split_possible(a, P, false)) return false;
    if (ch.org == ORG_MEGA && !ch.serial && P.ss_root > 1 && !mega_par_possible(P, false)) return false;
    return true;
}
static Choice tuned_choice(const lg_accel &a, const DParams &P, lg_accel::LaunchCtx &c, hipStream_t stream) {
    const Org rule = org_by_rule(a, P, false);
    const TuneKey key = tune_key(a, P);
    int known;
    if (lg::tune::lookup(key, &known)) return choice_possible(a, P, decode(known)) ? decode(known) : rule_choice(a, P);
    if (lg::tune::mode() == 1 && lg::tune::first_call_of_kind(key, g_call_serial.load())) return rule_choice(a, P); // the first call that launches the kind: the rule's choice, at no cost
    {   // a stream that is being captured into a graph cannot be waited on: no race there (the next plain launch of the kind measures)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) != hipSuccess) (void)hipGetLastError();
        else if (cs != hipStreamCaptureStatusNone) return rule_choice(a, P);
    }
    // the candidates (choice.h) and which of them can take this launch
    Choice slot[RACE_SLOTS];
    race_slots(!mega_par_by_rule(a, P, false), slot);
    lg::tune::Candidate cand[RACE_SLOTS];
    const unsigned long long items = (unsigned long long)P.ntiles * 64ull;
    const bool par = mega_par_possible(P, false);
    for (int k = 0; k < RACE_SLOTS; ++k) {
        const Choice s = slot[k];
        cand[k].choice = encode(s);
        // (tiles in parts: a small launch with nothing forced by lg_accel_set_tile_parts or lg_accel_set_tile_order; the queue organisation where it is possible, from 4096 pixels)
        cand[k].in_race = s.split
            ? (s.org == ORG_MEGA || (org_possible(a, P, false, ORG_QUEUE) && items >= 4096ull)) && mega_split_possible(a, P, false) && a.tile_parts < 0 && (a.tile_order < 0 || a.tile_order == DIR_DEFAULT)
            : org_possible(a, P, false, s.org) &&
              (s.serial ? s.org == ORG_MEGA : (s.org != ORG_MEGA || par)) &&
              !(s.org == ORG_MEGA && par && a.sample_order >= 0 && (int)s.serial != a.sample_order) && // (lg_accel_set_sample_order) // (one form of the megakernel for a frame of one sample per pixel: the serial one)
              !(s.org == ORG_QUEUE && items < 4096ull && rule != ORG_QUEUE) && // (a persistent scheduler for a handful of tiles: never ahead)
              !(s.dir != 0 && (s.org == ORG_WAVEFRONT || P.ntiles < 2u)) &&      // (one direction for the level-by-level passes and for a single tile)
              (a.tile_order < 0 || s.org == ORG_WAVEFRONT || s.dir == a.tile_order); // (lg_accel_set_tile_order: only the organisations race)
    }
    float best_ms[RACE_SLOTS];
    for (float &m : best_ms) m = INFINITY;
    struct Restore { const lg_accel &a; bool was; ~Restore() { a.profiling = was; } } restore{a, a.profiling};
    a.profiling = false; // (the measurement's launches are not the caller's: lg_profile_read must not count them)
    // (LASGUN_TUNE_FAIL=<organisation 0..2>: test hook -- every candidate of that organisation throws in the race, as one whose buffers do not fit would)
    static const int fail_org = [] { const char *e = std::getenv("LASGUN_TUNE_FAIL"); return e && e[0] >= '0' && e[0] <= '2' ? e[0] - '0' : -1; }();
    const int raced = lg::tune::race(key, cand, RACE_SLOTS, slot_of(slot, rule_choice(a, P)), stream, [&](int k) {
        if ((int)slot[k].org == fail_org) throw Error("LASGUN_TUNE_FAIL: injected failure of a candidate");
        enqueue_choice(a, P, c, slot[k], false, stream);
    }, best_ms);
    check_queue_error(a);
    if (std::getenv("LASGUN_DEBUG")) {
        std::fprintf(stderr, "[lasgun] measured for %llu pixels (top-down / bottom-up / middle-out): megakernel %.3f / %.3f / %.3f ms (samples in a row: %.3f / %.3f / %.3f), level by level %.3f ms, queue %.3f / %.3f / %.3f ms -> choice %d (rule: %d)\n",
                     items, best_ms[0], best_ms[1], best_ms[2], best_ms[3], best_ms[4], best_ms[5], best_ms[6], best_ms[12], best_ms[13], best_ms[14], // (one sample per pixel: "in a row" is the megakernel)
                     raced, (int)rule);
        if (std::isfinite(best_ms[SLOT_MEGA_PARTS]) || std::isfinite(best_ms[SLOT_QUEUE_PARTS])) std::fprintf(stderr, "[lasgun]   (tiles in quarters: megakernel %.3f ms, queue %.3f ms)\n", best_ms[SLOT_MEGA_PARTS], best_ms[SLOT_QUEUE_PARTS]);
    }
    return choice_possible(a, P, decode(raced)) ? decode(raced) : rule_choice(a, P);
}

// Enqueue one render on `stream`.  Caller holds a.mtx.
void enqueue(const lg_accel &a, DParams &P, bool stats, hipStream_t stream) {
    if (P.ntiles == 0) return;
    check_queue_error(a); // (an earlier launch on a caller's stream that stalled: reported here at the latest)
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    Choice ch{ORG_MEGA, -1, !mega_par_by_rule(a, P, stats), false}; // (dir -1: dir_unmeasured, below; the megakernel's samples by the rule; tiles in parts only as measured)
    if (stats) ch.dir = 0;                                                                          // the counting variant
    else if (a.queue == 1) ch.org = org_possible(a, P, stats, ORG_QUEUE) ? ORG_QUEUE : org_by_rule(a, P, stats); // lg_accel_set_streaming(3)
    else if (!a.streaming) ch.org = ORG_MEGA;                                                       // lg_accel_set_streaming(0)
    else if (a.streaming_forced) ch.org = org_possible(a, P, stats, ORG_WAVEFRONT) ? ORG_WAVEFRONT : ORG_MEGA; // lg_accel_set_streaming(2)
    else if (a.queue == 0 || !autotune_enabled()) {                                                 // the fitted rule (queue ruled out by set_streaming(0 .. 2))
        ch.org = org_by_rule(a, P, stats);
        if (a.queue == 0 && ch.org == ORG_QUEUE) ch.org = ORG_MEGA;
    } else ch = tuned_choice(a, P, c, stream);
    if (ch.dir < 0) ch.dir = P.ntiles < 2u ? 0 : dir_unmeasured(a, ch.org);
    if (ch.org == ORG_WAVEFRONT) ch.dir = 0;
    // (what is reported: samples in a row only where the megakernel has several; parts also where lg_accel_set_tile_parts forces them, never for level by level)
    a.last_org = encode(Choice{ch.org, ch.dir, ch.org == ORG_MEGA && ch.serial && P.ss_root > 1, ch.org != ORG_WAVEFRONT && (ch.split || a.tile_parts > 1)});
    enqueue_choice(a, P, c, ch, stats, stream);
}

void set_rect(DParams &P, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    P.mode = 0; P.x0 = x0; P.y0 = y0; P.x1 = x1; P.y1 = y1;
    P.tiles_x = (x1 - x0 + 7u) / 8u;
    uint32_t tiles_y = (y1 - y0 + 7u) / 8u;
    P.ntiles = P.tiles_x * tiles_y;
    P.ilv_n = 1; P.ilv_r = 0; P.ilv_b = 1;
    P.out_x0 = 0; P.out_pitch = P.w;
}
// the row table of the lattice addressing for (w, h, n): made once per launch context and kept while the caller stays with that film and period
// (the progressive front end's hundred calls share it)
constexpr size_t MAX_ROW_TABLES = 4;
static const DRowTab *lattice_rows(const lg_accel &a, hipStream_t stream, uint32_t w, uint32_t h, unsigned long long n) {
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    using RowTable = lg_accel::LaunchCtx::RowTable;
    for (auto &r : c.rowtabs)
        if (r->w == w && r->h == h && r->n == n) { r->last_use = ++c.rowtab_clock; return r->buf.p; }
    RowTable *r = nullptr;
    if (c.rowtabs.size() < MAX_ROW_TABLES) {
        c.rowtabs.emplace_back(new RowTable());
        r = c.rowtabs.back().get();
    } else { // the least recently used table makes room: launches that read it are ahead of the new copy in stream order, unless its buffer must grow
        r = c.rowtabs[0].get();
        for (auto &x : c.rowtabs) if (x->last_use < r->last_use) r = x.get();
        if (r->up) HIP_TRY(hipEventSynchronize(r->up)); // (its staging is rewritten below)
        if (r->buf.n < h) HIP_TRY(hipStreamSynchronize(stream)); // (a buffer goes back to the pool only when nothing can still read it)
    }
    r->w = 0; r->h = 0; r->n = 0; // (not a table of anything until the copy below is enqueued)
    if (r->buf.n < h) r->buf.alloc(h);
    r->stage.need((size_t)h * sizeof(DRowTab));
    DRowTab *t = static_cast<DRowTab *>(r->stage.p);
    for (uint32_t y = 0; y < h; ++y) { const unsigned long long o = (unsigned long long)y * w; t[y] = DRowTab{(uint32_t)(o / n), (uint32_t)(o % n)}; }
    HIP_TRY(hipMemcpyAsync(r->buf.p, t, (size_t)h * sizeof(DRowTab), hipMemcpyHostToDevice, stream));
    if (!r->up) HIP_TRY(hipEventCreateWithFlags(&r->up, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(r->up, stream));
    r->w = w; r->h = h; r->n = n; r->last_use = ++c.rowtab_clock;
    return r->buf.p;
}
// LASGUN_SUBSET_LATTICE=0 (A/B): a strided subset and a batch of them are never tiled by lattice column (set_subset, set_subsets)
static bool subset_lattice() { static const bool on = env_on("LASGUN_SUBSET_LATTICE"); return on; }
// the pixels of the subset {k + i*n} of an `area`-pixel film (k < area, n > 0), without forming area - k + n - 1 (which wraps for n near SIZE_MAX)
unsigned long long subset_count(unsigned long long area, unsigned long long k, unsigned long long n) { return k < area ? 1ull + (area - 1ull - k) / n : 0ull; }
void set_subset(const lg_accel &a, hipStream_t stream, DParams &P, size_t k, size_t n, uint32_t w, uint32_t h) {
    unsigned long long area = (unsigned long long)w * h;
    P.mode = 1; P.sub_k = k; P.sub_n = n;
    P.sub_count = subset_count(area, k, n);
    P.ntiles = (uint32_t)((P.sub_count + 63ull) / 64ull);
    // The subset tile by lattice column (mode 4, shade.h: 64 rows x <= n pixels per tile instead of 64 consecutive i) where that is the denser
    // window: a period shorter than the film's width and longer than a tile's 64 pixels in a row would be.  LASGUN_SUBSET_LATTICE=0: never (A/B).
    const unsigned long long cols = (w + n - 1) / n, tiles4 = ((unsigned long long)h + 63ull) / 64ull * cols;
    if (subset_lattice() && P.sub_count != 0 && n >= 8 && n <= w && h >= 16 && area < (1ull << 32) && tiles4 < (1ull << 31) && tiles4 <= 2ull * P.ntiles + 8ull) {
        P.mode = 4; P.sub_cols = (uint32_t)cols; P.sub_rows = 64u; P.ntiles = (uint32_t)tiles4;
        P.sub_kk = (uint32_t)(k % n); P.sub_kdiv = (uint32_t)(k / n);
        P.sub_rowtab = lattice_rows(a, stream, w, h, n);
    }
}

SubsetBatch make_batch(const size_t *ks, size_t count, size_t n, uint32_t w, uint32_t h) {
    if (n == 0) throw Error("n must be > 0");
    if (count != 0 && !ks) throw Error("ks is NULL");
    const unsigned long long area = (unsigned long long)w * h;
    SubsetBatch b;
    b.n = n;
    for (size_t j = 0; j < count; ++j) if (ks[j] < area) b.ks.push_back(ks[j]); // (a subset that starts behind the film has no pixel: lib.rs:152)
    std::sort(b.ks.begin(), b.ks.end());
    b.ks.erase(std::unique(b.ks.begin(), b.ks.end()), b.ks.end());
    for (unsigned long long k : b.ks) b.periods = std::max(b.periods, subset_count(area, k, n));
    b.items = (unsigned long long)b.ks.size() * b.periods;
    if (b.items >= 0xFFFFFFFFull) throw Error("too many pixels for one batch of subsets (2^32 work items)");
    b.whole = b.ks.size() == n;
    for (size_t j = 0; b.whole && j < b.ks.size(); ++j) b.whole = b.ks[j] == j;
    return b;
}
// the batch as addressing mode 3 on `stream` (its k table lives in the stream's launch context).  Caller holds a.mtx.
void set_subsets(const lg_accel &a, DParams &P, const SubsetBatch &b, hipStream_t stream) {
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    // (a table whose launch was never enqueued -- the call failed between set_subsets and subsets_enqueued -- has no event to wait for:
    // subsets_abandoned() below takes it out again on that path)
    lg_accel::LaunchCtx::KsTable &t = live_table(c);
    const size_t m_ = b.ks.size();
    t.stage.need(2 * m_ * sizeof(unsigned long long));
    unsigned long long *tab = static_cast<unsigned long long *>(t.stage.p); // the m values of k, then (k mod n) | (k / n) << 32 of each (the lattice form, shade.h mode 5)
    for (size_t j = 0; j < m_; ++j) { tab[j] = b.ks[j]; tab[m_ + j] = (b.ks[j] % b.n) | ((b.ks[j] / b.n) << 32); }
    t.buf.alloc(std::max<size_t>(2 * m_, 128));
    HIP_TRY(hipMemcpyAsync(t.buf.p, tab, 2 * m_ * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    P.mode = 3; P.pixel_list = t.buf.p; P.sub_m = (uint32_t)b.ks.size(); P.sub_n = b.n; P.sub_k = 0; P.sub_count = b.items;
    P.ntiles = (uint32_t)((b.items + 63ull) / 64ull);
    // the batch tile by lattice column (mode 5, shade.h: 64 / m rows x <= n pixels per tile instead of 64 consecutive work items -- 64 / m
    // periods of one row) where that wastes few lanes; LASGUN_SUBSET_LATTICE=0: never (A/B)
    const unsigned long long m = b.ks.size(), rows = m != 0 && m <= 64 ? 64ull / m : 0ull, cols = (P.w + b.n - 1) / b.n;
    const unsigned long long tiles5 = rows ? ((unsigned long long)P.h + rows - 1ull) / rows * cols : ~0ull;
    if (subset_lattice() && rows >= 2 && b.n >= 8 && b.n <= P.w && (unsigned long long)P.w * P.h < (1ull << 32) && tiles5 < (1ull << 31) && tiles5 * 3ull <= (unsigned long long)P.ntiles * 4ull + 24ull) {
        P.mode = 5; P.sub_cols = (uint32_t)cols; P.sub_rows = (uint32_t)rows; P.ntiles = (uint32_t)tiles5;
        P.sub_rowtab = lattice_rows(a, stream, P.w, P.h, b.n);
    }
}
// ... and once the batch's launch is enqueued: the event that releases its table
void subsets_enqueued(const lg_accel &a, hipStream_t stream) {
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    if (c.ks_live.empty() || c.ks_live.back()->done) return;
    HIP_TRY(hipEventCreateWithFlags(&c.ks_live.back()->done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c.ks_live.back()->done, stream));
}

// ... and when the call fails before its launch is enqueued: the table set_subsets made has no launch that reads it and no event that
// would ever release it (the copy into it may still be in flight: the stream is drained first)
void subsets_abandoned(const lg_accel &a, hipStream_t stream) {
    for (auto &c : a.ctxs)
        if (c->key == stream && !c->ks_live.empty() && !c->ks_live.back()->done) {
            (void)hipStreamSynchronize(stream);
            (void)hipGetLastError();
            c->ks_live.pop_back();
        }
}
