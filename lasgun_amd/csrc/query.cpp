// lasgun_amd/csrc/query.cpp -- ray queries (include/lasgun_hip.h: lg_intersect*, lg_occluded*, lg_visibility*, lg_open_directions*, lg_range_scan*, lg_radiance*, lg_camera_rays*,
// lg_capture_features*, lg_accel_material, lg_accel_instance): the caller's buffers checked, then one launch of the query's kernel (k_query.hip;
// k_visibility.hip, k_directions.hip, k_scan.hip and k_features.hip for the structured queries) on the caller's stream, sized like
// the render's level-by-level traversal passes (launch.cpp, enqueue_wavefront) and walking in the accel's traversal mode -- or, for
// lg_radiance*, that pipeline itself with the caller's rays as its level 0 (launch.cpp, enqueue_radiance).  With
// lg_accel_set_query_order(1) the rays' keys and their sort (k_sort.hip) are enqueued ahead of it on the same stream, and the walk takes
// its tiles from the sorted order; lg_query_order* return that order.
#include <cstddef>

#include "features_host.h"
#include "scan_host.h"
#include "internal.h"

static_assert(sizeof(lg_hit) == 96 && offsetof(lg_hit, p) == 8 && offsetof(lg_hit, ng) == 32 && offsetof(lg_hit, ns) == 56 &&
                  offsetof(lg_hit, kind) == 80 && offsetof(lg_hit, prim) == 84 && offsetof(lg_hit, instance) == 88 && offsetof(lg_hit, material) == 92,
              "lg_hit: the layout k_query.hip writes (six 16-byte stores per hit)");
static_assert(sizeof(lg_material) == sizeof(Material), "lg_material wraps Material");

static constexpr unsigned long long MAX_RAYS = 0xFFFFFFFFull * 64ull; // 64-ray tiles are counted in 32 bits
static constexpr unsigned long long MAX_SORTED_RAYS = 0xFFFFFFFFull;  // the sorted order's indices are 32-bit
// A query of at most 64 rays is one wave's tile whatever the order: it is walked as given (the same bytes; lg_query_order* sort any n)
static constexpr size_t SORT_MIN_RAYS = 65;

// A caller's device buffer: not NULL, aligned, device memory of the accel's device, and `bytes` long within its allocation -- checked
// before anything is enqueued (a pageable host pointer or another device's memory would fault the card, not fail the call).
static void check_device_buffer(int device, const void *p, size_t bytes, size_t align, const char *what) {
    if (!p) throw Error(std::string(what) + " is NULL");
    if ((uintptr_t)p % align) throw Error(std::string(what) + " is not " + std::to_string(align) + "-byte aligned");
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        throw Error(std::string(what) + " is not device memory (hipPointerGetAttributes)");
    }
    if (at.type != hipMemoryTypeDevice) throw Error(std::string(what) + " is not device memory (hipPointerGetAttributes)");
    if (at.device != device) throw Error(std::string(what) + " lives on device " + std::to_string(at.device) + ", the accel on device " + std::to_string(device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) == hipSuccess) {
        if ((const char *)p + bytes > (const char *)base + size) throw Error(std::string(what) + " ends beyond its allocation");
    } else (void)hipGetLastError();
}
static void check_device_buffer(const lg_accel &a, const void *p, size_t bytes, size_t align, const char *what) { check_device_buffer(a.device, p, bytes, align, what); }

// The scene's world bounds for the key (raykey.h): the root accel's box, its corners taken to world space
static KeyBounds world_key_bounds(const lg_accel &a) {
    const FlatScene &f = a.flat;
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    if (!f.accels.empty() && f.accels[0].node_base < f.nodes.size()) {
        const DNode &root = f.nodes[f.accels[0].node_base];
        for (int c = 0; c < 8; ++c) {
            const V3 p = xf_point(f.accels[0].m, V3{(c & 1) ? root.bmax[0] : root.bmin[0], (c & 2) ? root.bmax[1] : root.bmin[1], (c & 4) ? root.bmax[2] : root.bmin[2]});
            const double q[3] = {p.x, p.y, p.z};
            for (int k = 0; k < 3; ++k) {
                lo[k] = c == 0 ? q[k] : std::fmin(lo[k], q[k]); // (fmin / fmax: a NaN corner of a degenerate scene is stepped over)
                hi[k] = c == 0 ? q[k] : std::fmax(hi[k], q[k]);
            }
        }
    }
    return key_bounds(lo, hi);
}
// The sorted order of `rays` enqueued on `stream`: the context's scratch grown if it has to be (the one step that is more than an enqueue:
// a device-wide synchronise and an allocation, once per stream and size), then key + sort.  Returns where the permutation will be.
static const uint32_t *enqueue_query_order(const lg_accel &a, lg_accel::LaunchCtx &c, const double *rays, size_t n, uint32_t *keys_out, uint32_t *perm_out,
                                           hipStream_t stream) {
    const size_t need = sort_scratch_bytes(n);
    if (c.sort_mem.n < need) { HIP_TRY(hipDeviceSynchronize()); c.sort_mem.alloc(need); }
    const uint32_t *perm = nullptr;
    HIP_TRY(launch_query_order(rays, n, world_key_bounds(a), c.sort_mem.p, keys_out, perm_out, &perm, a.cus * 8u, stream));
    return perm;
}

// ... for a query of `n` rays where the accel walks its queries in sorted order; nullptr: as given
static const uint32_t *query_order_of(const lg_accel &a, lg_accel::LaunchCtx &c, const double *rays, size_t n, hipStream_t stream) {
    return a.query_order == 1 && n >= SORT_MIN_RAYS ? enqueue_query_order(a, c, rays, n, nullptr, nullptr, stream) : nullptr;
}

// The grid of a tiled traversal launch of P.ntiles tiles, a wave each (k_query.hip, k_visibility.hip, k_features.hip), sized like the render's
// level-by-level traversal passes: the scene resident in LDS -> its tables into P and one 1024-lane workgroup per CU; otherwise as many
// 256-lane workgroups as the kernel family's `occupancy` lets a CU hold; never more workgroups than the tiles fill with waves.  P gets the
// context's tile counter, cleared on `stream` here.  `depth`: the stack depth the launcher is told.
struct TraversalGrid { uint32_t blocks, depth; };
static TraversalGrid traversal_grid(const lg_accel &a, DParams &P, hipError_t (*occupancy)(const DParams &, bool, uint32_t, int *), lg_accel::LaunchCtx &c,
                                    hipStream_t stream) {
    const bool ldss = !a.fast && a.lds_scene && a.ldss_blocks;
    const uint32_t depth = a.fast ? a.stack_depth_fast1 : a.stack_depth;
    uint32_t cap = a.ldss_blocks;
    if (ldss) set_lds_scene(a, P);
    else {
        int per_cu = 0;
        HIP_TRY(occupancy(P, a.fast, depth, &per_cu));
        cap = (uint32_t)(per_cu < 1 ? 1 : per_cu) * a.cus;
    }
    const uint32_t waves_per_block = (ldss ? 1024u : 256u) / 64u;
    P.tile_counter = c.tile_counter.p;
    HIP_TRY(hipMemsetAsync(c.tile_counter.p, 0, TILE_COUNTER_WORDS * sizeof(uint32_t), stream));
    return {std::max(1u, std::min(cap, (P.ntiles + waves_per_block - 1u) / waves_per_block)), depth};
}

// One query enqueued on `stream` (caller holds a.mtx and has made the accel's device current): hits != nullptr for closest hits,
// occluded != nullptr for the any-hit walk
static void enqueue_query(const lg_accel &a, const double *rays, size_t n, lg_hit *hits, uint8_t *occluded, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = (uint32_t)((n + 63) / 64);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const uint32_t *perm = query_order_of(a, c, rays, n, stream); // (ahead of the counter's memset on the stream)
    const TraversalGrid g = traversal_grid(a, P, query_occupancy, c, stream);
    HIP_TRY(launch_query(P, rays, n, hits, occluded, a.accel_tri_base.p, perm, a.fast, g.blocks, g.depth, stream));
}

static void check_sorted_count(const lg_accel &a, size_t n) {
    if (a.query_order == 1 && n > MAX_SORTED_RAYS) throw Error("too many rays in one query for the sorted order (lg_accel_set_query_order): at most 2^32 - 1");
}

// Both host forms: copy the rays in, enqueue on the accel's stream, copy the results out, synchronise (as lg_capture_pixels)
static int query_host(const lg_accel *a, const double *rays, size_t n, void *out, bool any) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (!rays) throw Error("rays is NULL");
        if (!out) throw Error(any ? "occluded is NULL" : "hits is NULL");
        if (n > MAX_RAYS) throw Error("too many rays in one query");
        const size_t out_bytes = n * (any ? 1u : sizeof(lg_hit));
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        use_device(a->device);
        DevBuf<double> drays;
        DevBuf<uint8_t> dout;
        drays.alloc(n * 6);
        dout.alloc(out_bytes);
        HIP_TRY(hipMemcpyAsync(drays.p, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        enqueue_query(*a, drays.p, n, any ? nullptr : reinterpret_cast<lg_hit *>(dout.p), any ? dout.p : nullptr, a->stream);
        HIP_TRY(hipMemcpyAsync(out, dout.p, out_bytes, hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
    });
}
static int query_device(const lg_accel *a, const double *dev_rays, size_t n, void *dev_out, bool any, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (n > MAX_RAYS) throw Error("too many rays in one query");
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        check_device_buffer(*a, dev_out, n * (any ? 1u : sizeof(lg_hit)), any ? 1 : 16, any ? "occluded" : "hits");
        enqueue_query(*a, dev_rays, n, any ? nullptr : reinterpret_cast<lg_hit *>(dev_out), any ? reinterpret_cast<uint8_t *>(dev_out) : nullptr,
                      (hipStream_t)hip_stream);
    });
}

// ---- visibility matrices (lg_visibility*; k_visibility.hip): the segments from[i] -> to[j] made in the kernel, one bit each
static size_t visibility_used_bytes(size_t n_to) { return n_to / 8 + (n_to % 8 ? 1 : 0); }
// What both forms refuse before anything is allocated or enqueued (counts are not 0 here)
static void check_visibility(const lg_accel *a, const double *from, size_t n_from, const double *to, size_t n_to, const uint8_t *bits, size_t row_bytes,
                             const uint32_t *blocked) {
    if (!a) throw Error("accel is NULL");
    if (!from) throw Error("from is NULL");
    if (!to) throw Error("to is NULL");
    if (!bits && !blocked) throw Error("bits and blocked are both NULL: at least one output");
    const size_t used = visibility_used_bytes(n_to);
    if (bits && row_bytes < used) throw Error("row_bytes is " + std::to_string(row_bytes) + ", a row of " + std::to_string(n_to) + " bits takes " + std::to_string(used));
    const unsigned long long ti = (unsigned long long)(n_from / 8 + (n_from % 8 ? 1 : 0));
    if (ti > 0xFFFFFFFFull / used) throw Error("too many segments in one visibility matrix: 8 x 8 blocks are counted in 32 bits");
    if (bits && n_from > 1 && row_bytes > (SIZE_MAX - used) / (n_from - 1)) throw Error("bits: n_from rows of row_bytes bytes do not fit the address space");
}
// One matrix enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked counts and buffers): a tile is
// an 8 x 8 block
static void enqueue_visibility(const lg_accel &a, const double *from, size_t n_from, const double *to, size_t n_to, uint8_t *bits, size_t row_bytes, uint32_t *blocked,
                               hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = (uint32_t)(((n_from + 7) / 8) * visibility_used_bytes(n_to));
    const TraversalGrid g = traversal_grid(a, P, visibility_occupancy, ctx_for(a, stream), stream);
    if (blocked) HIP_TRY(hipMemsetAsync(blocked, 0, n_from * sizeof(uint32_t), stream)); // written, not accumulated: the kernel adds to zero
    HIP_TRY(launch_visibility(P, from, n_from, to, n_to, bits, row_bytes, blocked, a.fast, g.blocks, g.depth, stream));
}
// Host form: the points go up, the rows come back COMPACT (ceil(n_to / 8) bytes each) and are placed into the caller's stride here -- the
// bytes of a row behind its used part are never written
extern "C" int lg_visibility(const lg_accel *a, const double *from, size_t n_from, const double *to, size_t n_to, uint8_t *bits, size_t row_bytes, uint32_t *blocked) {
    return guarded([&] {
        if (n_from == 0 || n_to == 0) return;
        check_visibility(a, from, n_from, to, n_to, bits, row_bytes, blocked);
        const size_t used = visibility_used_bytes(n_to);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        DevBuf<double> dfrom, dto;
        DevBuf<uint8_t> dbits;
        DevBuf<uint32_t> dblocked;
        dfrom.alloc(n_from * 3);
        dto.alloc(n_to * 3);
        if (bits) dbits.alloc(n_from * used);
        if (blocked) dblocked.alloc(n_from);
        std::vector<uint8_t> rows(bits && row_bytes != used ? n_from * used : 0);
        std::vector<uint32_t> counts(blocked ? n_from : 0); // (staged: an error on the way leaves the caller's array as it was)
        HIP_TRY(hipMemcpyAsync(dfrom.p, from, n_from * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipMemcpyAsync(dto.p, to, n_to * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        enqueue_visibility(*a, dfrom.p, n_from, dto.p, n_to, bits ? dbits.p : nullptr, used, blocked ? dblocked.p : nullptr, a->stream);
        if (bits) HIP_TRY(hipMemcpyAsync(row_bytes != used ? rows.data() : bits, dbits.p, n_from * used, hipMemcpyDeviceToHost, a->stream));
        if (blocked) HIP_TRY(hipMemcpyAsync(counts.data(), dblocked.p, n_from * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
        if (bits && row_bytes != used)
            for (size_t i = 0; i < n_from; ++i) std::memcpy(bits + i * row_bytes, rows.data() + i * used, used);
        if (blocked) std::memcpy(blocked, counts.data(), n_from * sizeof(uint32_t));
    });
}
extern "C" int lg_visibility_device(const lg_accel *a, const double *dev_from, size_t n_from, const double *dev_to, size_t n_to, uint8_t *dev_bits, size_t row_bytes,
                             uint32_t *dev_blocked, void *hip_stream) {
    return guarded([&] {
        if (n_from == 0 || n_to == 0) return;
        check_visibility(a, dev_from, n_from, dev_to, n_to, dev_bits, row_bytes, dev_blocked);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        check_device_buffer(*a, dev_from, n_from * 3 * sizeof(double), 8, "from");
        check_device_buffer(*a, dev_to, n_to * 3 * sizeof(double), 8, "to");
        if (dev_bits) check_device_buffer(*a, dev_bits, (n_from - 1) * row_bytes + visibility_used_bytes(n_to), 1, "bits");
        if (dev_blocked) check_device_buffer(*a, dev_blocked, n_from * sizeof(uint32_t), 4, "blocked");
        enqueue_visibility(*a, dev_from, n_from, dev_to, n_to, dev_bits, row_bytes, dev_blocked, (hipStream_t)hip_stream);
    });
}

// ---- direction sets (lg_open_directions*; k_directions.hip): the rays (points[i], dirs[k]) made in the kernel, one bit each, walked only
// where the direction is above the point's horizon
// What both forms refuse before anything is allocated or enqueued (counts are not 0 here)
static void check_open_directions(const lg_accel *a, const double *points, size_t n_points, const double *dirs, size_t n_dirs, const uint8_t *bits, size_t row_bytes,
                                  const uint32_t *open, const uint32_t *above) {
    if (!a) throw Error("accel is NULL");
    if (!points) throw Error("points is NULL");
    if (!dirs) throw Error("dirs is NULL");
    if (!bits && !open && !above) throw Error("bits, open and above are all NULL: at least one output");
    if ((unsigned long long)n_dirs > 0xFFFFFFFFull) throw Error("too many directions in one set: at most 2^32 - 1 (tiles of 64 points x 8 directions are counted in 32 bits)");
    const size_t used = visibility_used_bytes(n_dirs);
    if (bits && row_bytes < used) throw Error("row_bytes is " + std::to_string(row_bytes) + ", a row of " + std::to_string(n_dirs) + " bits takes " + std::to_string(used));
    const unsigned long long pb = (unsigned long long)(n_points / 64 + (n_points % 64 ? 1 : 0));
    if (pb > 0xFFFFFFFFull / used) throw Error("too many pairs in one direction set: tiles of 64 points x 8 directions are counted in 32 bits");
    if (bits && n_points > 1 && row_bytes > (SIZE_MAX - used) / (n_points - 1)) throw Error("bits: n_points rows of row_bytes bytes do not fit the address space");
}
// One direction set enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked counts and buffers): a
// tile is 64 points x 8 directions
static void enqueue_open_directions(const lg_accel &a, const double *points, const double *normals, size_t n_points, const double *dirs, size_t n_dirs, uint8_t *bits,
                                    size_t row_bytes, uint32_t *open, uint32_t *above, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = (uint32_t)(((n_points + 63) / 64) * visibility_used_bytes(n_dirs));
    const TraversalGrid g = traversal_grid(a, P, open_directions_occupancy, ctx_for(a, stream), stream);
    if (open) HIP_TRY(hipMemsetAsync(open, 0, n_points * sizeof(uint32_t), stream)); // written, not accumulated: the kernel adds to zero
    if (above) HIP_TRY(hipMemsetAsync(above, 0, n_points * sizeof(uint32_t), stream));
    HIP_TRY(launch_open_directions(P, points, normals, n_points, dirs, n_dirs, bits, row_bytes, open, above, a.fast, g.blocks, g.depth, stream));
}
// Host form: the tables go up, the rows come back COMPACT (ceil(n_dirs / 8) bytes each) and are placed into the caller's stride here -- the
// bytes of a row behind its used part are never written; rows and counts are staged
extern "C" int lg_open_directions(const lg_accel *a, const double *points, const double *normals, size_t n_points, const double *dirs, size_t n_dirs, uint8_t *bits,
                                  size_t row_bytes, uint32_t *open, uint32_t *above) {
    return guarded([&] {
        if (n_points == 0 || n_dirs == 0) return;
        check_open_directions(a, points, n_points, dirs, n_dirs, bits, row_bytes, open, above);
        const size_t used = visibility_used_bytes(n_dirs);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        DevBuf<double> dpoints, dnormals, ddirs;
        DevBuf<uint8_t> dbits;
        DevBuf<uint32_t> dopen, dabove;
        dpoints.alloc(n_points * 3);
        if (normals) dnormals.alloc(n_points * 3);
        ddirs.alloc(n_dirs * 3);
        if (bits) dbits.alloc(n_points * used);
        if (open) dopen.alloc(n_points);
        if (above) dabove.alloc(n_points);
        std::vector<uint8_t> rows(bits ? n_points * used : 0); // (staged like the counts: an error on the way leaves the caller's arrays as they were)
        std::vector<uint32_t> nopen(open ? n_points : 0), nabove(above ? n_points : 0);
        HIP_TRY(hipMemcpyAsync(dpoints.p, points, n_points * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        if (normals) HIP_TRY(hipMemcpyAsync(dnormals.p, normals, n_points * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipMemcpyAsync(ddirs.p, dirs, n_dirs * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        enqueue_open_directions(*a, dpoints.p, normals ? dnormals.p : nullptr, n_points, ddirs.p, n_dirs, bits ? dbits.p : nullptr, used, open ? dopen.p : nullptr,
                                above ? dabove.p : nullptr, a->stream);
        if (bits) HIP_TRY(hipMemcpyAsync(rows.data(), dbits.p, n_points * used, hipMemcpyDeviceToHost, a->stream));
        if (open) HIP_TRY(hipMemcpyAsync(nopen.data(), dopen.p, n_points * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        if (above) HIP_TRY(hipMemcpyAsync(nabove.data(), dabove.p, n_points * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
        if (bits)
            for (size_t i = 0; i < n_points; ++i) std::memcpy(bits + i * row_bytes, rows.data() + i * used, used);
        if (open) std::memcpy(open, nopen.data(), n_points * sizeof(uint32_t));
        if (above) std::memcpy(above, nabove.data(), n_points * sizeof(uint32_t));
    });
}
extern "C" int lg_open_directions_device(const lg_accel *a, const double *dev_points, const double *dev_normals, size_t n_points, const double *dev_dirs, size_t n_dirs,
                                         uint8_t *dev_bits, size_t row_bytes, uint32_t *dev_open, uint32_t *dev_above, void *hip_stream) {
    return guarded([&] {
        if (n_points == 0 || n_dirs == 0) return;
        check_open_directions(a, dev_points, n_points, dev_dirs, n_dirs, dev_bits, row_bytes, dev_open, dev_above);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        check_device_buffer(*a, dev_points, n_points * 3 * sizeof(double), 8, "points");
        if (dev_normals) check_device_buffer(*a, dev_normals, n_points * 3 * sizeof(double), 8, "normals");
        check_device_buffer(*a, dev_dirs, n_dirs * 3 * sizeof(double), 8, "dirs");
        if (dev_bits) check_device_buffer(*a, dev_bits, (n_points - 1) * row_bytes + visibility_used_bytes(n_dirs), 1, "bits");
        if (dev_open) check_device_buffer(*a, dev_open, n_points * sizeof(uint32_t), 4, "open");
        if (dev_above) check_device_buffer(*a, dev_above, n_points * sizeof(uint32_t), 4, "above");
        enqueue_open_directions(*a, dev_points, dev_normals, n_points, dev_dirs, n_dirs, dev_bits, row_bytes, dev_open, dev_above, (hipStream_t)hip_stream);
    });
}

// ---- range scans (lg_range_scan*; k_scan.hip): the rays (origins[i], frames[i] * beams[k]) made in the kernel, their first hits written
// as planes and reduced per pose.  The arithmetic that needs no device -- the lane rule, the tile counts, the sizes, the NULL and
// alignment rules, the staging -- is scan_host.h's.
extern "C" int lg_range_scan_lanes(size_t n_poses, size_t n_beams, int lanes) { return scan_lanes(n_poses, n_beams, lanes); }
// One scan enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked counts and buffers): the two
// pre-fills, then the kernel in the shape's form
static void enqueue_range_scan(const lg_accel &a, const double *origins, const double *frames, size_t n_poses, const double *beams, size_t n_beams, const ScanShape &shape,
                               const lg_scan_out &out, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = shape.tiles;
    const TraversalGrid g = traversal_grid(a, P, range_scan_occupancy, ctx_for(a, stream), stream);
    if (out.hits) HIP_TRY(hipMemsetAsync(out.hits, 0, n_poses * sizeof(uint32_t), stream)); // written, not accumulated: the kernel adds to zero
    if (out.nearest) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)out.nearest, 0x7F800000, n_poses, stream)); // ... and takes minima below +INF
    HIP_TRY(launch_range_scan(P, origins, frames, n_poses, beams, n_beams, shape.form == SCAN_POSE_LANES, out.range, out.point, out.normal, out.id, out.hits,
                              reinterpret_cast<uint32_t *>(out.nearest), a.accel_tri_base.p, a.fast, g.blocks, g.depth, stream));
}
// Host form: the tables go up, the planes come back into staging and are copied out at the end
extern "C" int lg_range_scan(const lg_accel *a, const double *origins, const double *frames, size_t n_poses, const double *beams, size_t n_beams, int lanes,
                             const lg_scan_out *out) {
    return guarded([&] {
        if (n_poses == 0 || n_beams == 0) return;
        const ScanShape shape = check_scan(a, origins, n_poses, beams, n_beams, lanes, out);
        const size_t pairs = shape.pairs;
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        ScanStaging st(*out, n_poses, pairs);
        DevBuf<double> dorigins, dframes, dbeams;
        DevBuf<float> drange, dpoint, dnormal, dnearest;
        DevBuf<uint32_t> did, dhits;
        lg_scan_out dev{};
        dorigins.alloc(n_poses * 3);
        if (frames) dframes.alloc(n_poses * 9);
        dbeams.alloc(n_beams * 3);
        if (out->range) { drange.alloc(pairs); dev.range = drange.p; }
        if (out->point) { dpoint.alloc(pairs * 3); dev.point = dpoint.p; }
        if (out->normal) { dnormal.alloc(pairs * 3); dev.normal = dnormal.p; }
        if (out->id) { did.alloc(pairs * 4); dev.id = did.p; }
        if (out->hits) { dhits.alloc(n_poses); dev.hits = dhits.p; }
        if (out->nearest) { dnearest.alloc(n_poses); dev.nearest = dnearest.p; }
        HIP_TRY(hipMemcpyAsync(dorigins.p, origins, n_poses * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        if (frames) HIP_TRY(hipMemcpyAsync(dframes.p, frames, n_poses * 9 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipMemcpyAsync(dbeams.p, beams, n_beams * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        enqueue_range_scan(*a, dorigins.p, frames ? dframes.p : nullptr, n_poses, dbeams.p, n_beams, shape, dev, a->stream);
        if (out->range) HIP_TRY(hipMemcpyAsync(st.range.data(), drange.p, pairs * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        if (out->point) HIP_TRY(hipMemcpyAsync(st.point.data(), dpoint.p, pairs * 3 * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        if (out->normal) HIP_TRY(hipMemcpyAsync(st.normal.data(), dnormal.p, pairs * 3 * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        if (out->id) HIP_TRY(hipMemcpyAsync(st.id.data(), did.p, pairs * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        if (out->hits) HIP_TRY(hipMemcpyAsync(st.hits.data(), dhits.p, n_poses * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        if (out->nearest) HIP_TRY(hipMemcpyAsync(st.nearest.data(), dnearest.p, n_poses * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
        place_scan(*out, st);
    });
}
extern "C" int lg_range_scan_device(const lg_accel *a, const double *dev_origins, const double *dev_frames, size_t n_poses, const double *dev_beams, size_t n_beams,
                                    int lanes, const lg_scan_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n_poses == 0 || n_beams == 0) return;
        const ScanShape shape = check_scan(a, dev_origins, n_poses, dev_beams, n_beams, lanes, dev_out);
        check_scan_alignment(dev_origins, dev_frames, dev_beams, *dev_out);
        const size_t pairs = shape.pairs;
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        check_device_buffer(*a, dev_origins, n_poses * 3 * sizeof(double), 8, "origins");
        if (dev_frames) check_device_buffer(*a, dev_frames, n_poses * 9 * sizeof(double), 8, "frames");
        check_device_buffer(*a, dev_beams, n_beams * 3 * sizeof(double), 8, "beams");
        if (dev_out->range) check_device_buffer(*a, dev_out->range, pairs * sizeof(float), 4, "range");
        if (dev_out->point) check_device_buffer(*a, dev_out->point, pairs * 3 * sizeof(float), 4, "point");
        if (dev_out->normal) check_device_buffer(*a, dev_out->normal, pairs * 3 * sizeof(float), 4, "normal");
        if (dev_out->id) check_device_buffer(*a, dev_out->id, pairs * 4 * sizeof(uint32_t), 16, "id");
        if (dev_out->hits) check_device_buffer(*a, dev_out->hits, n_poses * sizeof(uint32_t), 4, "hits");
        if (dev_out->nearest) check_device_buffer(*a, dev_out->nearest, n_poses * sizeof(float), 4, "nearest");
        enqueue_range_scan(*a, dev_origins, dev_frames, n_poses, dev_beams, n_beams, shape, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- radiance queries: li() of the caller's rays through the level-by-level pipeline (launch.cpp, enqueue_radiance; k_radiance.hip)
// What the pipeline cannot take is refused before anything is enqueued: its visibility word holds 32 lights (as for a render, which then
// runs as the megakernel -- a query has no other organisation)
static void radiance_possible(const lg_accel &a) {
    const size_t nlights = a.flat.lights.size();
    if (nlights > 32) throw Error("radiance query: the scene has " + std::to_string(nlights) + " lights, the level-by-level pipeline's visibility word holds 32");
    if (a.scene->recursion >= 20) throw Error("radiance query: recursion depth " + std::to_string(a.scene->recursion) + ", the level-by-level pipeline takes fewer than 20");
}
// One query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the count and the buffers)
static void enqueue_radiance_query(const lg_accel &a, const double *rays, size_t n, double *radiance, hipStream_t stream) {
    check_queue_error(a);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const uint32_t *perm = query_order_of(a, c, rays, n, stream);
    enqueue_radiance(a, rays, n, radiance, perm, c, stream);
}
extern "C" int lg_radiance(const lg_accel *a, const double *rays, size_t n, double *radiance) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (!rays) throw Error("rays is NULL");
        if (!radiance) throw Error("radiance is NULL");
        if (n > MAX_RAYS) throw Error("too many rays in one query");
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        radiance_possible(*a);
        use_device(a->device);
        DevBuf<double> drays, dout;
        drays.alloc(n * 6);
        dout.alloc(n * 3);
        HIP_TRY(hipMemcpyAsync(drays.p, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        enqueue_radiance_query(*a, drays.p, n, dout.p, a->stream);
        HIP_TRY(hipMemcpyAsync(radiance, dout.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
    });
}
extern "C" int lg_radiance_device(const lg_accel *a, const double *dev_rays, size_t n, double *dev_radiance, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (n > MAX_RAYS) throw Error("too many rays in one query");
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        radiance_possible(*a);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        check_device_buffer(*a, dev_radiance, n * 3 * sizeof(double), 8, "radiance");
        enqueue_radiance_query(*a, dev_rays, n, dev_radiance, (hipStream_t)hip_stream);
    });
}

// ---- ray films: a film from the caller's rays (lg_capture_rays*; launch.cpp, enqueue_ray_film; k_radiance.hip, the film forms)
// pixels * samples as a ray count lg_radiance accepts
static size_t film_ray_count(const lg_accel &a, size_t pixels, uint32_t samples) {
    if (samples == 0) throw Error("samples is 0: a pixel slot has at least one ray");
    if (pixels > MAX_RAYS / samples) throw Error("too many rays in one query (pixels * samples)");
    const size_t n = pixels * (size_t)samples;
    check_sorted_count(a, n);
    return n;
}
// One film query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the counts and the buffers)
static void enqueue_film_query(const lg_accel &a, const double *rays, size_t pixels, uint32_t samples, const unsigned long long *offsets, unsigned long long npix,
                               uint32_t *rgba, double *rgb, hipStream_t stream) {
    check_queue_error(a);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const size_t n = pixels * (size_t)samples;
    const uint32_t *perm = query_order_of(a, c, rays, n, stream);
    FilmArgs F{};
    F.offsets = offsets; F.npix = npix; F.rgba = rgba; F.rgb = rgb;
    enqueue_ray_film(a, rays, pixels, samples, F, perm, c, stream);
}
// Host form: the rays go up, the slots' pixels come back COMPACT (slot g at g: pixels * 4 and / or pixels * 24 bytes, nothing else is
// copied) and are placed at their offsets here -- so a pixel no slot names is never touched, and a slot behind the film is dropped.
extern "C" int lg_capture_rays(const lg_accel *a, const double *rays, size_t pixels, uint32_t samples, const uint64_t *offsets, lg_film *film, double *rgb,
                             uint32_t w, uint32_t h) {
    return guarded([&] {
        if (pixels == 0) return;
        if (!a) throw Error("accel is NULL");
        if (!rays) throw Error("rays is NULL");
        if (!film && !rgb) throw Error("film and rgb are both NULL: at least one output");
        if (film && (film->w != w || film->h != h)) throw Error("film is " + std::to_string(film->w) + " x " + std::to_string(film->h) + ", not width x height");
        std::lock_guard<std::mutex> g(a->mtx);
        const size_t n = film_ray_count(*a, pixels, samples);
        radiance_possible(*a);
        use_device(a->device);
        const unsigned long long npix = (unsigned long long)w * h;
        DevBuf<double> drays, drgb;
        DevBuf<uint32_t> drgba;
        drays.alloc(n * 6);
        if (film) drgba.alloc(pixels);
        if (rgb) drgb.alloc(pixels * 3);
        std::vector<uint32_t> hrgba(film && offsets ? pixels : 0);
        std::vector<double> hrgb(rgb && offsets ? pixels * 3 : 0);
        const size_t direct = (size_t)std::min<unsigned long long>(pixels, npix); // no offsets: slot g is pixel g
        HIP_TRY(hipMemcpyAsync(drays.p, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        enqueue_film_query(*a, drays.p, pixels, samples, nullptr, pixels, film ? drgba.p : nullptr, rgb ? drgb.p : nullptr, a->stream);
        if (film) HIP_TRY(hipMemcpyAsync(offsets ? (void *)hrgba.data() : (void *)film->px, drgba.p, (offsets ? pixels : direct) * 4, hipMemcpyDeviceToHost, a->stream));
        if (rgb) HIP_TRY(hipMemcpyAsync(offsets ? hrgb.data() : rgb, drgb.p, (offsets ? pixels : direct) * 3 * sizeof(double), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
        if (!offsets) return;
        for (size_t s = 0; s < pixels; ++s) {
            const uint64_t off = offsets[s];
            if (off >= npix) continue;
            if (film) std::memcpy(film->px + 4 * off, &hrgba[s], 4);
            if (rgb) std::memcpy(rgb + 3 * off, &hrgb[3 * s], 3 * sizeof(double));
        }
    });
}
extern "C" int lg_capture_rays_device(const lg_accel *a, const double *dev_rays, size_t pixels, uint32_t samples, const uint64_t *dev_offsets, uint32_t w, uint32_t h,
                               void *dev_rgba, double *dev_rgb, void *hip_stream) {
    return guarded([&] {
        if (pixels == 0) return;
        if (!a) throw Error("accel is NULL");
        if (!dev_rgba && !dev_rgb) throw Error("dev_rgba and dev_rgb are both NULL: at least one output");
        std::lock_guard<std::mutex> g(a->mtx);
        const size_t n = film_ray_count(*a, pixels, samples);
        radiance_possible(*a);
        use_device(a->device);
        const unsigned long long npix = (unsigned long long)w * h;
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        if (dev_offsets) check_device_buffer(*a, dev_offsets, pixels * sizeof(uint64_t), 8, "pixel_offsets");
        if (dev_rgba) check_device_buffer(*a, dev_rgba, npix * 4, 4, "rgba");
        if (dev_rgb) check_device_buffer(*a, dev_rgb, npix * 3 * sizeof(double), 8, "rgb");
        if (npix == 0) return; // an empty film: every slot lies behind it
        enqueue_film_query(*a, dev_rays, pixels, samples, reinterpret_cast<const unsigned long long *>(dev_offsets), npix, reinterpret_cast<uint32_t *>(dev_rgba), dev_rgb,
                           (hipStream_t)hip_stream);
    });
}

// ---- feature buffers (lg_capture_features*; k_features.hip): depth, normal, albedo, coverage and ids of the camera's primary hits.  The
// struct handling that needs no device is features_host.h's.
// One capture enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the rectangle and the buffers):
// a tile is an 8 x 8 block of the rectangle (set_rect).  compact: the planes hold the rectangle's pixels
// alone, row-major (the host form's staging); otherwise they are addressed like the film
static void enqueue_features(const lg_accel &a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const lg_features &out, const double *material_rgb,
                             bool compact, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, w, h);
    set_rect(P, x0, y0, x1, y1);
    if (compact) { P.out_row0 = y0; P.out_x0 = x0; P.out_pitch = x1 - x0; }
    const TraversalGrid g = traversal_grid(a, P, features_occupancy, ctx_for(a, stream), stream);
    HIP_TRY(launch_features(P, out.depth, out.normal, out.albedo, out.coverage, out.id, out.albedo ? material_rgb : nullptr, (uint32_t)a.flat.material_pods.size(),
                            a.accel_tri_base.p, a.fast, g.blocks, g.depth, stream));
}
// Host form: the table goes up, the rectangle's pixels come back COMPACT into staging and are placed at their film offsets here -- nothing
// outside the rectangle is read or written, and an error on the way leaves the caller's planes as they were
extern "C" int lg_capture_features(const lg_accel *a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const lg_features *out, const double *material_rgb) {
    return guarded([&] {
        const size_t pixels = check_features(a, out, w, h, x0, y0, x1, y1, material_rgb);
        if (pixels == 0) return;
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        const size_t nmat = a->flat.material_pods.size();
        FeatureStaging st(*out, pixels);
        DevBuf<float> ddepth, dnormal, dalbedo, dcoverage;
        DevBuf<uint32_t> did;
        DevBuf<double> dtable;
        lg_features dev{};
        if (out->depth) { ddepth.alloc(pixels); dev.depth = ddepth.p; }
        if (out->normal) { dnormal.alloc(pixels * 3); dev.normal = dnormal.p; }
        if (out->albedo) { dalbedo.alloc(pixels * 3); dev.albedo = dalbedo.p; }
        if (out->coverage) { dcoverage.alloc(pixels); dev.coverage = dcoverage.p; }
        if (out->id) { did.alloc(pixels * 4); dev.id = did.p; }
        if (out->albedo) {
            dtable.alloc(std::max<size_t>(nmat * 3, 1));
            if (nmat) HIP_TRY(hipMemcpyAsync(dtable.p, material_rgb, nmat * 3 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        }
        enqueue_features(*a, w, h, x0, y0, x1, y1, dev, dtable.p, true, a->stream);
        if (out->depth) HIP_TRY(hipMemcpyAsync(st.depth.data(), ddepth.p, pixels * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        if (out->normal) HIP_TRY(hipMemcpyAsync(st.normal.data(), dnormal.p, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        if (out->albedo) HIP_TRY(hipMemcpyAsync(st.albedo.data(), dalbedo.p, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        if (out->coverage) HIP_TRY(hipMemcpyAsync(st.coverage.data(), dcoverage.p, pixels * sizeof(float), hipMemcpyDeviceToHost, a->stream));
        if (out->id) HIP_TRY(hipMemcpyAsync(st.id.data(), did.p, pixels * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
        place_features(*out, st, w, x0, y0, x1, y1);
    });
}
extern "C" int lg_capture_features_device(const lg_accel *a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const lg_features *out, const double *dev_material_rgb,
                           void *hip_stream) {
    return guarded([&] {
        if (check_features(a, out, w, h, x0, y0, x1, y1, dev_material_rgb) == 0) return;
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        const size_t npix = (size_t)w * h, nmat = a->flat.material_pods.size();
        if (out->depth) check_device_buffer(*a, out->depth, npix * sizeof(float), 4, "depth");
        if (out->normal) check_device_buffer(*a, out->normal, npix * 3 * sizeof(float), 4, "normal");
        if (out->albedo) check_device_buffer(*a, out->albedo, npix * 3 * sizeof(float), 4, "albedo");
        if (out->coverage) check_device_buffer(*a, out->coverage, npix * sizeof(float), 4, "coverage");
        if (out->id) check_device_buffer(*a, out->id, npix * 4 * sizeof(uint32_t), 16, "id");
        if (out->albedo) check_device_buffer(*a, dev_material_rgb, nmat * 3 * sizeof(double), 8, "material_rgb");
        enqueue_features(*a, w, h, x0, y0, x1, y1, *out, dev_material_rgb, false, (hipStream_t)hip_stream);
    });
}

// ---- lens rays (lg_lens_rays*; k_lens.hip)
static_assert(sizeof(lg_lens) == 112 && sizeof(DLens) == 112 && offsetof(lg_lens, origin) == 8 && offsetof(lg_lens, right) == 32 && offsetof(lg_lens, up) == 56 &&
                  offsetof(lg_lens, forward) == 80 && offsetof(lg_lens, fov_deg) == 104 && offsetof(DLens, fov_deg) == 104,
              "lg_lens: 112 bytes, no padding, the layout k_lens.hip reads");
static unsigned long long lens_ray_count(const lg_lens *lens, uint32_t w, uint32_t h, uint32_t root, const uint64_t *offsets, size_t pixels) {
    if (!lens) throw Error("lens is NULL");
    if (lens->kind != 0 && lens->kind != 1) throw Error("lens kind " + std::to_string(lens->kind) + ": 0 (equirectangular) or 1 (equidistant fisheye)");
    if (lens->reserved != 0) throw Error("lens: reserved must be 0");
    if (w == 0 || h == 0) throw Error("lens rays: an empty film");
    if (root == 0) throw Error("samples_root is 0");
    if (!offsets && pixels != (size_t)w * h) throw Error("lens rays: without pixel_offsets, pixels must be width * height");
    const unsigned long long S = (unsigned long long)root * root;
    if (pixels > MAX_RAYS / S) throw Error("too many lens rays (pixels * samples_root^2)");
    return pixels * S;
}
static void enqueue_lens_rays(const lg_lens *lens, uint32_t w, uint32_t h, uint32_t root, const uint64_t *dev_offsets, unsigned long long n, double *dev_rays,
                              hipStream_t stream) {
    DLens L;
    std::memcpy(&L, lens, sizeof L);
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((n + 255) / 256, 16384ull);
    HIP_TRY(launch_lens_rays(L, w, h, root, reinterpret_cast<const unsigned long long *>(dev_offsets), n, dev_rays, blocks, stream));
}

// the rectangle's rays: (x1-x0) * (y1-y0) * supersamples; 0 for an empty rectangle
static unsigned long long camera_ray_count(const lg_accel &a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    if (w == 0 || h == 0 || x0 > x1 || y0 > y1 || x1 > w || y1 > h) throw Error("rectangle outside the film");
    const unsigned long long S = (unsigned long long)a.scene->camera.ss_root * a.scene->camera.ss_root;
    return (unsigned long long)(x1 - x0) * (y1 - y0) * S;
}
static void enqueue_camera_rays(const lg_accel &a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *rays,
                                unsigned long long n, hipStream_t stream) {
    DParams P = base_params(a, w, h);
    P.x0 = x0; P.y0 = y0; P.x1 = x1; P.y1 = y1;
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((n + 255) / 256, (unsigned long long)a.cus * 64ull);
    HIP_TRY(launch_camera_rays(P, rays, n, blocks, stream));
}

extern "C" {

int lg_intersect(const lg_accel *a, const double *rays, size_t n, lg_hit *hits) { return query_host(a, rays, n, hits, false); }
int lg_occluded(const lg_accel *a, const double *rays, size_t n, uint8_t *occluded) { return query_host(a, rays, n, occluded, true); }
int lg_intersect_device(const lg_accel *a, const double *dev_rays, size_t n, lg_hit *dev_hits, void *hip_stream) {
    return query_device(a, dev_rays, n, dev_hits, false, hip_stream);
}
int lg_occluded_device(const lg_accel *a, const double *dev_rays, size_t n, uint8_t *dev_occluded, void *hip_stream) {
    return query_device(a, dev_rays, n, dev_occluded, true, hip_stream);
}
// (lg_visibility*, lg_radiance*, lg_capture_rays* and lg_capture_features* are defined in their sections above)

size_t lg_accel_material_count(const lg_accel *a) {
    if (!a) return 0;
    std::lock_guard<std::mutex> g(a->mtx);
    return a->flat.material_pods.size();
}
int lg_lens_rays(const lg_lens *lens, uint32_t width, uint32_t height, uint32_t samples_root, const uint64_t *pixel_offsets, size_t pixels, double *rays) {
    return guarded([&] {
        if (pixels == 0) return;
        const unsigned long long n = lens_ray_count(lens, width, height, samples_root, pixel_offsets, pixels);
        if (!rays) throw Error("rays is NULL");
        use_device();
        DevBuf<double> d;
        DevBuf<uint64_t> doff;
        d.alloc(n * 6);
        if (pixel_offsets) { doff.alloc(pixels); HIP_TRY(hipMemcpy(doff.p, pixel_offsets, pixels * sizeof(uint64_t), hipMemcpyHostToDevice)); }
        enqueue_lens_rays(lens, width, height, samples_root, pixel_offsets ? doff.p : nullptr, n, d.p, nullptr);
        HIP_TRY(hipMemcpy(rays, d.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost)); // (the default stream: the copy follows the kernel and blocks)
    });
}
int lg_lens_rays_device(int device, const lg_lens *lens, uint32_t width, uint32_t height, uint32_t samples_root, const uint64_t *dev_pixel_offsets, size_t pixels,
                        double *dev_rays, void *hip_stream) {
    return guarded([&] {
        if (pixels == 0) return;
        const unsigned long long n = lens_ray_count(lens, width, height, samples_root, dev_pixel_offsets, pixels);
        use_device(device);
        check_device_buffer(device, dev_rays, n * 6 * sizeof(double), 8, "rays");
        if (dev_pixel_offsets) check_device_buffer(device, dev_pixel_offsets, pixels * sizeof(uint64_t), 8, "pixel_offsets");
        enqueue_lens_rays(lens, width, height, samples_root, dev_pixel_offsets, n, dev_rays, (hipStream_t)hip_stream);
    });
}

int lg_accel_set_query_order(const lg_accel *a, int order) {
    return guarded([&] {
        if (!a) throw Error("accel is NULL");
        if (order != 0 && order != 1) throw Error("query order " + std::to_string(order) + ": 0 (as given) or 1 (sorted on the device)");
        std::lock_guard<std::mutex> g(a->mtx);
        a->query_order = order;
    });
}
int lg_accel_get_query_order(const lg_accel *a) {
    if (!a) return 0;
    std::lock_guard<std::mutex> g(a->mtx);
    return a->query_order;
}
int lg_query_order(const lg_accel *a, const double *rays, size_t n, uint32_t *perm, uint32_t *keys) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (!rays) throw Error("rays is NULL");
        if (!perm) throw Error("perm is NULL");
        if (n > MAX_SORTED_RAYS) throw Error("too many rays to order: at most 2^32 - 1");
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        DevBuf<double> drays;
        DevBuf<uint32_t> dkeys;
        drays.alloc(n * 6);
        if (keys) dkeys.alloc(n);
        HIP_TRY(hipMemcpyAsync(drays.p, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice, a->stream));
        const uint32_t *dperm = enqueue_query_order(*a, ctx_for(*a, a->stream), drays.p, n, keys ? dkeys.p : nullptr, nullptr, a->stream);
        HIP_TRY(hipMemcpyAsync(perm, dperm, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        if (keys) HIP_TRY(hipMemcpyAsync(keys, dkeys.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
    });
}
int lg_query_order_device(const lg_accel *a, const double *dev_rays, size_t n, uint32_t *dev_perm, uint32_t *dev_keys, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (n > MAX_SORTED_RAYS) throw Error("too many rays to order: at most 2^32 - 1");
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        check_device_buffer(*a, dev_perm, n * sizeof(uint32_t), 4, "perm");
        if (dev_keys) check_device_buffer(*a, dev_keys, n * sizeof(uint32_t), 4, "keys");
        check_queue_error(*a);
        (void)enqueue_query_order(*a, ctx_for(*a, (hipStream_t)hip_stream), dev_rays, n, dev_keys, dev_perm, (hipStream_t)hip_stream);
    });
}

int lg_camera_rays(const lg_accel *a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *rays) {
    return guarded([&] {
        if (!a) throw Error("accel is NULL");
        const unsigned long long n = camera_ray_count(*a, w, h, x0, y0, x1, y1);
        if (n == 0) return;
        if (!rays) throw Error("rays is NULL");
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        DevBuf<double> d;
        d.alloc(n * 6);
        enqueue_camera_rays(*a, w, h, x0, y0, x1, y1, d.p, n, a->stream);
        HIP_TRY(hipMemcpyAsync(rays, d.p, n * 6 * sizeof(double), hipMemcpyDeviceToHost, a->stream));
        sync_checked(*a);
    });
}
int lg_camera_rays_device(const lg_accel *a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *dev_rays, void *hip_stream) {
    return guarded([&] {
        if (!a) throw Error("accel is NULL");
        const unsigned long long n = camera_ray_count(*a, w, h, x0, y0, x1, y1);
        if (n == 0) return;
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        enqueue_camera_rays(*a, w, h, x0, y0, x1, y1, dev_rays, n, (hipStream_t)hip_stream);
    });
}

uint32_t lg_camera_samples(const lg_accel *a) {
    if (!a) return 0u;
    std::lock_guard<std::mutex> g(a->mtx);
    return a->scene->camera.ss_root * a->scene->camera.ss_root;
}

int lg_accel_material(const lg_accel *a, int32_t index, lg_material *out) {
    return guarded([&] {
        if (!a || !out) throw Error("accel / out is NULL");
        std::lock_guard<std::mutex> g(a->mtx);
        const std::vector<Material> &m = a->flat.material_pods;
        if (index < 0 || (size_t)index >= m.size()) throw Error("material index " + std::to_string(index) + " outside 0 .. " + std::to_string(m.size()));
        std::memcpy(out, &m[(size_t)index], sizeof *out);
    });
}
int lg_accel_instance(const lg_accel *a, uint32_t instance, int32_t *parent, int64_t *obj_ref) {
    return guarded([&] {
        if (!a) throw Error("accel is NULL");
        std::lock_guard<std::mutex> g(a->mtx);
        const FlatScene &f = a->flat;
        if ((size_t)instance >= f.accels.size()) throw Error("instance " + std::to_string(instance) + " outside 0 .. " + std::to_string(f.accels.size()));
        if (parent) *parent = f.accels[instance].parent;
        if (obj_ref) *obj_ref = f.accel_obj[instance];
    });
}

} // extern "C"
