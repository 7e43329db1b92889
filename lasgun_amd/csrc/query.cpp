// lasgun_amd/csrc/query.cpp -- ray queries (include/lasgun_hip.h: lg_intersect*, lg_occluded*, lg_visibility*, lg_open_directions*, lg_range_scan*, lg_hit_layers*, lg_hit_attributes*, lg_closest_points*, lg_nearest*, lg_closest_segments*, lg_trace_paths*, lg_radiance*, lg_radiance_gather*, lg_camera_rays*, lg_view_rays*, lg_capture_views*,
// lg_capture_features*, lg_capture_view_features*, lg_accel_material, lg_accel_instance): the caller's buffers checked, then one launch of the query's kernel (k_query.hip;
// k_visibility.hip, k_directions.hip, k_scan.hip, k_layers.hip, k_attributes.hip, k_closest.hip, k_nearest.hip, k_segments.hip, k_paths.hip, k_features.hip and k_view_features.hip for the structured queries) on the caller's stream, sized like
// the render's level-by-level traversal passes (launch.cpp, enqueue_wavefront) and walking in the accel's traversal mode -- or, for
// lg_radiance*, that pipeline itself with the caller's rays as its level 0 (launch.cpp, enqueue_radiance), and for lg_scatter* its level 0
// alone as a chain of one level (launch.cpp, enqueue_scatter; k_scatter.hip; scatter_host.h), under the call's own lights for lg_scatter_lit*
// (enqueue_scatter_lit; k_lit.hip; lit_host.h).  With
// lg_accel_set_query_order(1) the rays' keys and their sort (k_sort.hip) are enqueued ahead of it on the same stream, and the walk takes
// its tiles from the sorted order; lg_query_order* return that order.  A host form is one RoundTrip (below), whose host-memory half is
// planes_host.h's HostStaging; what a plane of a query's output struct is, is that query's one table (scan_host.h, layers_host.h,
// attributes_host.h, closest_host.h, nearest_host.h, segments_host.h, paths_host.h, scatter_host.h, lit_host.h, features_host.h, view_features_host.h), staged and checked through the two
// helpers below; what a bit row is, is bitrows_host.h's: device-free text, sanitized on the CPU.
#include <cstddef>
#include <deque>

#include "attributes_host.h"
#include "bitrows_host.h"
#include "closest_host.h"
#include "nearest_host.h"
#include "segments_host.h"
#include "features_host.h"
#include "gather_host.h"
#include "layers_host.h"
#include "paths_host.h"
#include "planes_host.h"
#include "scatter_host.h"
#include "lit_host.h"
#include "light_groups_host.h"
#include "scan_host.h"
#include "views_host.h"
#include "view_features_host.h"
#include "internal.h"

static_assert(sizeof(lg_hit) == 96 && offsetof(lg_hit, p) == 8 && offsetof(lg_hit, ng) == 32 && offsetof(lg_hit, ns) == 56 &&
                  offsetof(lg_hit, kind) == 80 && offsetof(lg_hit, prim) == 84 && offsetof(lg_hit, instance) == 88 && offsetof(lg_hit, material) == 92,
              "lg_hit: the layout k_query.hip writes (six 16-byte stores per hit)");
static_assert(sizeof(lg_material) == sizeof(Material), "lg_material wraps Material");

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
    grow(c.sort_mem, need);
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
    const bool ldss = lds_resident(a);
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

// One host form's round trip on the accel's stream (caller holds a.mtx): a device buffer is allocated as its array is named, then run() copies
// the inputs up, enqueues, copies the outputs down, synchronises and places what was staged, all in that order.  An output is DIRECT (out: the
// copy lands in the caller's memory), STAGED (staged: it lands in a buffer of this call's and reaches the caller's array after the synchronise:
// an error on the way leaves that array as it was) or HELD (held: staged, and the form places it).  A NULL array is one not asked for: NULL.
// The device buffers and the copies are here; the buffers of this call's and their placement are `staging` (planes_host.h).
class RoundTrip {
    struct Copy { void *to; const void *from; size_t bytes; };
    const lg_accel &a;
    std::deque<DevBuf<uint8_t>> mem;
    HostStaging staging;
    std::vector<Copy> up, down;
    template <class T> T *device(size_t n) { mem.emplace_back(); mem.back().alloc(std::max<size_t>(n, 1) * sizeof(T)); return reinterpret_cast<T *>(mem.back().p); }

  public:
    explicit RoundTrip(const lg_accel &accel) : a(accel) { use_device(a.device); }
    // n elements of `host` on the device (none: an element to point at, nothing copied)
    template <class T> const T *in(const T *host, size_t n) {
        if (!host) return nullptr;
        T *d = device<T>(n);
        if (n) up.push_back({d, host, n * sizeof(T)});
        return d;
    }
    // n elements for the kernel to write, the first `back` of which come back to `host` (asked for whatever `host` is)
    template <class T> T *out(T *host, size_t n, size_t back) {
        T *d = device<T>(n);
        down.push_back({host, d, back * sizeof(T)});
        return d;
    }
    template <class T> T *out(T *host, size_t n) { return host ? out(host, n, n) : nullptr; }
    template <class T> T *held(size_t n, const T **staged) {
        T *s = staging.hold<T>(n);
        *staged = s;
        return out(s, n, n);
    }
    template <class T> T *staged(T *host, size_t n) { return host ? out(staging.stage(host, n), n, n) : nullptr; }
    // a copy down from device memory that is not this call's, for the enqueue to ask for (it precedes the outputs')
    void download(void *host, const void *dev, size_t bytes) { HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, a.stream)); }
    template <class Enqueue> void run(Enqueue &&enqueue) {
        for (const Copy &c : up) HIP_TRY(hipMemcpyAsync(c.to, c.from, c.bytes, hipMemcpyHostToDevice, a.stream));
        enqueue();
        for (const Copy &c : down) download(c.to, c.from, c.bytes);
        sync_checked(a);
        staging.place();
    }
};
// The visitor of a plane table (planes_host.h) for a host form, over a copy of the caller's struct: every plane asked for becomes its device
// buffer, staged; `each`: the table counts elements a pixel, and a plane has that many times `each`
static auto staged_planes(RoundTrip &trip, size_t each = 1) {
    return [&trip, each](auto *&p, size_t count, size_t, const char *) { p = trip.staged(p, count * each); };
}
// ... and for a device form, over the caller's struct: every plane asked for is a device buffer of the accel's, aligned and long enough
static auto device_planes(const lg_accel &a, size_t each = 1) {
    return [&a, each](auto *p, size_t count, size_t align, const char *what) { if (p) check_device_buffer(a, p, count * each * sizeof *p, align, what); };
}

// Both host forms: the rays up, the query on the accel's stream, the results straight back (as lg_capture_pixels)
static int query_host(const lg_accel *a, const double *rays, size_t n, void *out, bool any) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (!rays) throw Error("rays is NULL");
        if (!out) throw Error(any ? "occluded is NULL" : "hits is NULL");
        if (n > QUERY_MAX_RAYS) throw Error("too many rays in one query");
        const size_t out_bytes = n * (any ? 1u : sizeof(lg_hit));
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        uint8_t *dout = trip.out(static_cast<uint8_t *>(out), out_bytes);
        trip.run([&] { enqueue_query(*a, drays, n, any ? nullptr : reinterpret_cast<lg_hit *>(dout), any ? dout : nullptr, a->stream); });
    });
}
static int query_device(const lg_accel *a, const double *dev_rays, size_t n, void *dev_out, bool any, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (n > QUERY_MAX_RAYS) throw Error("too many rays in one query");
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
// What both forms refuse before anything is allocated or enqueued (counts are not 0 here)
static void check_visibility(const lg_accel *a, const double *from, size_t n_from, const double *to, size_t n_to, const uint8_t *bits, size_t row_bytes,
                             const uint32_t *blocked) {
    if (!a) throw Error("accel is NULL");
    if (!from) throw Error("from is NULL");
    if (!to) throw Error("to is NULL");
    if (!bits && !blocked) throw Error("bits and blocked are both NULL: at least one output");
    check_bit_rows(n_from, n_to, 8, bits, row_bytes, "too many segments in one visibility matrix: 8 x 8 blocks are counted in 32 bits", "n_from");
}
// One matrix enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked counts and buffers): a tile is
// an 8 x 8 block
static void enqueue_visibility(const lg_accel &a, const double *from, size_t n_from, const double *to, size_t n_to, uint8_t *bits, size_t row_bytes, uint32_t *blocked,
                               hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = (uint32_t)(((n_from + 7) / 8) * bit_row_used_bytes(n_to));
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
        const size_t used = bit_row_used_bytes(n_to);
        const bool strided = bits && row_bytes != used; // compact rows are the caller's layout already: they come straight back
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        const double *dfrom = trip.in(from, n_from * 3), *dto = trip.in(to, n_to * 3);
        const uint8_t *rows = nullptr;
        uint8_t *dbits = strided ? trip.held(n_from * used, &rows) : trip.out(bits, n_from * used);
        uint32_t *dblocked = trip.staged(blocked, n_from);
        trip.run([&] { enqueue_visibility(*a, dfrom, n_from, dto, n_to, dbits, used, dblocked, a->stream); });
        if (strided) place_bit_rows(bits, row_bytes, rows, n_from, used);
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
        if (dev_bits) check_device_buffer(*a, dev_bits, bit_rows_extent(n_from, row_bytes, bit_row_used_bytes(n_to)), 1, "bits");
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
    check_bit_rows(n_points, n_dirs, 64, bits, row_bytes, "too many pairs in one direction set: tiles of 64 points x 8 directions are counted in 32 bits", "n_points");
}
// One direction set enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked counts and buffers): a
// tile is 64 points x 8 directions
static void enqueue_open_directions(const lg_accel &a, const double *points, const double *normals, size_t n_points, const double *dirs, size_t n_dirs, uint8_t *bits,
                                    size_t row_bytes, uint32_t *open, uint32_t *above, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = (uint32_t)(((n_points + 63) / 64) * bit_row_used_bytes(n_dirs));
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
        const size_t used = bit_row_used_bytes(n_dirs);
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        const double *dpoints = trip.in(points, n_points * 3), *dnormals = trip.in(normals, n_points * 3), *ddirs = trip.in(dirs, n_dirs * 3);
        const uint8_t *rows = nullptr;
        uint8_t *dbits = bits ? trip.held(n_points * used, &rows) : nullptr; // (held whatever the stride, like the counts)
        uint32_t *dopen = trip.staged(open, n_points), *dabove = trip.staged(above, n_points);
        trip.run([&] { enqueue_open_directions(*a, dpoints, dnormals, n_points, ddirs, n_dirs, dbits, used, dopen, dabove, a->stream); });
        if (bits) place_bit_rows(bits, row_bytes, rows, n_points, used);
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
        if (dev_bits) check_device_buffer(*a, dev_bits, bit_rows_extent(n_points, row_bytes, bit_row_used_bytes(n_dirs)), 1, "bits");
        if (dev_open) check_device_buffer(*a, dev_open, n_points * sizeof(uint32_t), 4, "open");
        if (dev_above) check_device_buffer(*a, dev_above, n_points * sizeof(uint32_t), 4, "above");
        enqueue_open_directions(*a, dev_points, dev_normals, n_points, dev_dirs, n_dirs, dev_bits, row_bytes, dev_open, dev_above, (hipStream_t)hip_stream);
    });
}

// ---- range scans (lg_range_scan*; k_scan.hip): the rays (origins[i], frames[i] * beams[k]) made in the kernel, their first hits written
// as planes and reduced per pose.  The arithmetic that needs no device -- the lane rule, the tile counts, the sizes, the NULL and
// alignment rules -- is scan_host.h's.
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
// Host form: the tables go up, the planes come back staged
extern "C" int lg_range_scan(const lg_accel *a, const double *origins, const double *frames, size_t n_poses, const double *beams, size_t n_beams, int lanes,
                             const lg_scan_out *out) {
    return guarded([&] {
        if (n_poses == 0 || n_beams == 0) return;
        const ScanShape shape = check_scan(a, origins, n_poses, beams, n_beams, lanes, out);
        const size_t pairs = shape.pairs;
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        const double *dorigins = trip.in(origins, n_poses * 3), *dframes = trip.in(frames, n_poses * 9), *dbeams = trip.in(beams, n_beams * 3);
        lg_scan_out dev = *out; // ... where a plane asked for becomes its device buffer
        scan_planes(dev, n_poses, pairs, staged_planes(trip));
        trip.run([&] { enqueue_range_scan(*a, dorigins, dframes, n_poses, dbeams, n_beams, shape, dev, a->stream); });
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
        scan_planes(*dev_out, n_poses, pairs, device_planes(*a));
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
        if (n > QUERY_MAX_RAYS) throw Error("too many rays in one query");
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        radiance_possible(*a);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        double *dout = trip.out(radiance, n * 3);
        trip.run([&] { enqueue_radiance_query(*a, drays, n, dout, a->stream); });
    });
}
extern "C" int lg_radiance_device(const lg_accel *a, const double *dev_rays, size_t n, double *dev_radiance, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        if (n > QUERY_MAX_RAYS) throw Error("too many rays in one query");
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        radiance_possible(*a);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        check_device_buffer(*a, dev_radiance, n * 3 * sizeof(double), 8, "radiance");
        enqueue_radiance_query(*a, dev_rays, n, dev_radiance, (hipStream_t)hip_stream);
    });
}

// ---- light groups (lg_radiance_groups*; launch.cpp, enqueue_radiance_groups; k_light_groups.hip): the radiance query with n_groups planes
// of li per ray.  What needs no device -- the limits, a group's rules, the sizes, the NULL and alignment rules, the table as it travels -- is
// light_groups_host.h's.
static_assert(sizeof(DLightGroup) == sizeof(lg_light_group) && MAX_LIGHT_GROUPS == LG_MAX_LIGHT_GROUPS && GROUP_AMBIENT == LG_GROUP_AMBIENT, "dscene.h restates the contract's group");
extern "C" int lg_accel_light_count(const lg_accel *a) { return a ? (int)a->flat.lights.size() : -1; }
// One call enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call and the buffers)
static void enqueue_groups_query(const lg_accel &a, const double *rays, size_t n, const GroupTable &table, double *radiance, hipStream_t stream) {
    check_queue_error(a);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const uint32_t *perm = query_order_of(a, c, rays, n, stream);
    enqueue_radiance_groups(a, rays, n, reinterpret_cast<const DLightGroup *>(table.groups), table.n_groups, radiance, perm, c, stream);
}
extern "C" int lg_radiance_groups(const lg_accel *a, const double *rays, size_t n, const lg_light_group *groups, size_t n_groups, double *radiance) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        std::lock_guard<std::mutex> g(a->mtx);
        GroupTable table;
        const GroupsShape shape = check_light_groups(a, rays, n, groups, n_groups, radiance, a->flat.lights.size(), table);
        check_sorted_count(*a, n);
        radiance_possible(*a);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, shape.ray_doubles);
        double *dout = trip.staged(radiance, shape.out_doubles);
        trip.run([&] { enqueue_groups_query(*a, drays, n, table, dout, a->stream); });
    });
}
extern "C" int lg_radiance_groups_device(const lg_accel *a, const double *dev_rays, size_t n, const lg_light_group *groups, size_t n_groups, double *dev_radiance,
                                         void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!a) throw Error("accel is NULL");
        std::lock_guard<std::mutex> g(a->mtx);
        GroupTable table;
        const GroupsShape shape = check_light_groups(a, dev_rays, n, groups, n_groups, dev_radiance, a->flat.lights.size(), table);
        check_light_groups_alignment(dev_rays, dev_radiance);
        check_sorted_count(*a, n);
        radiance_possible(*a);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, shape.ray_doubles * sizeof(double), 8, "rays");
        check_device_buffer(*a, dev_radiance, shape.out_doubles * sizeof(double), 8, "radiance");
        enqueue_groups_query(*a, dev_rays, n, table, dev_radiance, (hipStream_t)hip_stream);
    });
}

// ---- radiance gathers (lg_radiance_gather*; launch.cpp, enqueue_radiance_gather; k_gather.hip): li() of the rays (origins[i], frames[i] *
// dirs[k]) made in the kernel, written as a plane and / or reduced per pose by the caller's weights.  The arithmetic that needs no device --
// the lane rule, the tile counts, the sizes, the NULL and alignment rules, the batch -- is gather_host.h's.
extern "C" int lg_radiance_gather_lanes(size_t n_poses, size_t n_dirs, int lanes) { return gather_lanes(n_poses, n_dirs, lanes); }
// One gather enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked counts, scene and buffers)
static void enqueue_gather(const lg_accel &a, const double *origins, const double *frames, size_t n_poses, const double *dirs, size_t n_dirs, const double *weights,
                           size_t n_weights, const GatherShape &shape, const lg_gather_out &out, hipStream_t stream) {
    check_queue_error(a);
    static const size_t park_bytes = gather_park_bytes(std::getenv("LASGUN_GATHER_PARK_MB")); // (read once)
    const size_t batch = out.radiance ? n_poses : gather_batch_poses(n_poses, n_dirs, shape.form, park_bytes);
    const GatherCall g{origins, frames, dirs, out.sums ? weights : nullptr, n_poses, n_dirs, out.sums ? n_weights : 0, shape.form == GATHER_POSE_LANES, out.radiance, out.sums, batch};
    enqueue_radiance_gather(a, g, ctx_for(a, stream), stream);
}
// Host form: the tables go up, the outputs come back staged
extern "C" int lg_radiance_gather(const lg_accel *a, const double *origins, const double *frames, size_t n_poses, const double *dirs, size_t n_dirs, const double *weights,
                                  size_t n_weights, int lanes, const lg_gather_out *out) {
    return guarded([&] {
        if (n_poses == 0 || n_dirs == 0) return;
        const GatherShape shape = check_gather(a, origins, n_poses, dirs, n_dirs, weights, n_weights, lanes, out);
        std::lock_guard<std::mutex> g(a->mtx);
        radiance_possible(*a);
        RoundTrip trip(*a);
        const double *dorigins = trip.in(origins, n_poses * 3), *dframes = trip.in(frames, n_poses * 9), *ddirs = trip.in(dirs, n_dirs * 3);
        const double *dweights = out->sums ? trip.in(weights, n_dirs * n_weights) : nullptr;
        const lg_gather_out dev{trip.staged(out->radiance, shape.pairs * 3), trip.staged(out->sums, n_poses * n_weights * 3)};
        trip.run([&] { enqueue_gather(*a, dorigins, dframes, n_poses, ddirs, n_dirs, dweights, n_weights, shape, dev, a->stream); });
    });
}
extern "C" int lg_radiance_gather_device(const lg_accel *a, const double *dev_origins, const double *dev_frames, size_t n_poses, const double *dev_dirs, size_t n_dirs,
                                         const double *dev_weights, size_t n_weights, int lanes, const lg_gather_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n_poses == 0 || n_dirs == 0) return;
        const GatherShape shape = check_gather(a, dev_origins, n_poses, dev_dirs, n_dirs, dev_weights, n_weights, lanes, dev_out);
        check_gather_alignment(dev_origins, dev_frames, dev_dirs, dev_weights, *dev_out);
        std::lock_guard<std::mutex> g(a->mtx);
        radiance_possible(*a);
        use_device(a->device);
        check_device_buffer(*a, dev_origins, n_poses * 3 * sizeof(double), 8, "origins");
        if (dev_frames) check_device_buffer(*a, dev_frames, n_poses * 9 * sizeof(double), 8, "frames");
        check_device_buffer(*a, dev_dirs, n_dirs * 3 * sizeof(double), 8, "dirs");
        if (dev_out->sums) check_device_buffer(*a, dev_weights, n_dirs * n_weights * sizeof(double), 8, "weights");
        if (dev_out->radiance) check_device_buffer(*a, dev_out->radiance, shape.pairs * 3 * sizeof(double), 8, "radiance");
        if (dev_out->sums) check_device_buffer(*a, dev_out->sums, n_poses * n_weights * 3 * sizeof(double), 8, "sums");
        enqueue_gather(*a, dev_origins, dev_frames, n_poses, dev_dirs, n_dirs, dev_weights, n_weights, shape, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- ray films: a film from the caller's rays (lg_capture_rays*; launch.cpp, enqueue_ray_film; k_radiance.hip, the film forms)
// pixels * samples as a ray count lg_radiance accepts
static size_t film_ray_count(const lg_accel &a, size_t pixels, uint32_t samples) {
    if (samples == 0) throw Error("samples is 0: a pixel slot has at least one ray");
    if (pixels > QUERY_MAX_RAYS / samples) throw Error("too many rays in one query (pixels * samples)");
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
        RoundTrip trip(*a);
        const unsigned long long npix = (unsigned long long)w * h;
        const size_t direct = (size_t)std::min<unsigned long long>(pixels, npix); // no offsets: slot g is pixel g, and those of the film come straight back
        const double *drays = trip.in(rays, n * 6);
        const uint8_t *hrgba = nullptr; // with offsets: every slot is held and placed below
        const double *hrgb = nullptr;
        uint8_t *drgba = !film ? nullptr : offsets ? trip.held(pixels * 4, &hrgba) : trip.out(film->px, pixels * 4, direct * 4);
        double *drgb = !rgb ? nullptr : offsets ? trip.held(pixels * 3, &hrgb) : trip.out(rgb, pixels * 3, direct * 3);
        trip.run([&] { enqueue_film_query(*a, drays, pixels, samples, nullptr, pixels, reinterpret_cast<uint32_t *>(drgba), drgb, a->stream); });
        if (!offsets) return;
        for (size_t s = 0; s < pixels; ++s) {
            const uint64_t off = offsets[s];
            if (off >= npix) continue;
            if (film) std::memcpy(film->px + 4 * off, hrgba + 4 * s, 4);
            if (rgb) std::memcpy(rgb + 3 * off, hrgb + 3 * s, 3 * sizeof(double));
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

// the rectangle's rays: (x1-x0) * (y1-y0) * supersamples (the scene camera's, or a view's `root`^2); 0 for an empty rectangle
static unsigned long long camera_ray_count(const lg_accel &a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t root = 0) {
    if (w == 0 || h == 0 || x0 > x1 || y0 > y1 || x1 > w || y1 > h) throw Error("rectangle outside the film");
    if (root == 0) root = a.scene->camera.ss_root;
    return (unsigned long long)(x1 - x0) * (y1 - y0) * ((unsigned long long)root * root);
}
// (`view`: its fields in the camera's place -- camera_rays_kernel takes its camera from DParams)
static void enqueue_camera_rays(const lg_accel &a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *rays,
                                unsigned long long n, hipStream_t stream, const DView *view = nullptr) {
    DParams P = base_params(a, w, h);
    P.x0 = x0; P.y0 = y0; P.x1 = x1; P.y1 = y1;
    if (view) {
        P.cam_origin = view->origin; P.cam_view = view->view; P.cam_up = view->up; P.cam_aux = view->aux;
        P.image_plane_height = view->image_plane_height; P.pixel_separation = view->pixel_separation;
        P.ss_distance = view->ss_distance; P.ss_root = view->ss_root;
    }
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((n + 255) / 256, (unsigned long long)a.cus * 64ull);
    HIP_TRY(launch_camera_rays(P, rays, n, blocks, stream));
}

// ---- views (lg_view_look_at, lg_scene_view, lg_accel_view, lg_view_rays*, lg_capture_views*; launch.cpp, enqueue_view_batch; k_views.hip):
// one accel from K cameras into K films.  The arithmetic that needs no device -- the tile count, the sizes, what a valid view is, the NULL
// and alignment rules, lg_view -> DView -- is views_host.h's.
static lg_view view_of(const Camera &c) {
    lg_view v;
    std::memset(&v, 0, sizeof v);
    const V3 *from[4] = {&c.origin, &c.view, &c.up, &c.aux};
    double *to[4] = {v.origin, v.view, v.up, v.aux};
    for (int k = 0; k < 4; ++k) { to[k][0] = from[k]->x; to[k][1] = from[k]->y; to[k][2] = from[k]->z; }
    v.image_plane_height = c.image_plane_height; v.pixel_separation = c.pixel_separation;
    v.samples_root = c.ss_root;
    return v;
}
extern "C" int lg_view_look_at(lg_view *out, int perspective, double param, const double origin[3], const double look[3], const double up[3], uint8_t supersampling) {
    return guarded([&] {
        if (!out || !origin || !look || !up) throw Error("view look_at: a NULL pointer");
        Camera c; // the scene camera's own code, in the order a scene receives the three calls
        c.init(perspective != 0, param);
        c.look_at(V3{origin[0], origin[1], origin[2]}, V3{look[0], look[1], look[2]}, V3{up[0], up[1], up[2]});
        c.set_supersampling(supersampling);
        *out = view_of(c);
    });
}
extern "C" int lg_scene_view(const lg_scene *s, lg_view *out) {
    return guarded([&] {
        if (!s || !out) throw Error("scene / out is NULL");
        *out = view_of(s->s.camera);
    });
}
extern "C" int lg_accel_view(const lg_accel *a, lg_view *out) {
    return guarded([&] {
        if (!a || !out) throw Error("accel / out is NULL");
        std::lock_guard<std::mutex> g(a->mtx);
        *out = view_of(a->scene->camera);
    });
}
extern "C" int lg_view_rays(const lg_accel *a, const lg_view *view, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *rays) {
    return guarded([&] {
        if (!a) throw Error("accel is NULL");
        if (!view) throw Error("view is NULL");
        check_view(*view, 0);
        const unsigned long long n = camera_ray_count(*a, w, h, x0, y0, x1, y1, view->samples_root);
        if (n == 0) return;
        if (!rays) throw Error("rays is NULL");
        const DView dv = to_dview(*view);
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        double *d = trip.out(rays, n * 6);
        trip.run([&] { enqueue_camera_rays(*a, w, h, x0, y0, x1, y1, d, n, a->stream, &dv); });
    });
}
extern "C" int lg_view_rays_device(const lg_accel *a, const lg_view *view, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *dev_rays,
                                   void *hip_stream) {
    return guarded([&] {
        if (!a) throw Error("accel is NULL");
        if (!view) throw Error("view is NULL");
        check_view(*view, 0);
        const unsigned long long n = camera_ray_count(*a, w, h, x0, y0, x1, y1, view->samples_root);
        if (n == 0) return;
        const DView dv = to_dview(*view);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        enqueue_camera_rays(*a, w, h, x0, y0, x1, y1, dev_rays, n, (hipStream_t)hip_stream, &dv);
    });
}
// One batch enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call, the scene and the buffers)
static void enqueue_views(const lg_accel &a, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, const ViewShape &shape, uint32_t *rgba, double *rgb, hipStream_t stream) {
    check_queue_error(a);
    const std::vector<DView> table = to_dviews(views, n_views);
    const ViewArgs V{nullptr, (unsigned long long)n_views, w, h, shape.tiles_x, shape.tiles_per_view, 0ull, rgba, rgb};
    enqueue_view_batch(a, table.data(), V, shape.samples_root, ctx_for(a, stream), stream);
}
// Host form: the K films come back into staging and reach the caller's arrays after the synchronise (an error on the way leaves them as they were)
extern "C" int lg_capture_views(const lg_accel *a, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, uint8_t *rgba, double *rgb) {
    return guarded([&] {
        if (n_views == 0) return;
        const ViewShape shape = check_views(a, views, n_views, w, h, rgba, rgb);
        std::lock_guard<std::mutex> g(a->mtx);
        radiance_possible(*a);
        RoundTrip trip(*a);
        uint8_t *drgba = trip.staged(rgba, shape.pixels * 4);
        double *drgb = trip.staged(rgb, shape.pixels * 3);
        trip.run([&] { enqueue_views(*a, views, n_views, w, h, shape, reinterpret_cast<uint32_t *>(drgba), drgb, a->stream); });
    });
}
extern "C" int lg_capture_views_device(const lg_accel *a, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, void *dev_rgba, double *dev_rgb, void *hip_stream) {
    return guarded([&] {
        if (n_views == 0) return;
        const ViewShape shape = check_views(a, views, n_views, w, h, dev_rgba, dev_rgb);
        check_views_alignment(dev_rgba, dev_rgb);
        std::lock_guard<std::mutex> g(a->mtx);
        radiance_possible(*a);
        use_device(a->device);
        if (dev_rgba) check_device_buffer(*a, dev_rgba, shape.pixels * 4, 4, "rgba");
        if (dev_rgb) check_device_buffer(*a, dev_rgb, shape.pixels * 3 * sizeof(double), 8, "rgb");
        enqueue_views(*a, views, n_views, w, h, shape, reinterpret_cast<uint32_t *>(dev_rgba), dev_rgb, (hipStream_t)hip_stream);
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
// Host form: the table goes up, the rectangle's pixels come back COMPACT into held buffers and are placed at their film offsets here --
// nothing outside the rectangle is read or written, and an error on the way leaves the caller's planes as they were
extern "C" int lg_capture_features(const lg_accel *a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const lg_features *out, const double *material_rgb) {
    return guarded([&] {
        const size_t pixels = check_features(a, out, w, h, x0, y0, x1, y1, material_rgb);
        if (pixels == 0) return;
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        lg_features dev = *out; // ... where a plane asked for becomes its device buffer, which comes back into compact[its place in the table]
        std::vector<const void *> compact;
        feature_planes(dev, [&](auto *&p, size_t per_pixel, size_t, const char *) {
            const std::remove_reference_t<decltype(*p)> *rows = nullptr;
            if (p) p = trip.held(pixels * per_pixel, &rows);
            compact.push_back(rows);
        });
        // the table for albedo alone (a scene without materials: an element to point at, nothing copied)
        const double *dtable = out->albedo ? trip.in(material_rgb, a->flat.material_pods.size() * 3) : nullptr;
        trip.run([&] { enqueue_features(*a, w, h, x0, y0, x1, y1, dev, dtable, true, a->stream); });
        place_features(*out, compact.data(), w, x0, y0, x1, y1);
    });
}
extern "C" int lg_capture_features_device(const lg_accel *a, uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const lg_features *out, const double *dev_material_rgb,
                           void *hip_stream) {
    return guarded([&] {
        if (check_features(a, out, w, h, x0, y0, x1, y1, dev_material_rgb) == 0) return;
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        const size_t npix = (size_t)w * h, nmat = a->flat.material_pods.size();
        feature_planes(*out, device_planes(*a, npix));
        if (out->albedo) check_device_buffer(*a, dev_material_rgb, nmat * 3 * sizeof(double), 8, "material_rgb");
        enqueue_features(*a, w, h, x0, y0, x1, y1, *out, dev_material_rgb, false, (hipStream_t)hip_stream);
    });
}

// ---- view features (lg_capture_view_features*; k_view_features.hip): depth, normal, albedo, coverage, ids and hit points of the primary
// hits of K cameras, K whole films' planes in one launch.  What needs no device -- the plane table, the NULL and alignment rules, the
// film's limits, the tile count, the sizes -- is view_features_host.h's (and views_host.h's below it).
// One capture enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call and the buffers): the
// K records through the launch context's pinned staging into a table of the call's own, then ONE launch over n_views * tiles_per_view
// tiles -- no chunks: the outputs are the caller's, at most 60 bytes a pixel, and nothing is parked
static void enqueue_view_features(const lg_accel &a, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, const ViewShape &shape, const lg_view_features &out,
                                  const double *material_rgb, hipStream_t stream) {
    check_queue_error(a);
    const std::vector<DView> table = to_dviews(views, n_views);
    DParams P = base_params(a, w, h);
    P.ss_root = shape.samples_root; // (the views' own: S = samples_root^2 walks a pixel)
    P.ntiles = shape.pixel_tiles;
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    try {
        const ViewArgs V{stage_view_table(table.data(), n_views, c, stream), (unsigned long long)n_views, w, h, shape.tiles_x, shape.tiles_per_view, 0ull, nullptr, nullptr};
        const TraversalGrid g = traversal_grid(a, P, view_features_occupancy, c, stream);
        HIP_TRY(launch_view_features(P, V, out.depth, out.normal, out.albedo, out.coverage, out.id, out.point, out.albedo ? material_rgb : nullptr,
                                     (uint32_t)a.flat.material_pods.size(), a.accel_tri_base.p, a.fast, g.blocks, g.depth, stream));
        subsets_enqueued(a, stream);
    } catch (...) { subsets_abandoned(a, stream); throw; }
}
// Host form: the table goes up, the K films' planes come back into staging and reach the caller's arrays after the synchronise (an error
// on the way leaves them as they were)
extern "C" int lg_capture_view_features(const lg_accel *a, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, const lg_view_features *out, const double *material_rgb) {
    return guarded([&] {
        if (n_views == 0) return;
        const ViewShape shape = check_view_features(a, views, n_views, w, h, out, material_rgb);
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        lg_view_features dev = *out; // ... where a plane asked for becomes its device buffer
        view_feature_planes(dev, staged_planes(trip, shape.pixels));
        // the table for albedo alone (a scene without materials: an element to point at, nothing copied)
        const double *dtable = out->albedo ? trip.in(material_rgb, a->flat.material_pods.size() * 3) : nullptr;
        trip.run([&] { enqueue_view_features(*a, views, n_views, w, h, shape, dev, dtable, a->stream); });
    });
}
extern "C" int lg_capture_view_features_device(const lg_accel *a, const lg_view *views, size_t n_views, uint32_t w, uint32_t h, const lg_view_features *dev_out,
                                               const double *dev_material_rgb, void *hip_stream) {
    return guarded([&] {
        if (n_views == 0) return;
        const ViewShape shape = check_view_features(a, views, n_views, w, h, dev_out, dev_material_rgb);
        check_view_features_alignment(*dev_out, dev_material_rgb);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        view_feature_planes(*dev_out, device_planes(*a, shape.pixels));
        if (dev_out->albedo) check_device_buffer(*a, dev_material_rgb, a->flat.material_pods.size() * 3 * sizeof(double), 8, "material_rgb");
        enqueue_view_features(*a, views, n_views, w, h, shape, *dev_out, dev_material_rgb, (hipStream_t)hip_stream);
    });
}

// ---- hit layers (lg_hit_layers*; k_layers.hip): the first max_layers surfaces along each of the caller's rays, the next segment made in
// the kernel, the answer as layer-major planes.  The arithmetic that needs no device -- the limits, n * max_layers and the sizes, the NULL
// and alignment rules -- is layers_host.h's.
// One query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the counts and the buffers):
// ONE launch over the rays' 64-ray tiles -- no chunks: the outputs are the caller's, and nothing is parked
static void enqueue_hit_layers(const lg_accel &a, const double *rays, size_t n, uint32_t max_layers, const lg_layers_out &out, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = (uint32_t)((n + 63) / 64);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const uint32_t *perm = query_order_of(a, c, rays, n, stream); // (ahead of the counter's memset on the stream)
    const TraversalGrid g = traversal_grid(a, P, hit_layers_occupancy, c, stream);
    HIP_TRY(launch_hit_layers(P, rays, n, max_layers, out.hits, out.along, out.id, out.count, out.inside, a.accel_tri_base.p, perm, a.fast, g.blocks, g.depth, stream));
}
// Host form: the rays go up, the planes come back staged
extern "C" int lg_hit_layers(const lg_accel *a, const double *rays, size_t n, uint32_t max_layers, const lg_layers_out *out) {
    return guarded([&] {
        if (n == 0) return;
        const size_t total = check_layers(a, rays, n, max_layers, out);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        lg_layers_out dev = *out; // ... where a plane asked for becomes its device buffer
        layer_planes(dev, n, total, staged_planes(trip));
        trip.run([&] { enqueue_hit_layers(*a, drays, n, max_layers, dev, a->stream); });
    });
}
extern "C" int lg_hit_layers_device(const lg_accel *a, const double *dev_rays, size_t n, uint32_t max_layers, const lg_layers_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        const size_t total = check_layers(a, dev_rays, n, max_layers, dev_out);
        check_layers_alignment(dev_rays, *dev_out);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        layer_planes(*dev_out, n, total, device_planes(*a));
        enqueue_hit_layers(*a, dev_rays, n, max_layers, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- hit attributes (lg_hit_attributes*, lg_hit_attributes_of*; k_attributes.hip): where on its primitive each ray's hit lies and the frame
// it is shaded in, as planes indexed by the ray.  What needs no device -- the limits and the sizes, the NULL and alignment rules, the
// counts table and the record check -- is attributes_host.h's.
// One query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call and the buffers).
// records == nullptr, the walking form: ONE launch over the rays' 64-ray tiles -- no chunks: the outputs are the caller's, and nothing is
// parked.  Otherwise the _of form: no walk, no tile counter, no sort; a grid-stride launch over the records.
static void enqueue_hit_attributes(const lg_accel &a, const double *rays, const lg_hit *records, size_t n, const lg_attr_out &out, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    if (records) {
        const unsigned long long want = ((unsigned long long)n + 255ull) / 256ull;
        const uint32_t blocks = (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>(want, (unsigned long long)a.cus * 8ull));
        HIP_TRY(launch_attr_of(P, rays, records, n, a.attr_counts.p, out.flags, out.bary, out.uv, out.local, out.frame, out.dp, blocks, stream));
        return;
    }
    P.ntiles = (uint32_t)((n + 63) / 64);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const uint32_t *perm = query_order_of(a, c, rays, n, stream); // (ahead of the counter's memset on the stream)
    const TraversalGrid g = traversal_grid(a, P, attributes_occupancy, c, stream);
    HIP_TRY(launch_attributes(P, rays, n, out.hits, out.flags, out.bary, out.uv, out.local, out.frame, out.dp, a.accel_tri_base.p, perm, a.fast, g.blocks, g.depth, stream));
}
// Host forms: the rays (and the records) go up, the planes come back staged
static int hit_attributes_host(const lg_accel *a, const double *rays, const lg_hit *records, bool of_form, size_t n, const lg_attr_out *out) {
    return guarded([&] {
        if (n == 0) return;
        check_attributes(a, rays, records, of_form, n, out);
        std::lock_guard<std::mutex> g(a->mtx);
        if (!of_form) check_sorted_count(*a, n);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        const lg_hit *drecords = of_form ? trip.in(records, n) : nullptr;
        lg_attr_out dev = *out; // ... where a plane asked for becomes its device buffer
        attr_planes(dev, n, staged_planes(trip));
        trip.run([&] { enqueue_hit_attributes(*a, drays, drecords, n, dev, a->stream); });
    });
}
static int hit_attributes_device(const lg_accel *a, const double *dev_rays, const lg_hit *dev_records, bool of_form, size_t n, const lg_attr_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        check_attributes(a, dev_rays, dev_records, of_form, n, dev_out);
        check_attributes_alignment(dev_rays, dev_records, *dev_out);
        std::lock_guard<std::mutex> g(a->mtx);
        if (!of_form) check_sorted_count(*a, n);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        if (of_form) check_device_buffer(*a, dev_records, n * sizeof(lg_hit), 16, "hits");
        attr_planes(*dev_out, n, device_planes(*a));
        enqueue_hit_attributes(*a, dev_rays, of_form ? dev_records : nullptr, n, *dev_out, (hipStream_t)hip_stream);
    });
}
extern "C" int lg_hit_attributes(const lg_accel *a, const double *rays, size_t n, const lg_attr_out *out) { return hit_attributes_host(a, rays, nullptr, false, n, out); }
extern "C" int lg_hit_attributes_device(const lg_accel *a, const double *dev_rays, size_t n, const lg_attr_out *dev_out, void *hip_stream) {
    return hit_attributes_device(a, dev_rays, nullptr, false, n, dev_out, hip_stream);
}
extern "C" int lg_hit_attributes_of(const lg_accel *a, const double *rays, const lg_hit *hits, size_t n, const lg_attr_out *out) {
    return hit_attributes_host(a, rays, hits, true, n, out);
}
extern "C" int lg_hit_attributes_of_device(const lg_accel *a, const double *dev_rays, const lg_hit *dev_hits, size_t n, const lg_attr_out *dev_out, void *hip_stream) {
    return hit_attributes_device(a, dev_rays, dev_hits, true, n, dev_out, hip_stream);
}

// ---- closest points (lg_closest_points*; k_closest.hip): for each of the caller's points the nearest surface point of the scene.  What
// needs no device -- the limits and the sizes, the NULL and alignment rules, the sphere gate, the pruning test's constants and the stack
// depth -- is closest_host.h's.
// The query's own tables, made from the accel's flattened scene at its first call (caller holds a.mtx and has made the device current)
static const ClosestTables &closest_tables_of(const lg_accel &a) {
    if (!a.closest) {
        const FlatScene &f = a.flat;
        auto t = std::make_shared<ClosestTables>(closest_tables(ClosestScene{f.accels.data(), f.accels.size(), f.nodes.data(), f.nodes.size(), f.primref.data(),
                                                                             f.primref.size(), f.leaf_soup.data(), f.leaf_soup.size()}));
        a.closest_cl.obtain(t->accel.size() * sizeof(ClosestAccel));
        HIP_TRY(hipMemcpy(a.closest_cl.p, t->accel.data(), t->accel.size() * sizeof(ClosestAccel), hipMemcpyHostToDevice));
        a.closest = t;
    }
    return *a.closest;
}
// What the scene itself may be refused for, in the contract's order
static const ClosestTables &check_closest_scene(const lg_accel &a) {
    const ClosestTables &t = closest_tables_of(a);
    if (t.refused >= 0)
        throw Error("closest points: instance " + std::to_string(t.refused) + " holds a sphere under a transform chain that is no similarity (lg_scene_closest_gate)");
    if (t.depth > CLOSEST_MAX_DEPTH)
        throw Error("closest points: the scene's trees need a stack of " + std::to_string(t.depth) + " entries, the kernel's holds " + std::to_string(CLOSEST_MAX_DEPTH));
    return t;
}
// One query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call, the scene and the
// buffers): ONE launch over the points' 64-point tiles -- no chunks: the outputs are the caller's, and nothing is parked
static void enqueue_closest(const lg_accel &a, const ClosestTables &t, const double *points, size_t n, double radius, const lg_closest_out &out, hipStream_t stream) {
    check_queue_error(a);
    const DParams P = base_params(a, 1, 1);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const size_t lds = closest_stack_bytes(t.depth);
    // beyond the default 64 KiB the kernel's limit is raised -- always to the most any scene may ask for, so that two accels of different
    // depths used from two threads never lower it under each other's launch
    if (lds > (64u << 10)) HIP_TRY(closest_set_lds_limit(closest_stack_bytes(CLOSEST_MAX_DEPTH)));
    int per_cu = 0;
    HIP_TRY(closest_occupancy(t.depth, &per_cu));
    const unsigned long long tiles = ((unsigned long long)n + 63ull) / 64ull, want = (tiles + 3ull) / 4ull; // four waves a workgroup
    const uint32_t blocks = (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>(want, (unsigned long long)(per_cu < 1 ? 1 : per_cu) * a.cus));
    HIP_TRY(hipMemsetAsync(c.tile_counter.p, 0, TILE_COUNTER_WORDS * sizeof(uint32_t), stream));
    HIP_TRY(launch_closest(P, points, n, radius * radius, t.qmax, out.distance, out.point, out.id, a.accel_tri_base.p, a.closest_cl.p, c.tile_counter.p, blocks, t.depth, stream));
}
// Host form: the points go up, the planes come back staged
extern "C" int lg_closest_points(const lg_accel *a, const double *points, size_t n, double radius, const lg_closest_out *out) {
    return guarded([&] {
        if (n == 0) return;
        check_closest(a, points, n, radius, out);
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        const ClosestTables &t = check_closest_scene(*a);
        const double *dpoints = trip.in(points, n * 3);
        lg_closest_out dev = *out; // ... where a plane asked for becomes its device buffer
        closest_planes(dev, n, staged_planes(trip));
        trip.run([&] { enqueue_closest(*a, t, dpoints, n, radius, dev, a->stream); });
    });
}
extern "C" int lg_closest_points_device(const lg_accel *a, const double *dev_points, size_t n, double radius, const lg_closest_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        check_closest(a, dev_points, n, radius, dev_out);
        check_closest_alignment(dev_points, *dev_out);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        const ClosestTables &t = check_closest_scene(*a);
        check_device_buffer(*a, dev_points, n * 3 * sizeof(double), 8, "points");
        closest_planes(*dev_out, n, device_planes(*a));
        enqueue_closest(*a, t, dev_points, n, radius, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- proximity queries (lg_nearest*; k_nearest.hip): for each of the caller's points, under a radius of its own, the k nearest primitives
// in order, the count of those within the radius, and whether any is.  The scene's tables, its gate and its depth rule are closest points'
// own (closest_tables_of, check_closest_scene); what else needs no device -- the five planes, k, n * k and the sizes, the LDS rule -- is
// nearest_host.h's.
// What the scene itself may be refused for, in the contract's order: the gate, the stack's depth, then stack plus lists against the LDS
static const ClosestTables &check_nearest_scene(const lg_accel &a, uint32_t entries) {
    const ClosestTables &t = check_closest_scene(a);
    check_nearest_lds(t.depth, entries);
    return t;
}
// One query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call, the scene and the
// buffers): ONE launch over the points' 64-point tiles, in the form the planes asked for need, the grid sized by that form's occupancy
static void enqueue_nearest(const lg_accel &a, const ClosestTables &t, const double *points, const double *radii, size_t n, double radius, uint32_t entries,
                            const lg_nearest_out &out, hipStream_t stream) {
    check_queue_error(a);
    const DParams P = base_params(a, 1, 1);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const int form = nearest_form(out.count != nullptr, entries != 0u);
    // beyond the default 64 KiB the kernels' limit is raised -- always to the most any call may ask for, so that two accels used from two
    // threads never lower it under each other's launch
    if (nearest_lds_bytes(t.depth, entries) > (64u << 10)) HIP_TRY(nearest_set_lds_limit(NEAREST_LDS_LIMIT));
    int per_cu = 0;
    HIP_TRY(nearest_occupancy(form, t.depth, entries, &per_cu));
    const unsigned long long tiles = ((unsigned long long)n + 63ull) / 64ull, want = (tiles + 3ull) / 4ull; // four waves a workgroup
    const uint32_t blocks = (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>(want, (unsigned long long)(per_cu < 1 ? 1 : per_cu) * a.cus));
    HIP_TRY(hipMemsetAsync(c.tile_counter.p, 0, TILE_COUNTER_WORDS * sizeof(uint32_t), stream));
    HIP_TRY(launch_nearest(P, form, points, radii, n, radii ? 0.0 : radius * radius, t.qmax, entries, out.touch, out.count, out.distance, out.point, out.id, a.accel_tri_base.p,
                           a.closest_cl.p, c.tile_counter.p, blocks, t.depth, stream));
}
// Host form: points and radii go up, the planes come back staged
extern "C" int lg_nearest(const lg_accel *a, const double *points, const double *radii, size_t n, double radius, uint32_t k, const lg_nearest_out *out) {
    return guarded([&] {
        if (n == 0) return;
        const size_t nk = check_nearest(a, points, radii, n, radius, k, out);
        const uint32_t entries = nearest_entries(*out, k);
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        const ClosestTables &t = check_nearest_scene(*a, entries);
        const double *dpoints = trip.in(points, n * 3), *dradii = trip.in(radii, n);
        lg_nearest_out dev = *out; // ... where a plane asked for becomes its device buffer
        nearest_planes(dev, n, nk, staged_planes(trip));
        trip.run([&] { enqueue_nearest(*a, t, dpoints, dradii, n, radius, entries, dev, a->stream); });
    });
}
extern "C" int lg_nearest_device(const lg_accel *a, const double *dev_points, const double *dev_radii, size_t n, double radius, uint32_t k, const lg_nearest_out *dev_out,
                                 void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        const size_t nk = check_nearest(a, dev_points, dev_radii, n, radius, k, dev_out);
        check_nearest_alignment(dev_points, dev_radii, *dev_out);
        const uint32_t entries = nearest_entries(*dev_out, k);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        const ClosestTables &t = check_nearest_scene(*a, entries);
        check_device_buffer(*a, dev_points, n * 3 * sizeof(double), 8, "points");
        if (dev_radii) check_device_buffer(*a, dev_radii, n * sizeof(double), 8, "radii");
        nearest_planes(*dev_out, n, nk, device_planes(*a));
        enqueue_nearest(*a, t, dev_points, dev_radii, n, radius, entries, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- segment proximity (lg_closest_segments*; k_segments.hip): for each of the caller's segments, under a radius of its own, the nearest
// surface point of the scene to the segment.  The scene's tables, its gate and its depth rule are closest points' own (closest_tables_of,
// check_closest_scene); what else needs no device -- the five planes, the sizes -- is segments_host.h's.  The LDS is the stack alone.
// One query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call, the scene and the
// buffers): ONE launch over the segments' 64-segment tiles, in the form the planes asked for need
static void enqueue_segments(const lg_accel &a, const ClosestTables &t, const double *segments, const double *radii, size_t n, double radius, const lg_segments_out &out,
                             hipStream_t stream) {
    check_queue_error(a);
    const DParams P = base_params(a, 1, 1);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const bool touch_only = segments_touch_only(out);
    // beyond the default 64 KiB the kernels' limit is raised -- always to the most any scene may need, as closest points does
    if (closest_stack_bytes(t.depth) > (64u << 10)) HIP_TRY(segments_set_lds_limit(closest_stack_bytes(CLOSEST_MAX_DEPTH)));
    int per_cu = 0;
    HIP_TRY(segments_occupancy(touch_only, t.depth, &per_cu));
    const unsigned long long tiles = ((unsigned long long)n + 63ull) / 64ull, want = (tiles + 3ull) / 4ull; // four waves a workgroup
    const uint32_t blocks = (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>(want, (unsigned long long)(per_cu < 1 ? 1 : per_cu) * a.cus));
    HIP_TRY(hipMemsetAsync(c.tile_counter.p, 0, TILE_COUNTER_WORDS * sizeof(uint32_t), stream));
    HIP_TRY(launch_segments(P, touch_only, segments, radii, n, radii ? 0.0 : radius * radius, t.qmax, out.touch, out.distance, out.param, out.point, out.id, a.accel_tri_base.p,
                            a.closest_cl.p, c.tile_counter.p, blocks, t.depth, stream));
}
// Host form: segments and radii go up, the planes come back staged
extern "C" int lg_closest_segments(const lg_accel *a, const double *segments, const double *radii, size_t n, double radius, const lg_segments_out *out) {
    return guarded([&] {
        if (n == 0) return;
        check_segments(a, segments, radii, n, radius, out);
        std::lock_guard<std::mutex> g(a->mtx);
        RoundTrip trip(*a);
        const ClosestTables &t = check_closest_scene(*a);
        const double *dsegments = trip.in(segments, n * 6), *dradii = trip.in(radii, n);
        lg_segments_out dev = *out; // ... where a plane asked for becomes its device buffer
        segments_planes(dev, n, staged_planes(trip));
        trip.run([&] { enqueue_segments(*a, t, dsegments, dradii, n, radius, dev, a->stream); });
    });
}
extern "C" int lg_closest_segments_device(const lg_accel *a, const double *dev_segments, const double *dev_radii, size_t n, double radius, const lg_segments_out *dev_out,
                                          void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        check_segments(a, dev_segments, dev_radii, n, radius, dev_out);
        check_segments_alignment(dev_segments, dev_radii, *dev_out);
        std::lock_guard<std::mutex> g(a->mtx);
        use_device(a->device);
        const ClosestTables &t = check_closest_scene(*a);
        check_device_buffer(*a, dev_segments, n * 6 * sizeof(double), 8, "segments");
        if (dev_radii) check_device_buffer(*a, dev_radii, n * sizeof(double), 8, "radii");
        segments_planes(*dev_out, n, device_planes(*a));
        enqueue_segments(*a, t, dev_segments, dev_radii, n, radius, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- ray paths (lg_trace_paths*; k_paths.hip): each of the caller's rays followed through up to max_bounces vertices, the next segment
// formed in the kernel by the rule of the hit's material, the answer as vertex-major and per-ray planes.  What needs no device -- the limits,
// n * max_bounces and the sizes, the rule table's validation, the NULL and alignment rules -- is paths_host.h's.
// One query enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call and the buffers): the
// rules through the launch context's pinned staging into a table of the call's own (the caller's array may be freed on return), then ONE
// launch over the rays' 64-ray tiles -- no chunks: the outputs are the caller's, and nothing is parked
static void enqueue_trace_paths(const lg_accel &a, const double *rays, size_t n, uint32_t max_bounces, const lg_path_rule *rules, size_t n_rules, int normal,
                                const uint32_t *start_medium, const lg_paths_out &out, hipStream_t stream) {
    check_queue_error(a);
    DParams P = base_params(a, 1, 1);
    P.ntiles = (uint32_t)((n + 63) / 64);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    try {
        const void *table = stage_rule_table(rules, n_rules * sizeof(lg_path_rule), c, stream);
        const uint32_t *perm = query_order_of(a, c, rays, n, stream); // (ahead of the counter's memset on the stream)
        const TraversalGrid g = traversal_grid(a, P, trace_paths_occupancy, c, stream);
        HIP_TRY(launch_trace_paths(P, rays, n, max_bounces, table, (uint32_t)n_rules, normal == 1, start_medium, out.hits, out.point, out.id, out.along, out.count, out.end,
                                   out.gain, out.last, out.medium, a.accel_tri_base.p, perm, a.fast, g.blocks, g.depth, stream));
        subsets_enqueued(a, stream);
    } catch (...) { subsets_abandoned(a, stream); throw; }
}
// Host form: the rays (and the starting media) go up, the planes come back staged
extern "C" int lg_trace_paths(const lg_accel *a, const double *rays, size_t n, uint32_t max_bounces, const lg_path_rule *rules, size_t n_rules, int normal,
                              const uint32_t *start_medium, const lg_paths_out *out) {
    return guarded([&] {
        if (n == 0) return;
        const size_t total = check_paths(a, rays, n, max_bounces, rules, n_rules, lg_accel_material_count(a), normal, out);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        const uint32_t *dmedium = trip.in(start_medium, n);
        lg_paths_out dev = *out; // ... where a plane asked for becomes its device buffer
        path_planes(dev, n, total, staged_planes(trip));
        trip.run([&] { enqueue_trace_paths(*a, drays, n, max_bounces, rules, n_rules, normal, dmedium, dev, a->stream); });
    });
}
extern "C" int lg_trace_paths_device(const lg_accel *a, const double *dev_rays, size_t n, uint32_t max_bounces, const lg_path_rule *rules, size_t n_rules, int normal,
                                     const uint32_t *dev_start_medium, const lg_paths_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        const size_t total = check_paths(a, dev_rays, n, max_bounces, rules, n_rules, lg_accel_material_count(a), normal, dev_out);
        check_paths_alignment(dev_rays, dev_start_medium, *dev_out);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        if (dev_start_medium) check_device_buffer(*a, dev_start_medium, n * sizeof(uint32_t), 4, "start_medium");
        path_planes(*dev_out, n, total, device_planes(*a));
        enqueue_trace_paths(*a, dev_rays, n, max_bounces, rules, n_rules, normal, dev_start_medium, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- surface scatter (lg_scatter*; launch.cpp, enqueue_scatter; k_scatter.hip): one level of li()'s tree, opened -- the hit, the light and
// ambient sum at it and the two specular children with their weights, as planes indexed by the ray.  What needs no device -- the limits,
// the sizes, the NULL and alignment rules, the light count's refusal -- is scatter_host.h's.
static_assert(SCATTER_HIT == LG_SCATTER_HIT && SCATTER_REFLECT == LG_SCATTER_REFLECT && SCATTER_REFRACT == LG_SCATTER_REFRACT, "dscene.h restates the contract's flags");
// One call enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call and the buffers)
static void enqueue_scatter_query(const lg_accel &a, const double *rays, size_t n, const lg_scatter_out &out, hipStream_t stream) {
    check_queue_error(a);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const uint32_t *perm = query_order_of(a, c, rays, n, stream);
    ScatterArgs Q{};
    Q.hits = out.hits; Q.direct = out.direct; Q.flags = out.flags;
    Q.reflect = out.reflect; Q.reflect_weight = out.reflect_weight; Q.refract = out.refract; Q.refract_weight = out.refract_weight;
    enqueue_scatter(a, rays, n, Q, perm, c, stream);
}
// Host form: the rays go up, the planes come back staged
extern "C" int lg_scatter(const lg_accel *a, const double *rays, size_t n, const lg_scatter_out *out) {
    return guarded([&] {
        if (n == 0) return;
        check_scatter(a, rays, n, out, a ? a->flat.lights.size() : 0);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        lg_scatter_out dev = *out; // ... where a plane asked for becomes its device buffer
        scatter_planes(dev, n, staged_planes(trip));
        trip.run([&] { enqueue_scatter_query(*a, drays, n, dev, a->stream); });
    });
}
extern "C" int lg_scatter_device(const lg_accel *a, const double *dev_rays, size_t n, const lg_scatter_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        check_scatter(a, dev_rays, n, dev_out, a ? a->flat.lights.size() : 0);
        check_scatter_alignment(dev_rays, *dev_out);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        scatter_planes(*dev_out, n, device_planes(*a));
        enqueue_scatter_query(*a, dev_rays, n, *dev_out, (hipStream_t)hip_stream);
    });
}

// ---- lit scatter (lg_scatter_lit*; launch.cpp, enqueue_scatter_lit; k_lit.hip): surface scatter under lights that come with the call,
// with every light's term and the visibility bits as two more planes.  What needs no device -- the light set's rules, W, the sizes, the
// NULL and alignment rules -- is lit_host.h's.
static_assert(MAX_CALL_LIGHTS == LG_MAX_CALL_LIGHTS && sizeof(DLight) == sizeof(lg_light), "dscene.h restates the contract's light record and limit");
// The skip (k_lit.hip): on unless LASGUN_LIT_SKIP=0 (for the measurement of what it buys); never where `visible` is asked for
static bool lit_skip_on() {
    static const bool on = [] { const char *e = std::getenv("LASGUN_LIT_SKIP"); return !(e && e[0] == '0'); }();
    return on;
}
// One call enqueued on `stream` (caller holds a.mtx, has made the accel's device current and has checked the call and the buffers):
// `table` is the light table where the kernels will find it -- a per-ray table on the device -- or, shared, the caller's host array
static void enqueue_lit_query(const lg_accel &a, const double *rays, size_t n, const lg_light_set &lights, const lg_light *table, const LitSizes &z, const lg_lit_out &out,
                              hipStream_t stream) {
    check_queue_error(a);
    lg_accel::LaunchCtx &c = ctx_for(a, stream);
    const uint32_t *perm = query_order_of(a, c, rays, n, stream);
    LitArgs Q{};
    const lg_scatter_out &so = out.scatter;
    Q.hits = so.hits; Q.direct = so.direct; Q.flags = so.flags;
    Q.reflect = so.reflect; Q.reflect_weight = so.reflect_weight; Q.refract = so.refract; Q.refract_weight = so.refract_weight;
    Q.terms = z.K ? out.terms : nullptr;
    Q.visible = z.K ? out.visible : nullptr;
    Q.n_lights = (uint32_t)z.K; Q.per_ray = lights.per_ray; Q.vis_words = (uint32_t)z.W;
    Q.skip = z.K && !Q.visible && lit_skip_on() ? 1u : 0u;
    for (int k = 0; k < 3; ++k) Q.ambient[k] = lights.ambient[k];
    Q.lights = lights.per_ray ? reinterpret_cast<const DLight *>(table) : nullptr;
    enqueue_scatter_lit(a, rays, n, Q, lights.per_ray ? nullptr : reinterpret_cast<const DLight *>(table), perm, c, stream);
}
// Host form: the rays (and a per-ray light table) go up, the planes come back staged
extern "C" int lg_scatter_lit(const lg_accel *a, const double *rays, size_t n, const lg_light_set *lights, const lg_lit_out *out) {
    return guarded([&] {
        if (n == 0) return;
        const LitSizes z = check_lit(a, rays, n, lights, out);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        const lg_light *table = lights->per_ray && z.K ? trip.in(lights->lights, z.lights) : lights->lights;
        lg_lit_out dev = *out; // ... where a plane asked for becomes its device buffer
        lit_planes(dev, z, staged_planes(trip));
        trip.run([&] { enqueue_lit_query(*a, drays, n, *lights, table, z, dev, a->stream); });
    });
}
extern "C" int lg_scatter_lit_device(const lg_accel *a, const double *dev_rays, size_t n, const lg_light_set *lights, const lg_lit_out *dev_out, void *hip_stream) {
    return guarded([&] {
        if (n == 0) return;
        const LitSizes z = check_lit(a, dev_rays, n, lights, dev_out);
        check_lit_alignment(dev_rays, *lights, *dev_out, z);
        std::lock_guard<std::mutex> g(a->mtx);
        check_sorted_count(*a, n);
        use_device(a->device);
        check_device_buffer(*a, dev_rays, n * 6 * sizeof(double), 8, "rays");
        if (lights->per_ray && z.K) check_device_buffer(*a, lights->lights, z.lights * sizeof(lg_light), 8, "lights->lights");
        lit_planes(*dev_out, z, device_planes(*a));
        enqueue_lit_query(*a, dev_rays, n, *lights, lights->lights, z, *dev_out, (hipStream_t)hip_stream);
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
    if (pixels > QUERY_MAX_RAYS / S) throw Error("too many lens rays (pixels * samples_root^2)");
    return pixels * S;
}
static void enqueue_lens_rays(const lg_lens *lens, uint32_t w, uint32_t h, uint32_t root, const uint64_t *dev_offsets, unsigned long long n, double *dev_rays,
                              hipStream_t stream) {
    DLens L;
    std::memcpy(&L, lens, sizeof L);
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((n + 255) / 256, 16384ull);
    HIP_TRY(launch_lens_rays(L, w, h, root, reinterpret_cast<const unsigned long long *>(dev_offsets), n, dev_rays, blocks, stream));
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
        RoundTrip trip(*a);
        const double *drays = trip.in(rays, n * 6);
        uint32_t *dkeys = trip.out(keys, n);
        trip.run([&] { // (the permutation is left in the context's scratch: it comes back from there)
            trip.download(perm, enqueue_query_order(*a, ctx_for(*a, a->stream), drays, n, dkeys, nullptr, a->stream), n * sizeof(uint32_t));
        });
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
        RoundTrip trip(*a);
        double *d = trip.out(rays, n * 6);
        trip.run([&] { enqueue_camera_rays(*a, w, h, x0, y0, x1, y1, d, n, a->stream); });
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
