// lasgun_amd/csrc/internal.h -- what the host-side units of liblasgun_hip share (round 6: capi.cpp was one 2,600-line file):
//   devmem.cpp  the process-wide pools (device blocks, streams, pinned staging, error words), the current device, the last error
//   accel.cpp   lg_accel_from: flatten, LDS images, upload; the tables rebuilt with what was left out of them
//   launch.cpp  one render enqueued: launch contexts, the three organisations, the rule and the measured choice (tune.cpp), addressing modes
//   capi.cpp    the C ABI of include/lasgun_hip.h over them
// No torch types, no C++ exceptions across the boundary, no CPU render path.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lasgun_hip.h"
#include "host.h"
#include "raykey.h"
#include "tune.h"

namespace lg {
// k_mega.hip, k_wavefront.hip, k_queue.hip, k_probe.hip
hipError_t launch_trace(const DParams &P, bool stats, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t trace_occupancy(uint32_t stack_depth, bool fast, size_t extra_lds, int *blocks_per_cu);
hipError_t launch_wf_trace(const DParams &P, bool fast, bool shadow, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_wf_shade(const DParams &P, uint32_t blocks, hipStream_t stream);
hipError_t launch_wf_combine(const DParams &P, uint32_t blocks, hipStream_t stream);
// k_tri_frames.hip: the frame table's build kernel (tri_frames_host.h); P: the scene tables alone
hipError_t launch_tri_frames(const DParams &P, const DTriFrameJob *jobs, uint32_t n, DTriFrame *out, hipStream_t stream);
// k_query.hip: ray queries (query.cpp) -- hits != nullptr: closest hit into lg_hit[n]; occluded != nullptr: the any-hit walk, one byte per ray
// perm != nullptr: the rays are walked in that order (slot s walks ray perm[s]); answers go to the ray's own slot either way
hipError_t launch_query(const DParams &P, const double *rays, unsigned long long n, void *hits, uint8_t *occluded, const uint32_t *tri_base,
                        const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
// k_sort.hip: the rays' coherence keys (raykey.h) and their stable sort; scratch of sort_scratch_bytes(n) bytes, 256-byte aligned
size_t sort_scratch_bytes(unsigned long long n);
hipError_t launch_query_order(const double *rays, unsigned long long n, const KeyBounds &B, void *scratch, uint32_t *keys_out, uint32_t *perm_out,
                              const uint32_t **perm, uint32_t grid_cap, hipStream_t stream);
hipError_t launch_camera_rays(const DParams &P, double *rays, unsigned long long n, uint32_t blocks, hipStream_t stream);
// (the *_occupancy of the query kernels: workgroups per CU of the 256-lane form that P, without an LDS-resident scene, takes -- travform.h)
hipError_t query_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t query_set_lds_limit(size_t bytes, bool ldss);
hipError_t launch_wf_resolve(const DParams &P, uint32_t blocks, hipStream_t stream);
// k_radiance.hip: level 0 of the level-by-level pipeline for a radiance query's rays (launch.cpp, enqueue_radiance)
hipError_t launch_rq_closest(const DParams &P, const RadianceArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_rq_shade(const DParams &P, const RadianceArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_rq_combine(const DParams &P, const RadianceArgs &Q, uint32_t blocks, hipStream_t stream);
// ... and its film forms (lg_capture_rays*): one ray per pixel slot finished into a film; the resolve pass of several samples per slot
hipError_t launch_rf_closest(const DParams &P, const FilmArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_rf_shade(const DParams &P, const FilmArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_rf_combine(const DParams &P, const FilmArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_rf_resolve(const FilmArgs &Q, const double *li, unsigned long long slots, uint32_t samples, uint32_t blocks, hipStream_t stream);
hipError_t rq_set_lds_limit(size_t bytes, bool ldss);
// k_scatter.hip: surface scatter (lg_scatter*; launch.cpp, enqueue_scatter) -- level 0 as a chain of one level: the closest pass over the
// query's rays (it writes the hit records and the misses' planes) and, in the shade pass's place, the emit pass (the hits' planes)
hipError_t launch_scatter_closest(const DParams &P, const ScatterArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_scatter_emit(const DParams &P, const ScatterArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t scatter_set_lds_limit(size_t bytes, bool ldss);
// k_lit.hip: lit scatter (lg_scatter_lit*; launch.cpp, enqueue_scatter_lit) -- surface scatter's chain under the call's lights: its own closest
// pass (a miss's rows of `terms` and `visible` too), the shadow pass over hit tiles x visibility words, and the emit pass
hipError_t launch_lit_closest(const DParams &P, const LitArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_lit_shadow(const DParams &P, const LitArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_lit_emit(const DParams &P, const LitArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t lit_set_lds_limit(size_t bytes, bool ldss);
// k_light_groups.hip: light groups (lg_radiance_groups*; launch.cpp, enqueue_radiance_groups) -- the radiance query's level-0 closest pass with
// a GroupArgs, and the shade and combine passes of EVERY level (P.wf_level) carrying Q.n_groups planes; the spread pass of the deepest level
hipError_t launch_lg_closest(const DParams &P, const GroupArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_lg_shade(const DParams &P, const GroupArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_lg_combine(const DParams &P, const GroupArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_lg_spread(const DParams &P, const GroupArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t light_groups_set_lds_limit(size_t bytes, bool ldss);
// k_gather.hip: level 0 for the rays of a radiance gather (launch.cpp, enqueue_radiance_gather), and its reduction:
// sums[(i*n_weights + c)*3 ..] = the sequential weighted sum of pose i's li over the directions
hipError_t launch_gather_closest(const DParams &P, const GatherArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_gather_shade(const DParams &P, const GatherArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_gather_combine(const DParams &P, const GatherArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_gather_resolve(const double *li, const double *weights, double *sums, unsigned long long n_poses, unsigned long long n_dirs, unsigned long long n_weights,
                                 uint32_t blocks, hipStream_t stream);
hipError_t gather_set_lds_limit(size_t bytes, bool ldss);
// k_views.hip: level 0 for the cameras of a view batch (launch.cpp, enqueue_view_batch), and the resolve pass of its chunks
// (P.ntiles = the chunk's pixel tiles) where a pixel has several samples
hipError_t launch_view_closest(const DParams &P, const ViewArgs &Q, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t launch_view_shade(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_view_combine(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t launch_view_resolve(const DParams &P, const ViewArgs &Q, uint32_t blocks, hipStream_t stream);
hipError_t view_set_lds_limit(size_t bytes, bool ldss);
// k_lens.hip: the rays of a lens camera (lg_lens_rays*)
hipError_t launch_lens_rays(const DLens &L, uint32_t w, uint32_t h, uint32_t root, const unsigned long long *offsets, unsigned long long n, double *rays,
                            uint32_t blocks, hipStream_t stream);
// k_visibility.hip: visibility matrices (lg_visibility*) -- the any-hit walk of the segments from[i] -> to[j], an 8 x 8 block of the matrix
// per wave; bit j of bits[i * row_bytes ..] and / or the row's count in blocked[i] (zeroed by the caller ahead of the launch)
hipError_t launch_visibility(const DParams &P, const double *from, unsigned long long n_from, const double *to, unsigned long long n_to, uint8_t *bits,
                             unsigned long long row_bytes, uint32_t *blocked, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t visibility_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t visibility_set_lds_limit(size_t bytes, bool ldss);
// k_directions.hip: direction sets (lg_open_directions*) -- the any-hit walk of the rays (points[i], dirs[k]) that are above the point's
// horizon, 64 points x 8 directions per wave; bit k of bits[i * row_bytes ..] set iff open, and / or the counts in open[i] and above[i]
// (both zeroed by the caller ahead of the launch); normals may be nullptr (every pair above)
hipError_t launch_open_directions(const DParams &P, const double *points, const double *normals, unsigned long long n_points, const double *dirs,
                                  unsigned long long n_dirs, uint8_t *bits, unsigned long long row_bytes, uint32_t *open, uint32_t *above, bool fast,
                                  uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t open_directions_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t open_directions_set_lds_limit(size_t bytes, bool ldss);
// k_scan.hip: range scans (lg_range_scan*) -- the closest-hit walk of the rays (origins[i], frames[i] * beams[k]), one pose x 64 beams
// (beam lanes) or 64 poses x 8 beams (pose_lanes) per wave; only the outputs that are not nullptr are written, element (i, k) at
// i * n_beams + k; hits and nearest are pre-filled by the caller ahead of the launch (0 and 0x7F800000); frames may be nullptr
hipError_t launch_range_scan(const DParams &P, const double *origins, const double *frames, unsigned long long n_poses, const double *beams,
                             unsigned long long n_beams, bool pose_lanes, float *range, float *point, float *normal, void *id, uint32_t *hits, uint32_t *nearest,
                             const uint32_t *tri_base, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t range_scan_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t range_scan_set_lds_limit(size_t bytes, bool ldss);
// k_layers.hip: hit layers (lg_hit_layers*) -- the closest-hit walk of the caller's rays repeated up to max_layers times a ray, the next
// segment started at the hit's p - ng * 2^-36 (shade_frame's pm) in registers; a 64-ray tile per wave and a ray per lane; only the planes
// that are not nullptr are written, layer-major: element (j, i) at j * n + i; perm != nullptr: the tiles are cut from the sorted order
hipError_t launch_hit_layers(const DParams &P, const double *rays, unsigned long long n, uint32_t max_layers, void *hits, double *along, void *id, uint32_t *count,
                             double *inside, const uint32_t *tri_base, const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t hit_layers_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t hit_layers_set_lds_limit(size_t bytes, bool ldss);
// k_attributes.hip: hit attributes (lg_hit_attributes*) -- query_kernel's closest form with the attribute planes of each hit behind its
// record (barycentrics, uv, local point, the BSDF's tangents, the geometric dpdu / dpdv; attr_resolve.h); only the planes that are not
// nullptr are written, indexed by the ray; perm != nullptr: the tiles are cut from the sorted order.  launch_attr_of (lg_hit_attributes_of*):
// no walk -- record i (lg_hit, DEVICE memory) names the primitive, checked against `counts` (attributes_host.h) before it is resolved
hipError_t launch_attributes(const DParams &P, const double *rays, unsigned long long n, void *hits, uint32_t *flags, double *bary, double *uv, double *local,
                             double *frame, double *dp, const uint32_t *tri_base, const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth,
                             hipStream_t stream);
hipError_t launch_attr_of(const DParams &P, const double *rays, const void *records, unsigned long long n, const uint32_t *counts, uint32_t *flags, double *bary,
                          double *uv, double *local, double *frame, double *dp, uint32_t blocks, hipStream_t stream);
hipError_t attributes_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t attributes_set_lds_limit(size_t bytes, bool ldss);
// k_closest.hip: closest points (lg_closest_points*) -- for each point the nearest surface point of the scene, a 64-point tile per wave and a
// point per lane, a distance-ordered walk of the reference trees from the global tables with a per-lane stack of stack_depth (node, accel)
// entries in dynamic LDS; `cl`: the ClosestAccel table (closest_host.h), qmax the largest |q|_inf it prunes for, r2 = radius * radius; only
// the planes that are not nullptr are written
hipError_t launch_closest(const DParams &P, const double *points, unsigned long long n, double r2, double qmax, double *distance, double *point, void *id,
                          const uint32_t *tri_base, const void *cl, uint32_t *tile_counter, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t closest_occupancy(uint32_t stack_depth, int *blocks_per_cu);
hipError_t closest_set_lds_limit(size_t bytes);
size_t closest_stack_bytes(uint32_t stack_depth);
struct ClosestTables; // closest_host.h
// k_nearest.hip: proximity queries (lg_nearest*) -- closest_kernel's walk keeping the k nearest candidates of each point in a per-lane list
// behind the stack in dynamic LDS (nearest_host.h, nearest_lds_bytes(stack_depth, k)), counting the candidates within the point's radius, or
// leaving at the first one: `form` is nearest_form(count asked for, a slot plane asked for); radii: nullptr for the shared radius
// (r2 = radius * radius); k: the list entries a lane keeps (0 without a slot plane); only the planes that are not nullptr are written
int nearest_form(bool count, bool slots);
hipError_t launch_nearest(const DParams &P, int form, const double *points, const double *radii, unsigned long long n, double r2, double qmax, uint32_t k, uint8_t *touch,
                          uint32_t *count, double *distance, double *point, void *id, const uint32_t *tri_base, const void *cl, uint32_t *tile_counter, uint32_t blocks,
                          uint32_t stack_depth, hipStream_t stream);
hipError_t nearest_occupancy(int form, uint32_t stack_depth, uint32_t k, int *blocks_per_cu);
hipError_t nearest_set_lds_limit(size_t bytes);
// k_segments.hip: segment proximity (lg_closest_segments*) -- closest_kernel's walk for a segment a lane (segment_prim.h's candidates, a
// segment-against-box pruning in two stages), the stack alone in dynamic LDS; touch_only: `touch` is the only plane asked for and a lane
// leaves at its first admissible candidate; radii: nullptr for the shared radius (r2 = radius * radius); only the planes that are not
// nullptr are written
hipError_t launch_segments(const DParams &P, bool touch_only, const double *segments, const double *radii, unsigned long long n, double r2, double qmax, uint8_t *touch,
                           double *distance, double *param, double *point, void *id, const uint32_t *tri_base, const void *cl, uint32_t *tile_counter, uint32_t blocks,
                           uint32_t stack_depth, hipStream_t stream);
hipError_t segments_occupancy(bool touch_only, uint32_t stack_depth, int *blocks_per_cu);
hipError_t segments_set_lds_limit(size_t bytes);
// k_paths.hip: ray paths (lg_trace_paths*) -- layers_kernel's loop with a direction update: at each hit the rule of its material (`rules`:
// n_rules lg_path_rule records in DEVICE memory) ends the path or forms the next segment in registers (bounce.h); only the planes that are
// not nullptr are written, vertex-major: element (j, i) at j * n + i; perm != nullptr: the tiles are cut from the sorted order
hipError_t launch_trace_paths(const DParams &P, const double *rays, unsigned long long n, uint32_t max_bounces, const void *rules, uint32_t n_rules, bool use_ns,
                              const uint32_t *start_medium, void *hits, double *point, void *id, double *along, uint32_t *count, uint32_t *end, double *gain, double *last,
                              uint32_t *medium, const uint32_t *tri_base, const uint32_t *perm, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t trace_paths_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t trace_paths_set_lds_limit(size_t bytes, bool ldss);
// k_features.hip: feature buffers (lg_capture_features*) -- the closest-hit walk of the camera's own rays, an 8 x 8 tile of the rectangle per
// wave and a pixel per lane; only the planes that are not nullptr are written, at DParams' output addressing (out_row0 / out_x0 / out_pitch)
hipError_t launch_features(const DParams &P, float *depth, float *normal, float *albedo, float *coverage, void *id, const double *material_rgb, uint32_t nmat,
                           const uint32_t *tri_base, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t features_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t features_set_lds_limit(size_t bytes, bool ldss);
// k_view_features.hip: view features (lg_capture_view_features*) -- features_kernel over the K cameras of a table: global pixel tile
// G = v * tiles_per_view + t per wave, a pixel per lane; only the planes that are not nullptr are written, film v's pixel at v * w * h + y * w + x
// (V.rgba / V.rgb are not used)
hipError_t launch_view_features(const DParams &P, const ViewArgs &V, float *depth, float *normal, float *albedo, float *coverage, void *id, float *point,
                                const double *material_rgb, uint32_t nmat, const uint32_t *tri_base, bool fast, uint32_t blocks, uint32_t stack_depth, hipStream_t stream);
hipError_t view_features_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu);
hipError_t view_features_set_lds_limit(size_t bytes, bool ldss);
hipError_t wf_trace_occupancy(uint32_t stack_depth, bool fast, size_t extra_lds, int *blocks_per_cu);
hipError_t launch_queue(const DParams &P, uint32_t blocks, hipStream_t stream);
hipError_t queue_occupancy(uint32_t stack_depth, size_t extra_lds, int *blocks_per_cu);
hipError_t queue_set_lds_limit(size_t bytes, bool ldss);
hipError_t mega_set_lds_limit(size_t bytes, bool ldss);
hipError_t wf_set_lds_limit(size_t bytes, bool ldss);
hipError_t launch_kat(int kind, const double *params, const float *vpos, const uint32_t *tri_v, uint32_t ntri, V3 o, V3 d, double *out,
                      hipStream_t stream);
hipError_t launch_kat_si(V3 o, V3 d, double t, V3 dpdu, V3 dpdv, double *out, hipStream_t stream);
hipError_t launch_math(int op, size_t n, const double *a, const double *b, double *out, hipStream_t stream);
hipError_t launch_trace_pixel(const DParams &P, bool fast, uint32_t stack_depth, uint32_t x, uint32_t y, double *out, hipStream_t stream);
hipError_t launch_probe_copy(const void *src, void *dst, size_t bytes, hipStream_t stream);
hipError_t launch_probe_lds(uint32_t blocks, uint32_t iters, uint32_t *sink, hipStream_t stream);
} // namespace lg

using namespace lg;

extern thread_local std::string tl_error; // devmem.cpp
extern int g_device;
extern bool g_device_chosen; // lg_set_device was called: single-device captures stay on that device
extern std::vector<int> g_devices; // lg_set_devices: the devices a host-film lg_capture is split over (empty = g_device)

inline int fail(const std::string &msg) {
    tl_error = msg;
    return 1;
}
#define HIP_TRY(expr)                                                                                                   \
    do {                                                                                                                \
        hipError_t _e = (expr);                                                                                         \
        if (_e != hipSuccess) throw Error(std::string(#expr) + ": " + hipGetErrorString(_e));                           \
    } while (0)

void use_device(int dev); // devmem.cpp
void use_device();

// A switch of the environment that is on unless its value begins with '0' (callers keep the answer in a static: once per process)
inline bool env_on(const char *name) { const char *e = std::getenv(name); return !(e && e[0] == '0'); }
// LASGUN_PRUNE=0|1 replaces the scene-dependent DEFAULT of the pruned walk (test suites run whole under either; -1: not set), for the launch
// (launch.cpp, base_params) and for the records the accel is built with (accel.cpp) alike; lg_accel_set_prune still wins
inline int prune_env() {
    static const int v = [] { const char *e = std::getenv("LASGUN_PRUNE"); return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1; }();
    return v;
}

// Device allocations of 1 KiB and more are recycled through a small per-process pool (at most 4 GiB parked per
// device): capture() builds and drops an accel -- film staging, per-pixel state -- for every frame, like the
// reference, and hipMalloc / hipFree of those buffers would otherwise cost about a millisecond of each frame.
// Nothing relies on the contents of a fresh buffer: every buffer is written (kernel, memset or copy) before it is read.
struct DevPool {
    std::mutex mtx;
    struct Block { int device; size_t bytes; void *p; };
    std::vector<Block> parked;
    size_t parked_bytes[64] = {0};
    static constexpr size_t MIN_BYTES = 1u << 10, CAP = 4ull << 30, MAX_BLOCKS = 256; // (from 1 KiB: the table arena, tile counters and queue counts of a frame are recycled too)
    // a parked block of at least `bytes` (and at most 1.25x that); *capacity receives its real size
    void *take(int device, size_t bytes, size_t *capacity) {
        std::lock_guard<std::mutex> g(mtx);
        size_t best = parked.size();
        for (size_t i = 0; i < parked.size(); ++i)
            if (parked[i].device == device && parked[i].bytes >= bytes && parked[i].bytes <= bytes + bytes / 4 &&
                (best == parked.size() || parked[i].bytes < parked[best].bytes)) best = i;
        if (best == parked.size()) return nullptr;
        void *p = parked[best].p;
        *capacity = parked[best].bytes;
        parked_bytes[device & 63] -= parked[best].bytes;
        parked.erase(parked.begin() + (long)best);
        return p;
    }
    bool park(int device, size_t bytes, void *p) {
        std::lock_guard<std::mutex> g(mtx);
        if (bytes < MIN_BYTES || parked_bytes[device & 63] + bytes > CAP || parked.size() >= MAX_BLOCKS) return false;
        parked.push_back(Block{device, bytes, p});
        parked_bytes[device & 63] += bytes;
        return true;
    }
    // give the parked blocks of `device` (or of every device: -1) back to the driver; returns the bytes freed.
    // The caller has made sure nothing on the device still uses them (blocks are parked only after a synchronise).
    size_t trim(int device) {
        std::vector<Block> drop;
        {
            std::lock_guard<std::mutex> g(mtx);
            for (size_t i = 0; i < parked.size();)
                if (device < 0 || parked[i].device == device) {
                    drop.push_back(parked[i]);
                    parked_bytes[parked[i].device & 63] -= parked[i].bytes;
                    parked.erase(parked.begin() + (long)i);
                } else ++i;
        }
        size_t freed = 0;
        int cur = 0;
        (void)hipGetDevice(&cur);
        for (const Block &b : drop) {
            if (hipSetDevice(b.device) == hipSuccess && hipFree(b.p) == hipSuccess) freed += b.bytes;
        }
        (void)hipSetDevice(cur);
        return freed;
    }
};
// never destroyed: buffers released at interpreter exit, after static destructors have begun, still find it
extern DevPool &g_pool; // devmem.cpp

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    size_t bytes_ = 0; // capacity in bytes (what the pool is told)
    int device_ = 0;
    bool borrowed_ = false; // a view into another DevBuf's allocation (TableStage): nothing to free
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    friend void swap(DevBuf &a, DevBuf &b) { std::swap(a.p, b.p); std::swap(a.n, b.n); std::swap(a.bytes_, b.bytes_); std::swap(a.device_, b.device_); std::swap(a.borrowed_, b.borrowed_); }
    void view(T *ptr, size_t count) { release(); p = ptr; n = count; borrowed_ = true; }
    void obtain(size_t bytes) {
        release();
        HIP_TRY(hipGetDevice(&device_));
        bytes_ = bytes;
        void *q = bytes >= DevPool::MIN_BYTES ? g_pool.take(device_, bytes, &bytes_) : nullptr; // bytes_: the block's real capacity
        if (!q) {
            hipError_t e = hipMalloc(&q, bytes);
            if (e == hipErrorOutOfMemory) { // the pool may be sitting on the memory: hand it back and try once more
                (void)hipGetLastError();
                g_pool.trim(device_);
                e = hipMalloc(&q, bytes);
            }
            if (e != hipSuccess) throw Error(std::string("hipMalloc(") + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
        }
        p = (T *)q;
    }
    void upload(const std::vector<T> &v) {
        obtain((v.size() ? v.size() : 1) * sizeof(T));
        n = v.size();
        if (n) HIP_TRY(hipMemcpy(p, v.data(), n * sizeof(T), hipMemcpyHostToDevice));
    }
    void alloc(size_t count) {
        obtain((count ? count : 1) * sizeof(T));
        n = count;
    }
    void release() {
        if (p && !borrowed_ && !g_pool.park(device_, bytes_, p)) (void)hipFree(p);
        p = nullptr; n = 0; bytes_ = 0; borrowed_ = false;
    }
    ~DevBuf() { release(); }
};
// A launch's buffer that is too small is allocated anew -- after a device-wide synchronise: nothing may still use the old one
template <class T> void grow(DevBuf<T> &buf, size_t need) {
    if (buf.n < need) { HIP_TRY(hipDeviceSynchronize()); buf.alloc(need); }
}

// The scene tables of an accel go to the device in ONE allocation and ONE copy: capture() builds an accel for every frame like the
// reference (lib.rs:64), and two dozen hipMalloc + hipMemcpy pairs of a few kilobytes each were a third of lg_accel_from's millisecond
// on the headline scene.  Tables of 256 KiB and more keep an allocation and a copy of their own (staging them would cost a host
// memcpy of megabytes); the rest are staged here, 256-byte aligned, and become views into `arena` at commit().
struct TableStage {
    std::vector<uint8_t> host;
    std::vector<std::function<void(uint8_t *)>> fix;
    template <class T> void add(DevBuf<T> &buf, const std::vector<T> &v) {
        const size_t bytes = v.size() * sizeof(T);
        if (bytes >= (256u << 10)) { buf.upload(v); return; }
        const size_t off = (host.size() + 255) & ~(size_t)255;
        host.resize(off + (bytes ? bytes : 1));
        if (bytes) std::memcpy(host.data() + off, v.data(), bytes);
        const size_t count = v.size();
        DevBuf<T> *b = &buf;
        fix.push_back([b, off, count](uint8_t *base) { b->view(reinterpret_cast<T *>(base + off), count); });
    }
    void commit(DevBuf<uint8_t> &arena) {
        arena.alloc(host.size() ? host.size() : 1);
        if (!host.empty()) HIP_TRY(hipMemcpy(arena.p, host.data(), host.size(), hipMemcpyHostToDevice));
        for (auto &f : fix) f(arena.p);
    }
};

// Streams are recycled per device as well: capture() makes an accel per frame, and creating its stream (and the copy stream of a
// banded capture) cost a tenth of a millisecond each.  A stream goes back when its accel dies; whatever it may still hold is ahead
// of the next owner's work in stream order.
struct StreamPool {
    std::mutex mtx;
    std::vector<std::pair<int, hipStream_t>> spare;
    hipStream_t take(int device) {
        {
            std::lock_guard<std::mutex> g(mtx);
            for (size_t i = 0; i < spare.size(); ++i)
                if (spare[i].first == device) { hipStream_t s = spare[i].second; spare.erase(spare.begin() + (long)i); return s; }
        }
        hipStream_t s = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return s;
    }
    void give(int device, hipStream_t s) {
        if (!s) return;
        {
            std::lock_guard<std::mutex> g(mtx);
            if (spare.size() < 64) { spare.emplace_back(device, s); return; }
        }
        (void)hipStreamDestroy(s);
    }
};
extern StreamPool &g_streams; // never destroyed (see g_pool)

// Pinned host staging for the small tables a *_device entry point uploads (a batch's k table, a lattice row table): the copy is
// enqueued on the caller's stream from memory that stays put until the copy is through, so the call only enqueues (round 5 used a blocking
// hipMemcpy, and a device-wide synchronise when a row table changed: ADVICE r5).  Blocks are powers of two, recycled per process.
struct PinnedPool {
    std::mutex mtx;
    std::vector<std::pair<size_t, void *>> spare;
    void *take(size_t bytes, size_t *capacity) {
        size_t cap = 4096;
        while (cap < bytes) cap <<= 1;
        *capacity = cap;
        {
            std::lock_guard<std::mutex> g(mtx);
            for (size_t i = 0; i < spare.size(); ++i)
                if (spare[i].first == cap) { void *q = spare[i].second; spare.erase(spare.begin() + (long)i); return q; }
        }
        void *q = nullptr;
        hipError_t e = hipHostMalloc(&q, cap, hipHostMallocPortable);
        if (e != hipSuccess) throw Error(std::string("hipHostMalloc(staging): ") + hipGetErrorString(e));
        return q;
    }
    void give(size_t cap, void *q) {
        if (!q) return;
        {
            std::lock_guard<std::mutex> g(mtx);
            if (spare.size() < 64) { spare.emplace_back(cap, q); return; }
        }
        (void)hipHostFree(q);
    }
};
extern PinnedPool &g_pinned; // never destroyed (see g_pool)
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    void need(size_t bytes) { if (cap < bytes) { g_pinned.give(cap, p); p = nullptr; cap = 0; p = g_pinned.take(bytes, &cap); } }
    ~PinnedBuf() { g_pinned.give(cap, p); }
};


// Sticky error words of the queue organisation (k_queue.hip: a wave that gave up waiting for work).  They live in PINNED HOST memory
// that every device writes straight into (system-scope store), one word per accel, handed out from pages of 1024: the host reads
// a word without a HIP call -- after any synchronise, at the head of every enqueue, in lg_accel_synchronize -- and only the host
// ever clears it, after it has reported it.  (Round 4 kept the word among the per-launch control words: the memset before the
// next chunk or supersample erased it, and a launch on a caller's stream was looked at before it had finished -- ADVICE r4.)
struct ErrWords {
    std::mutex mtx;
    std::vector<uint32_t *> pages;
    std::vector<uint32_t *> spare;
    uint32_t *take() {
        std::lock_guard<std::mutex> g(mtx);
        if (spare.empty()) {
            void *q = nullptr;
            hipError_t e = hipHostMalloc(&q, 4096, hipHostMallocPortable | hipHostMallocMapped);
            if (e != hipSuccess) throw Error(std::string("hipHostMalloc(error words): ") + hipGetErrorString(e));
            std::memset(q, 0, 4096);
            pages.push_back((uint32_t *)q);
            for (int i = 1023; i >= 0; --i) spare.push_back((uint32_t *)q + i);
        }
        uint32_t *w = spare.back();
        spare.pop_back();
        *(volatile uint32_t *)w = 0u;
        return w;
    }
    void give(uint32_t *w) {
        if (!w) return;
        std::lock_guard<std::mutex> g(mtx);
        spare.push_back(w);
    }
};
extern ErrWords &g_err_words; // never destroyed (see g_pool)

struct lg_scene {
    Scene s;
};
struct lg_aggregate {
    Aggregate a;
};
struct lg_film {
    uint32_t w = 0, h = 0;
    std::vector<uint8_t> owned;
    uint8_t *px = nullptr;
};

struct lg_accel {
    const Scene *scene = nullptr;
    int device = 0; // the HIP device this accel's tables and launches live on
    FlatScene flat;
    DevBuf<uint8_t> arena; // the small tables live here (TableStage); the DevBufs below are views into it or allocations of their own
    DevBuf<DNode> nodes;
    DevBuf<DNode4> nodes4;
    DevBuf<uint32_t> primref;
    DevBuf<DSphere> spheres;
    DevBuf<int32_t> sphere_mat;
    DevBuf<DCuboid> cuboids;
    DevBuf<int32_t> cuboid_mat;
    DevBuf<uint32_t> tri_v, tri_n, tri_t;
    DevBuf<float> vpos, vnorm, vtex;
    DevBuf<DLeafRec> leaf_soup;
    DevBuf<DChunk> chunks;
    DevBuf<DStrip> strips;
    DevBuf<uint32_t> sphere_ref_leaf, cuboid_ref_leaf, tri_ref_leaf, accel_ref_leaf;
    DevBuf<DAccel> accels;
    DevBuf<DMaterial> materials;
    DevBuf<DLight> lights;
    DevBuf<uint32_t> accel_tri_base; // ray queries only (k_query.hip): per accel, its mesh's first triangle (FlatScene::accel_tri_base)
    DevBuf<uint32_t> attr_counts;    // lg_hit_attributes_of* only (k_attributes.hip): what a record may name (attributes_host.h, attr_counts_build)
    // the frame table of flat triangles (tri_frames_host.h: the plan; k_tri_frames.hip fills it at the build; DParams::tri_frames)
    DevBuf<DTriFrame> tri_frames;
    DevBuf<DTriFrameJob> tri_frame_jobs; // the build kernel's list, one entry per record
    DevBuf<uint32_t> tri_frame_base;     // per accel: its first record, NO_HIT where it has none
    uint32_t tri_frame_records = 0;      // records of the table; 0: the accel holds none
    // lg_closest_points* only (k_closest.hip): the gate's verdict, the stack depth and the pruning test's constants per accel (closest_host.h),
    // made from `flat` and uploaded at the accel's first such call -- no part of the tables lg_accel_from builds or lg_accel_info counts
    mutable std::shared_ptr<ClosestTables> closest;
    mutable DevBuf<uint8_t> closest_cl;
    // launch resources (mutable: a `const lg_accel*` render call still enqueues work).  Everything a launch
    // scribbles on lives in a per-STREAM context, so launches of one accel on different streams (frame k+1's
    // primary pass filling the tail of frame k's shadow pass) do not share tile counters or per-pixel state.
    struct LaunchCtx {
        hipStream_t key = nullptr;
        unsigned long long last_use = 0;
        DevBuf<uint32_t> tile_counter;                         // [0] next tile; one head per XCD band behind it (TILE_COUNTER_WORDS)
        DevBuf<double> frames, stash;                          // megakernel: Whitted frame stack, parked shading frame
        DevBuf<uint8_t> wf_mem;                                // wavefront pipeline: every per-level array of a chunk, carved from one allocation
        DevBuf<uint32_t> wf_counters;                          // its queue counts and per-launch tile counters
        DevBuf<double> film_li;                                // ray films of several samples per pixel (lg_capture_rays*): every ray's li, 24 bytes a ray, until the resolve pass; grown on demand
        DevBuf<double> gather_li;                              // radiance gathers without a radiance plane (lg_radiance_gather*): a batch's li, 24 bytes a ray, until its resolve pass; grown on demand
        DevBuf<uint8_t> sort_mem;                              // ray queries in sorted order (k_sort.hip): ping-pong keys and indices, histograms; grown on demand
        // strided subsets by lattice column (shade.h, modes 4 / 5): (floor(y*w / n), (y*w) mod n) per film row -- one table per (w, h, n), the
        // last MAX_ROW_TABLES of them kept (a caller that alternates periods or films on one stream finds each again), each uploaded from
        // pinned staging of its own on the context's stream (`up`: that copy is through; the staging may be rewritten)
        struct RowTable { uint32_t w = 0, h = 0; unsigned long long n = 0, last_use = 0; DevBuf<DRowTab> buf; PinnedBuf stage; hipEvent_t up = nullptr; };
        std::vector<std::unique_ptr<RowTable>> rowtabs;
        unsigned long long rowtab_clock = 0;
        // lg_capture_subsets: the k tables of the batches in flight on this stream (addressing mode 3), each with the event that says
        // its launch is through -- a table is copied (from pinned staging of its own, on the stream) into a buffer of its own before its
        // launch is enqueued, so neither a later batch on the stream nor the caller's freed array can reach it
        struct KsTable { DevBuf<unsigned long long> buf; PinnedBuf stage; hipEvent_t done = nullptr; };
        std::vector<std::unique_ptr<KsTable>> ks_live;
        ~LaunchCtx() {
            for (auto &k : ks_live) if (k->done) (void)hipEventDestroy(k->done);
            for (auto &r : rowtabs) if (r->up) (void)hipEventDestroy(r->up);
        }
    };
    mutable std::vector<std::unique_ptr<LaunchCtx>> ctxs;
    // wavefront pipeline, big launches: the frame is cut into bands rendered on internal streams (each with a launch context
    // of its own), so one band's closest pass fills the tails of another band's shadow and shade passes and the sparse deeper
    // levels of a recursive scene run beside other bands' level 0 (enqueue_wavefront)
    mutable std::vector<hipStream_t> aux_streams;
    mutable std::vector<hipEvent_t> aux_done;
    mutable hipEvent_t aux_fork = nullptr;
    mutable unsigned wf_split = 0;               // lg_accel_set_wf_split: bands of a big wavefront launch (0 = LASGUN_WF_SPLIT, default 1)
    mutable unsigned long long ctx_clock = 0;
    mutable bool streaming = true; // use the streaming pipeline when the scene allows it
    mutable bool streaming_forced = false; // lg_accel_set_streaming(2): ignore the two criteria below (tests)
    // the pipeline pays for its per-pixel state traffic only where node / sphere / box traversal dominates a
    // ray's cost (tools/threshold_sweep.py): set from the scene by lg_accel_from
    bool streaming_pays = false;
    unsigned long long streaming_min_items = 1ull << 20;
    unsigned long long specular_small_items = 1ull << 20; // a glass / mirror scene resident in LDS: frames up to this many pixels go level by level
    bool mega_narrow = false;        // the LDS-resident megakernel in 768-lane workgroups: scenes of fewer than 512 spheres / boxes (measured, k_mega.hip)
    uint32_t wf_blocks = 1, wf_blocks_fast = 1;   // grids of the wavefront pipeline's 256-lane traversal kernels
    uint32_t queue_blocks = 1;                    // grid of the queue organisation's persistent kernel (256-lane form)
    mutable uint32_t *q_err = nullptr;            // the queue organisation's sticky error word (pinned host memory, g_err_words): taken at its first launch
    mutable int queue = -1;                       // lg_accel_set_streaming(3) forces the queue organisation, (0..2) rule it out; -1 = queue_default
    mutable int last_org = -1;                    // what the last launch ran as, encoded (choice.h); -1 before the first (lg_accel_last_organisation)
    mutable int tile_parts = -1;                  // lg_accel_set_tile_parts: the megakernel hands a tile out whole (1) or in 2 / 4 / 8 parts; -1 = whole unless the measured choice says quarters
    mutable int sample_order = -1;                // lg_accel_set_sample_order: 0 a pixel's samples side by side, 1 one after the other, -1 = side by side (megakernel: rule / measured)
    mutable int query_order = 0;                  // lg_accel_set_query_order: 0 a query's rays are walked as given, 1 sorted on the device by a coherence key (k_sort.hip)
    mutable int tile_order = -1;                  // lg_accel_set_tile_order: 0 top-down, 1 bottom-up, 2 from the middle row outwards, -1 = middle-out unless the measured choice says otherwise
    bool queue_default = false;                   // glass / mirror over a big mesh: long uneven walks, sparse deep levels (k_queue.hip)
    mutable size_t queue_budget = 0;              // bytes one launch context may hold for it (0 = from the free memory at first use)
    unsigned long long queue_min_items = 1ull << 16; // launches below this many pixels stay with the megakernel
    mutable size_t wf_budget = 0;                 // bytes one launch context may hold for it (0 = from the free memory at first use)
    // LDS-resident scene (reference tree only): the tables in their LDS layout, when they fit beside the stacks
    DevBuf<uint32_t> lds_image;
    DevBuf<uint32_t> accel_image;     // scenes in L2: the accel records alone, in their LDS layout (DParams::accel_image); empty: too many accels
    uint32_t accel_image_n16 = 0;
    uint32_t lds_image_n16 = 0, lds_node_off = 0, lds_prim_off = 0, lds_soup_off = 0, lds_accel_off = 0;
    // the level-0 closest pass's origin-relative form (dscene.h, DRelAccel): every accel's own node records and leaf slots in the image, origins
    // zero (launch.cpp fills them per launch); empty: more than L0_REL_MAX_ACCELS accels, or two accels share records (accel.cpp)
    std::vector<DRelAccel> l0_rel;
    mutable bool l0_relative = true;  // lg_accel_set_l0_relative
    mutable int last_l0_relative = -1; // the last level-0 closest launch of the level-by-level pipeline: 1 origin-relative, 0 absolute; -1 before the first
    // the pair form of that image (dscene.h, DParams::lds_pairs; pairs_host.h): lds_image holds pair records in place of the node records --
    // where the switch asks for them and every tree's ranges fit a child word (pair_refusal: why not, when the builder said no)
    bool lds_pairs = false;
    int image_prune = -2;             // rebuild_tables: the caller's lg_accel_set_prune setting while `prune` says which records the tables must hold (-2: `prune` itself)
    std::string pair_refusal;
    std::vector<std::array<uint32_t, 3>> pair_rel; // per accel: root record's byte offset, first pair record's, pair records (DParams::pair_rel)
    mutable bool node_pairs = true;   // lg_accel_set_node_pairs (a change re-makes the image: rebuild_tables)
    mutable int last_node_pairs = -1; // the last launch over the LDS-resident scene: 1 pair records, 0 node records; -1 before the first
    // the packet form of level 0's closest pass (packet.h; launch.cpp, packet_walk: the gate)
    mutable bool packet_walk = true;   // lg_accel_set_packet_walk
    mutable int last_packet_walk = -1; // the last level-0 closest launch of the level-by-level pipeline: 1 the packet form, 0 the per-lane walk; -1 before the first
    // the fused form of the camera's level 0 (k_wavefront.hip, FUSED; launch.cpp, fused_shade: the gate)
    mutable bool fused_shade = true;   // lg_accel_set_fused_shade
    mutable int last_fused_shade = -1; // the last chain of the level-by-level pipeline: 1 its level 0 took the fused form (two passes, no shade pass), 0 the three kernels; -1 before the first
    // the frame table in the fused packet closest pass (shade.h, shade_frame_tri; launch.cpp, tri_frames: the gate)
    mutable bool tri_frames_on = true; // lg_accel_set_tri_frames
    mutable int last_tri_frames = -1;  // the last chain of the level-by-level pipeline: 1 its level-0 closest launch read the table, 0 it did not; -1 before the first
    mutable int packet_scene = -1;     // the scene graph's part of the gate (packet_host.h, PacketRefusal), made at the first launch that asks; -1: not yet
    uint32_t ldss_blocks = 0;         // one 1024-lane workgroup per CU; 0 = variant unavailable for this scene
    uint32_t cus = 1;                 // compute units of the accel's device
    mutable bool lds_scene = true;    // lg_accel_set_lds_scene
    mutable DevBuf<DStats> stats;
    mutable DevBuf<uint8_t> staging;    // device film for host-film captures
    mutable DevBuf<double> staging_rad;
    mutable std::mutex mtx;
    hipStream_t stream = nullptr;
    uint32_t stack_depth = 1;      // reference traversal
    uint32_t stack_depth_fast1 = 1; // fast traversal (one word per pending child; also deep enough for its reference re-trace)
    uint32_t max_blocks = 1;
    uint32_t max_blocks_fast = 1;
    uint64_t device_bytes = 0;
    mutable bool profiling = false;
    mutable bool fast = false; // opt-in fast traversal mode (lg_accel_set_mode)
    mutable int prune = -1;    // lg_accel_set_prune: -1 = prune_default
    bool prune_default = false; // the scene carries a mesh with fat leaves
    mutable bool shadow_skip = true; // lg_accel_set_shadow_skip: the level-by-level closest pass flags hits whose shadow rays decide nothing
    mutable uint32_t level_door = 3u; // lg_accel_set_level_door: LEVEL_DOOR_* bits of the exact walk's enter block (walk.h, ST_ENTER)
    bool fast_available = true;
    std::string fast_refusal = "fast mode unavailable: its tree is too deep for the LDS stack";
    mutable std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    // streaming pipeline, per kernel kind: 0 primary trace, 1 frame, 2 shadow trace, 3 shade; 4 = megakernel
    mutable std::vector<std::pair<hipEvent_t, hipEvent_t>> kind_events[5];
    ~lg_accel() {
        for (auto &e : events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        for (auto &v : kind_events) for (auto &e : v) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        for (auto e : aux_done) (void)hipEventDestroy(e);
        if (aux_fork) (void)hipEventDestroy(aux_fork);
        for (auto st : aux_streams) g_streams.give(device, st);
        g_streams.give(device, stream);
        g_err_words.give(q_err);
    }
};

// the scene's tables are resident in LDS for this accel's launches (the reference walk; the kernels' 1024-lane forms)
// the effective setting of the pruned walk (launch.cpp, base_params): LASGUN_PRUNE=0|1 replaces the scene-dependent default, lg_accel_set_prune wins
inline bool prune_effective(const lg_accel &a) {
    const bool dflt = prune_env() < 0 ? a.prune_default : prune_env() != 0;
    return !a.fast && (a.prune < 0 ? dflt : a.prune != 0);
}
// (an image of pair records serves the plain exact walk alone: while the accel holds one, the pruned walk is launched from the L2 tables)
inline bool lds_resident(const lg_accel &a) { return !a.fast && a.lds_scene && a.ldss_blocks && !(a.lds_pairs && prune_effective(a)); }

constexpr size_t MAX_LAUNCH_CTXS = 8;
constexpr unsigned MAX_WF_BANDS = 4; // bands of a big wavefront launch on internal streams (lg_accel_set_wf_split)
constexpr size_t PRUNE_MIN_TRIS = 4096; // the pruned walk is the default from this many triangles in a mesh (accel.cpp; profiles/r05_prune_threshold.jsonl)

// ---- launch.cpp: one render enqueued (callers hold a.mtx and have made the accel's device current)
lg_accel::LaunchCtx &ctx_for(const lg_accel &a, hipStream_t stream);
void check_queue_error(const lg_accel &a);
void sync_checked(const lg_accel &a);
DParams base_params(const lg_accel &a, uint32_t w, uint32_t h);
void set_lds_scene(const lg_accel &a, DParams &P);
bool scene_lds_image(const Scene &scene, bool pairs, std::vector<uint32_t> &img, uint32_t info[8]); // accel.cpp: the LDS image of a scene alone, no device
// accel.cpp: the frame table's plan of a flattened scene (tri_frames_host.h), no device -- base[a] per accel, the table's records returned
uint32_t scene_tri_frames(const FlatScene &f, const Scene &scene, std::vector<uint32_t> &base);
void ensure_aux_streams(const lg_accel &a, unsigned n);
void enqueue(const lg_accel &a, DParams &P, bool stats, hipStream_t stream);
void enqueue_radiance(const lg_accel &a, const double *rays, size_t n, double *radiance, const uint32_t *perm, lg_accel::LaunchCtx &c, hipStream_t stream);
// One checked lg_radiance_groups* call: `groups` is the host table of n_groups entries (it travels by value in every launch's arguments)
void enqueue_radiance_groups(const lg_accel &a, const double *rays, size_t n, const DLightGroup *groups, uint32_t n_groups, double *radiance, const uint32_t *perm,
                             lg_accel::LaunchCtx &c, hipStream_t stream);
// One checked lg_scatter* call: Q's planes are the caller's device arrays (rays, perm, n, base and tri_base are set here)
void enqueue_scatter(const lg_accel &a, const double *rays, size_t n, ScatterArgs Q, const uint32_t *perm, lg_accel::LaunchCtx &c, hipStream_t stream);
// One checked lg_scatter_lit* call: Q's planes, and a per-ray light table, are the caller's device arrays; `shared` is the HOST table of a
// call whose lights are shared (staged here; Q.lights is set from it)
void enqueue_scatter_lit(const lg_accel &a, const double *rays, size_t n, LitArgs Q, const DLight *shared, const uint32_t *perm, lg_accel::LaunchCtx &c, hipStream_t stream);
void enqueue_ray_film(const lg_accel &a, const double *rays, size_t slots, uint32_t samples, const FilmArgs &film, const uint32_t *perm, lg_accel::LaunchCtx &c,
                      hipStream_t stream);
// One checked lg_radiance_gather* call on device tables (query.cpp; gather_host.h): batch_poses = n_poses where radiance is given
struct GatherCall {
    const double *origins, *frames, *dirs, *weights; // frames may be nullptr; weights where sums is given
    size_t n_poses, n_dirs, n_weights;
    bool pose_lanes;
    double *radiance, *sums;                         // either may be nullptr
    size_t batch_poses;                              // whole poses whose li is parked at a time (sums alone)
};
void enqueue_radiance_gather(const lg_accel &a, const GatherCall &g, lg_accel::LaunchCtx &c, hipStream_t stream);
// One checked lg_capture_views* call (query.cpp; views_host.h): `views` is the HOST table, copied through pinned staging into a device table of
// the call's own on `stream` before its launches; V.views and V.base_tile are set here
void enqueue_view_batch(const lg_accel &a, const DView *views, ViewArgs V, uint32_t samples_root, lg_accel::LaunchCtx &c, hipStream_t stream);
// ... and the staging alone, for a call that launches a kernel of its own over the table (lg_capture_view_features*): the device table
// of this call, released by subsets_enqueued() behind the launch or by subsets_abandoned() where the call fails before it
const DView *stage_view_table(const DView *views, size_t n_views, lg_accel::LaunchCtx &c, hipStream_t stream);
// ... and the same for the rule table of lg_trace_paths* (`bytes`: a multiple of 8), released the same way
const void *stage_rule_table(const void *rules, size_t bytes, lg_accel::LaunchCtx &c, hipStream_t stream);
void set_rect(DParams &P, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1);
unsigned long long subset_count(unsigned long long area, unsigned long long k, unsigned long long n);
void set_subset(const lg_accel &a, hipStream_t stream, DParams &P, size_t k, size_t n, uint32_t w, uint32_t h);
// Several subsets {k_j + i*n} of one n as ONE render (lg_capture_subsets): the k values sorted and without repeats or empty subsets,
// the periods the longest subset has, and whether the batch is every pixel of the film (every k of 0 .. n-1: the frame itself).
struct SubsetBatch {
    std::vector<unsigned long long> ks;
    unsigned long long n = 1, periods = 0, items = 0;
    bool whole = false;
};
SubsetBatch make_batch(const size_t *ks, size_t count, size_t n, uint32_t w, uint32_t h);
void set_subsets(const lg_accel &a, DParams &P, const SubsetBatch &b, hipStream_t stream);
void subsets_enqueued(const lg_accel &a, hipStream_t stream);
void subsets_abandoned(const lg_accel &a, hipStream_t stream);
// Which API call is running (the measured choice counts calls, not launches: tune.h): a scope at every entry from outside
struct CallScope {
    CallScope();
    ~CallScope();
};
template <class F> int guarded(F f) {
    try {
        CallScope call;
        f();
        return 0;
    } catch (const std::exception &e) {
        return fail(e.what());
    }
}

// ---- accel.cpp
void rebuild_tables(const lg_accel *ca, bool fast);
lg_accel *accel_from_on(const lg_scene *s, int device);
