/* include/lasgun_hip.h -- C ABI of liblasgun_hip.so, the MI355X-native drop-in for lasgun's
 * per-pixel ray-trace path.
 *
 * Every entry point in the CORE section replaces one item of the reference's public Rust
 * surface (file:line under nfrasser/lasgun); a Rust shim binds them 1:1.
 * Plain pointers and sizes only; no C++ exception ever crosses this boundary.  Functions that
 * can fail return nonzero / NULL and leave a message in lg_last_error() (thread-local).
 * Panics of the reference (empty aggregate, missing mesh handle, BVH stack overflow) become
 * such errors.  There is NO CPU fallback: without a usable HIP device every render call fails.
 *
 * Film layout (src/film.rs:22-45, src/img.rs:46-67): w*h pixels, row-major, top-left origin,
 * 4 bytes RGBA per pixel, A = 255.
 */
#ifndef LASGUN_HIP_H
#define LASGUN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_scene lg_scene;         /* src/scene.rs:11-40      Scene      */
typedef struct lg_aggregate lg_aggregate; /* src/scene/node.rs:25-33 Aggregate  */
typedef struct lg_accel lg_accel;         /* src/lib.rs:42           Accel<'s>  */
typedef struct lg_film lg_film;           /* src/film.rs:7-20        Film       */

/* src/material/mod.rs:3-10 -- `Material` is a Copy enum; here a tagged POD.
 * kind 0 Matte   p = kd[3], sigma
 * kind 1 Plastic p = kd[3], ks[3], roughness
 * kind 2 Metal   p = eta[3], k[3], u_roughness, v_roughness
 * kind 3 Glass   p = kr[3], kt[3], eta
 * kind 4 Mirror  p = kr[3] */
typedef struct lg_material {
    int32_t kind;
    double p[10];
} lg_material;

/* ------------------------------- CORE: the reference's surface ------------------------------ */
const char *lg_last_error(void);

lg_material lg_material_default(void);                                                        /* material/mod.rs:15 */
lg_material lg_material_matte(const double kd[3], double sigma);                              /* material/mod.rs:19 */
lg_material lg_material_plastic(const double kd[3], const double ks[3], double roughness);    /* material/mod.rs:24 */
lg_material lg_material_metal(const double eta[3], const double k[3], double u_roughness, double v_roughness); /* :30 */
lg_material lg_material_glass(const double kr[3], const double kt[3], double eta);            /* material/mod.rs:36 */
lg_material lg_material_mirror(const double kr[3]);                                           /* material/mod.rs:43 */

lg_scene *lg_scene_new(void);                                                                 /* scene.rs:50 */
void lg_scene_free(lg_scene *);
void lg_scene_set_perspective_camera(lg_scene *, double fov);                                 /* scene.rs:69 */
void lg_scene_set_orthographic_camera(lg_scene *, double scale);                              /* scene.rs:74 */
/* The Rust setters return `&mut Camera`; the camera lives in the scene, so these take the scene. */
void lg_camera_look_at(lg_scene *, const double origin[3], const double look[3], const double up[3]); /* camera.rs:85 */
void lg_camera_set_supersampling(lg_scene *, uint8_t base);                                   /* camera.rs:96 */
void lg_camera_set_aperture_radius(lg_scene *, double radius);                                /* camera.rs:100 */
void lg_scene_set_solid_background(lg_scene *, const double color[3]);                        /* scene.rs:79 */
void lg_scene_set_radial_background(lg_scene *, const double inner[3], const double outer[3], double scale); /* :83 */
void lg_scene_set_ambient_light(lg_scene *, const double color[3]);                           /* scene.rs:87 */
void lg_scene_set_mesh_smoothing(lg_scene *, int enabled);                                    /* scene.rs:91 */
void lg_scene_set_max_recursion_depth(lg_scene *, uint32_t max_depth);                        /* scene.rs:95 */
void lg_scene_set_threads(lg_scene *, size_t threads);                                        /* scene.rs:99: caps the devices of lg_set_devices */
void lg_scene_add_point_light(lg_scene *, const double position[3], const double intensity[3], const double falloff[3]); /* :103 */
int lg_scene_parse_obj(lg_scene *, const char *text, size_t len, uint32_t *out_ref);          /* scene.rs:120 -> Result */
int lg_scene_load_obj(lg_scene *, const char *path, uint32_t *out_ref);                       /* scene.rs:127 -> Result */
lg_aggregate *lg_scene_root(lg_scene *);                   /* `scene.root` (pub field, scene.rs:14): BORROWED */
void lg_scene_set_root(lg_scene *, lg_aggregate *moved);   /* scene.rs:132: takes ownership */

lg_aggregate *lg_aggregate_new(void);                                                         /* node.rs:36 */
void lg_aggregate_free(lg_aggregate *);                    /* only for aggregates never moved into a scene/group */
void lg_aggregate_add_group(lg_aggregate *, lg_aggregate *moved);                             /* node.rs:49 */
void lg_aggregate_add_sphere(lg_aggregate *, const double center[3], double radius, const lg_material *); /* node.rs:53 */
void lg_aggregate_add_cube(lg_aggregate *, const double origin[3], double dim, const lg_material *);      /* node.rs:58 */
void lg_aggregate_add_box(lg_aggregate *, const double minbound[3], const double maxbound[3], const lg_material *); /* :63 */
void lg_aggregate_add_obj(lg_aggregate *, uint32_t mesh);                                     /* node.rs:70 */
void lg_aggregate_add_obj_of(lg_aggregate *, uint32_t mesh, const lg_material *);             /* node.rs:75 */
void lg_aggregate_swap_backface(lg_aggregate *);                                              /* node.rs:80 */
void lg_aggregate_translate(lg_aggregate *, const double delta[3]);                           /* node.rs:85 */
void lg_aggregate_scale(lg_aggregate *, double x, double y, double z);                        /* node.rs:91 */
void lg_aggregate_rotate_x(lg_aggregate *, double theta_deg);                                 /* node.rs:96 */
void lg_aggregate_rotate_y(lg_aggregate *, double theta_deg);                                 /* node.rs:101 */
void lg_aggregate_rotate_z(lg_aggregate *, double theta_deg);                                 /* node.rs:106 */
void lg_aggregate_rotate(lg_aggregate *, double theta_deg, const double axis[3]);             /* node.rs:111 */

lg_film *lg_film_new(uint32_t width, uint32_t height);                     /* film.rs:24 (zero-filled) */
lg_film *lg_film_wrap(uint32_t width, uint32_t height, uint8_t *rgba);     /* film.rs:36 new_with_output: caller owns rgba */
uint8_t *lg_film_pixels(lg_film *);
uint32_t lg_film_width(lg_film *);
uint32_t lg_film_height(lg_film *);
void lg_film_free(lg_film *);

/* Accel::from(&scene) (lib.rs:42, bvh.rs:135): builds the nested HLBVH on the host exactly as
 * the reference does, flattens it and uploads it to HBM.  Borrows `scene` until lg_accel_free. */
lg_accel *lg_accel_from(const lg_scene *);
void lg_accel_free(lg_accel *);

/* capture(&scene, &mut film) (lib.rs:55-104): builds the accel, renders every pixel, returns when the film is written.  Devices: the
 * ones named with lg_set_devices / lg_set_device; a process that named none gets EVERY visible device for films of 2^18 pixels and
 * more (the reference takes every core, lib.rs:58-62; `scene.threads` caps the count) -- one accel per device, one RCCL gather --
 * and the HIP current device for smaller films (an accel and a communicator per GPU would cost more than the render). */
int lg_capture(const lg_scene *, lg_film *);                                       /* lib.rs:55 */
/* capture_subset(k, n, &accel, &mut img) (lib.rs:110-162): exactly the pixels {k + i*n < w*h} of the row-major film, no other byte touched;
 * callable over and over on one film (www/renderer.ts:103-120).  Which lane renders which pixel of the subset is the build's business: for
 * 8 <= n <= width a 64-lane tile is 64 rows of one LATTICE COLUMN of the subset (x = (k - y*w) mod n + n*c) -- the densest 64 pixels there are --
 * instead of 64 consecutive i, a strip n*64 pixels long (LASGUN_SUBSET_LATTICE=0: the latter). */
int lg_capture_subset(size_t k, size_t n, const lg_accel *, lg_film *);            /* lib.rs:110 */
lg_film *lg_render(const lg_scene *, uint32_t width, uint32_t height);             /* lib.rs:46 */

/* ----------------------- EXTRAS: no counterpart in the reference ---------------------------- */
typedef struct lg_stats { /* deterministic work counters of one render (stats kernel variant) */
    uint64_t primary_rays, shadow_rays, secondary_rays, nodes_tested, spheres_tested, cuboids_tested, triangles_tested,
        accel_entries, hits;
} lg_stats;

int lg_set_device(int device);      /* HIP device new accels are created on (default 0) */
int lg_device_count(void);
/* Device allocations of 1 MiB and more are recycled through a small per-process pool (at most 4 GiB parked per device;
 * flushed automatically when an allocation runs out of memory).  lg_trim_pool gives the parked blocks of `device`
 * (-1: of every device) back to the driver and returns the number of bytes freed. */
uint64_t lg_trim_pool(int device);
/* Devices a host-film lg_capture / lg_render is split over, one host thread per device -- the counterpart
 * of the reference's split over `scene.threads` CPU threads (lib.rs:58-104): count == 0 selects every visible
 * device; a non-zero `scene.threads` caps how many of them are used.  Each device renders the 64-row blocks
 * {r, r+n, ...} of the film (contiguous row tiles when the height is not a multiple of 64*n) from its own copy
 * of the scene and copies them straight into the host film; there is no inter-device traffic.  Until this is
 * called, lg_capture uses the one device of lg_set_device.  An index may repeat (its shares then run
 * concurrently on that device).  lg_accel handles stay bound to the device they were created on. */
int lg_set_devices(const int *device_ids, int count);

/* Accel::from on a given device (lg_accel_from uses the device of lg_set_device). */
lg_accel *lg_accel_from_on(const lg_scene *, int device);

/* ONE film on several GPUs of this process, gathered over xGMI -- the node-level counterpart of the reference's fan-out
 * over threads (lib.rs:55-104).  lg_multi_create builds the scene's accel on every device of the list (device_ids[0] is
 * the ROOT) and, when the list names more than one distinct device, one RCCL communicator per device (ncclCommInitAll;
 * RCCL is dlopen'ed at that moment, never for single-device use).  A capture renders rank r's share on its device --
 * the `block_rows`-row blocks {r, r+n, ...} when the height is a multiple of block_rows * n (64 balances the load to a few
 * per cent), contiguous row tiles otherwise or when block_rows is 0 -- and then moves every share with ONE grouped RCCL
 * exchange (ncclSend on the owners, ncclRecv on the root, inside one ncclGroupStart / ncclGroupEnd) straight to its place
 * in the film in the ROOT's device memory; the root's own contiguous tile is rendered in place.  A device may repeat in the
 * list (its shares are then copied device-locally): that is how a 1-GPU box rehearses the split; with the environment
 * variable LASGUN_MULTI_FORCE_RCCL=1 such shares travel through RCCL as well (send / recv to self).
 * lg_multi_capture_device: dev_rgba is width*height*4 bytes on the root device; synchronous.  lg_multi_capture: the
 * same into a host film (+ one D2H copy).  The scene must outlive the lg_multi. */
typedef struct lg_multi lg_multi;
lg_multi *lg_multi_create(const lg_scene *, const int *device_ids, int count, uint32_t block_rows);
void lg_multi_free(lg_multi *);
int lg_multi_capture_device(lg_multi *, uint32_t width, uint32_t height, void *dev_rgba_on_root);
int lg_multi_capture(lg_multi *, lg_film *);
/* The all-gather form: EVERY rank's device receives the whole film -- dev_rgba[r] is width*height*4 bytes on
 * rank r's device.  One ncclAllGather per device inside one group; contiguous tiles arrive in row order, interleaved blocks are
 * put in row order by n strided device copies.  One device per rank (no repeats); the height must split evenly.  Synchronous. */
int lg_multi_capture_device_all(lg_multi *, uint32_t width, uint32_t height, void *const *dev_rgba);
int lg_multi_rank_count(const lg_multi *);
lg_accel *lg_multi_accel(const lg_multi *, int rank);   /* rank's accel (to select traversal mode / organisation per rank) */
int lg_multi_uses_rccl(const lg_multi *);                /* 1 when a communicator was created */

/* Render image rows [y0, y1) of a width x height film straight into DEVICE memory, no host copy:
 * dev_rgba[0] is pixel (0, row0) of the image.  `hip_stream` is the hipStream_t to enqueue on,
 * used as given (NULL = HIP's default stream, as everywhere in HIP; lg_accel_stream() = the
 * accel's own non-blocking stream); the call only enqueues.  One stream at a time per accel.  This is the multi-GPU row-tile entry point. */
int lg_capture_rows_device(const lg_accel *, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, uint32_t row0,
                           void *dev_rgba, void *hip_stream);
/* Balanced multi-GPU sharding: render the rows y with (y / block_rows) % n == r into a COMPACT
 * device tile of height/n rows (tile row vy <-> image row ((vy/block_rows)*n + r)*block_rows +
 * vy%block_rows).  height must be a multiple of block_rows*n. */
int lg_capture_interleaved_device(const lg_accel *, uint32_t width, uint32_t height, uint32_t block_rows, uint32_t n,
                                  uint32_t r, void *dev_rgba, void *hip_stream);
/* capture_subset into a full width*height device film (pixels outside the subset untouched). */
int lg_capture_subset_device(size_t k, size_t n, const lg_accel *, uint32_t width, uint32_t height, void *dev_rgba,
                             void *hip_stream);
/* SEVERAL subsets {ks[j] + i*n} of one n as ONE render: the pixels written are exactly those of the `count` calls
 * lg_capture_subset(ks[j], n, ...) and no others (repeated k values count once, a k behind the film is an empty subset, as at
 * lib.rs:152).  No counterpart in the reference: its progressive caller (www/renderer.ts:103-120) calls capture_subset a hundred times
 * in a row, and a launch chain per call fills a fraction of a GPU; a batch costs count/n of a frame, and the batch of every k of
 * 0 .. n-1 IS the frame.  Host film: one D2H copy per batch; device film: only enqueues on `hip_stream`, like the calls above. */
int lg_capture_subsets(const size_t *ks, size_t count, size_t n, const lg_accel *, lg_film *);
int lg_capture_subsets_device(const size_t *ks, size_t count, size_t n, const lg_accel *, uint32_t width, uint32_t height,
                              void *dev_rgba, void *hip_stream);
void *lg_accel_stream(const lg_accel *);      /* the accel's own hipStream_t */
int lg_accel_synchronize(const lg_accel *);    /* hipStreamSynchronize(lg_accel_stream()) */

/* f64 radiance before quantisation for subset (k, n); rgb = width*height*3 doubles on the HOST,
 * pixels outside the subset are left untouched. */
int lg_capture_radiance(size_t k, size_t n, const lg_accel *, uint32_t width, uint32_t height, double *rgb);
/* Any list of pixels (offset = y * width + x < width * height) of a width x height film; results are compact and in
 * list order on the HOST: rgba_out[4*i..] and / or rgb_out[3*i..] (f64 radiance before quantisation) for offsets[i];
 * either output may be NULL.  For samples and crops of films too large to move whole (tests, tooling). */
int lg_capture_pixels(const lg_accel *, uint32_t width, uint32_t height, const uint64_t *offsets, size_t count,
                      uint8_t *rgba_out, double *rgb_out);
/* The crop [x0, x1) x [y0, y1) of a width x height film, compact and row-major on the HOST (either output may be NULL). */
int lg_capture_rect(const lg_accel *, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                    uint8_t *rgba_out, double *rgb_out);
/* Work counters for rendering rows [y0, y1) (runs the counting kernel variant once). */
int lg_capture_stats(const lg_accel *, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, lg_stats *out);

/* Audit of the pruned reference walk (lg_accel_set_prune) on real data: rows [y0, y1) are rendered once
 * with the counting variant of the pruned walk, and every node and every run of triangles it SKIPS (although the reference's own
 * box test passes) is also walked the reference's way.  A primitive found there that the reference would have ACCEPTED at that
 * moment -- `t < isect.t` for a closest-hit ray (sphere.rs:86, cuboid.rs:95, triangle.rs:251), t < 1 for a shadow ray
 * (point.rs:49) -- is a violation of the property the walk's exactness rests on: `violations` must be 0.  For the others,
 * (t - limit) / margin is sampled (margin: the skipping rule's own, eps' * |1/d_axis|): min_slack_* = how far beyond the limit the
 * nearest skipped primitive was (+inf: no sample; a box whose own plane parameter IS the slab entry sits at 1 + a rounding).  Reference traversal only (not the fast mode); the pruned walk is forced
 * on for this render whatever the accel's setting. */
typedef struct lg_prune_audit {
    uint64_t skipped_nodes, skipped_runs, primitives, violations;
    double min_slack_nodes, min_slack_runs;
    double max_margin_used_nodes; /* largest (slab entry parameter - t) / margin over the primitives under skipped nodes: the share of the
                                   * shipped margin that property (P) actually needed on this scene (1 would be the edge of a violation) */
} lg_prune_audit;
int lg_audit_prune(const lg_accel *, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, lg_prune_audit *out);
/* The same for the opt-in FAST mode (lg_accel_set_mode(1)), end to end: every ray of rows [y0, y1) -- primary, shadow and secondary, as the
 * render generates them -- is traced by the fast walk as shipped (its trees, its pruning, its candidate check and tie fallback) AND by the
 * reference walk, and the answers are compared on the device: the same primitive in the same accel at the same t, bit for bit, for a
 * closest-hit ray; the same `t < 1` verdict for a shadow ray (point.rs:49).  `violations` must be 0 for the film to be the reference's;
 * `fallbacks` counts the rays the fast walk itself sent to the reference walk (exact ties, winners the reference tree would not have tested).
 * Fast mode's margins are argued, not derived: this is its measurement, frame by frame.  The accel must be in fast mode. */
typedef struct lg_fast_audit { uint64_t rays, fallbacks, violations; } lg_fast_audit;
int lg_audit_fast(const lg_accel *, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, lg_fast_audit *out);

/* Traversal mode of an accel.  0 (default) = the reference's own traversal over the reference's
 * own BVH: the parity path.  1 = opt-in FAST mode: a binned-SAH BVH (one primitive per leaf)
 * over the same primitives, front-to-back with pruning beyond the best hit; same primitive tests
 * and arithmetic.  Its winner is put to the reference tree's own box tests (leaf to root, through every
 * nested accel); a winner that fails them, or an exact tie in t, re-traces the ray with the reference
 * traversal.  Verified byte-identical to mode 0 on every test and benchmark config; its two rounding margins are argued, not
 * PROVEN, and it CAN differ from the reference where a ray lies within rounding of a far triangle's plane (DESIGN.md section 3.3:
 * 5 pixels in 4,100 fuzz scenes whose meshes span ten orders of magnitude).  Refused -- non-zero return, lg_last_error -- for a scene with a
 * transform that does not invert (rotate() about a non-unit axis) or a mesh whose largest |coordinate| exceeds 2^20 times the longest
 * edge of its smallest triangle.  The fast trees cost 5-10x the
 * reference build, so lg_accel_from does not build them: the first lg_accel_set_mode(accel, 1) does (it
 * synchronises the device and uploads the tables again; the Scene must still be alive, as for any use of the accel). */
int lg_accel_set_mode(const lg_accel *, int mode);
/* Pruned form of the reference traversal (mode 0 only): the reference's tree and visit order, but a node is skipped when on
 * some axis the ray reaches its slab only beyond the best accepted hit (closest hit) or beyond the light (shadow rays) by
 * more than a margin derived from the rounding of the reference's own intersection formulas: every
 * primitive below such a node would be rejected by the reference's `t >= isect.t` (sphere.rs:86, cuboid.rs:95,
 * triangle.rs:251), so every pixel is what the unpruned walk gives.  Nodes over a nested BVHAccel are never skipped; inside a
 * mesh only the ray's dominant axis counts.  -1 (default): on for scenes that carry a mesh of >= 4096 triangles (the
 * reference's 254-triangle leaves are where it pays; below that it measured 5-30 % slower and its leaf records are a third to a half of
 * the accel build: profiles/r05_prune_threshold.jsonl -- rounds 3-5 had 256), off otherwise; 0 / 1: off / on (1 on an accel whose
 * tables were built without the leaf records builds them then). */
int lg_accel_set_prune(const lg_accel *, int enabled);
/* Level-by-level pipeline: the closest pass flags the hits at which no light can contribute whether or not it is visible -- BSDF::f is
 * exactly zero when the light and the viewer are on opposite sides of the geometric normal, so the light's term is +-0 either way -- and
 * the shadow pass does not walk them.  Exact; applies to scenes of 1 .. 32 lights of finite intensity.  1 (default):
 * on; 0: every hit's shadow rays are walked (A/B, tests; LASGUN_SHADOW_SKIP=0 does the same for every accel).  Same bytes either way. */
int lg_accel_set_shadow_skip(const lg_accel *, int enabled);
/* Exact walk, where a ray reaches a nested accel (a group or a mesh): bit 0 -- one row of the accel's inverse transform and one axis of
 * its root box are tried first, and a ray that has that whole slab behind it does not enter (the root box's own test would say so); bit 1 --
 * a group that holds one untransformed mesh and nothing else is walked as one level with it.  Both exact; the
 * counting forms (lg_capture_stats*, lg_trace_pixel*) and the fast mode never take them.  3 (default): both; 0 .. 3: as given (A/B, tests;
 * LASGUN_LEVEL_DOOR=0..3 masks every accel's setting).  Same bytes, hit records and visibility bits with every mask. */
int lg_accel_set_level_door(const lg_accel *, int mask);
/* Level-by-level pipeline, level 0's closest pass over an LDS-resident scene: every ray of a perspective camera leaves from the same point,
 * so the workgroup that has copied the scene into LDS subtracts that point from the node boxes and sphere centres once, in LDS, instead of
 * every lane at every test -- the same subtraction on the same bits.  Taken only where that holds in every bit: a
 * perspective camera (pixel_separation == 0) whose origin, and whose origin in every accel's local space, is finite with no -0 component,
 * finite up / aux, at most 16 accels, the plain exact walk.  1 (default): on; 0: the absolute form (A/B, tests; LASGUN_L0_RELATIVE=0 does
 * the same for every accel).  Same bytes either way.  lg_accel_last_l0_relative: the form the last such launch took (1 / 0; -1 before the
 * first).  lg_scene_l0_relative_origins: the device-free part of the gate for a scene and its own camera -- returns the number of accels and
 * writes the camera's origin in each accel's local space to origins[3 * accel ..] (at most `cap` accels), 0 where the gate says no, -1 on an error. */
int lg_accel_set_l0_relative(const lg_accel *, int enabled);
int lg_accel_last_l0_relative(const lg_accel *);
int lg_scene_l0_relative_origins(const lg_scene *, double *origins, int cap);
/* The exact walk from LDS, two boxes a trip: the LDS image of an accel whose tables fit there holds one 112-byte
 * PAIR record per interior node -- its two children's boxes and a typed word per child -- and one root record per tree in place of the
 * node records.  Every kernel that walks the plain exact form (not fast, not pruned) from LDS tests both children of a node in one trip and
 * pushes only a far child that is hit: the same box tests on the same operands, each at most once per ray, the leaves in the reference's
 * order.  1 (default): on where every tree's slot ranges fit a child word and the accel does not render pruned; 0: the node records (A/B,
 * tests; LASGUN_NODE_PAIRS=0 does the same for every accel).  A change re-makes the image with the accel's tables.  Same bytes either way.
 * lg_accel_last_node_pairs: the records the last launch over the LDS-resident scene read (1 pair / 0 node; -1 before the first). */
int lg_accel_set_node_pairs(const lg_accel *, int enabled);
int lg_accel_last_node_pairs(const lg_accel *);
/* The packet form of that walk: level 0's closest pass of the level-by-level pipeline walks the 64 rays of a wave
 * with one cursor, one stack and one slot counter; a lane takes part at a record exactly when it hit every ancestor of it, so its own
 * sequence of box and primitive tests is the per-lane walk's.  Taken where the launch takes the pair form, for the scene's own camera, and
 * every nested accel is a single root record entered from the root accel (a lone mesh and its group count as one).  1 (default): on;
 * 0: the per-lane walk (A/B, tests; LASGUN_PACKET_WALK=0 does the same for every accel).  Same bytes either way.
 * lg_accel_last_packet_walk: the form the last such launch took (1 / 0; -1 before the first). */
int lg_accel_set_packet_walk(const lg_accel *, int enabled);
int lg_accel_last_packet_walk(const lg_accel *);
/* The scene graph's part of that gate, without a device (tests): 0 where the packet form may take the scene, otherwise the reason it may
 * not (lasgun_amd/csrc/packet_host.h, PacketRefusal: 5 the root is a mesh, 6 a nested tree with interior nodes, 7 a nested accel inside a
 * nested accel, 8 a nested group's leaf holds another accel, 9 the root tree is deeper than the stack); -1 on an error. */
int lg_scene_packet_walk_gate(const lg_scene *);
/* The camera's level 0 of the level-by-level pipeline in its FUSED form: for a scene without recursion levels and
 * with exactly one light, where the closest launch takes the packet form and the shadow launch the pair form, the closest pass shades in
 * its epilogue (a hit whose shadow ray decides nothing is finished there; every other hit parks its point, the light's term and the
 * ambient term) and the shadow pass adds the light's term where the light is visible and writes the pixel: two passes, no shade pass.
 * Radiance queries, gathers, view batches, light groups, lit scatter and every other scene keep the three passes.  1 (default): on;
 * 0: the three passes (A/B, tests; LASGUN_FUSED_SHADE=0 does the same for every accel).  Same bytes either way.
 * lg_accel_last_fused_shade: the form level 0 of the last chain took (1 / 0; -1 before the first). */
int lg_accel_set_fused_shade(const lg_accel *, int enabled);
int lg_accel_last_fused_shade(const lg_accel *);
/* That form's gate for a scene, without a device (tests): 0 where a render by the scene's own camera (camera_level0 = 1) takes the form
 * with every switch at its default, otherwise the reason it does not (lasgun_amd/csrc/fused_host.h, FusedRefusal: 2 level 0 is not the
 * camera's, 3 more than one level, 4 not exactly one light, 5 the closest launch would not take the packet form, 6 the shadow launch
 * would not take the pair form); -1 on an error. */
int lg_scene_fused_shade_gate(const lg_scene *, int camera_level0);
/* The frame table of flat triangles: lg_accel_from makes, on the device, one record per triangle of every mesh
 * instance without vertex normals and with at most 1,024 triangles -- what a hit's shading frame holds that no ray enters: the normals
 * and tangents carried up the scene graph for both signs of the triangle's normal, and the material -- provided the accel's records are
 * at most 4,096 together.  The fused form's closest pass reads a hit's record instead of evaluating those expressions again; every other
 * kernel, and every hit without a record, evaluates them as before.  1 (default): on; 0: no launch reads the table (A/B, tests;
 * LASGUN_TRI_FRAMES=0 does the same for every accel).  Same bytes either way.
 * lg_accel_last_tri_frames: whether the level-0 closest launch of the last chain read the table (1 / 0; -1 before the first). */
int lg_accel_set_tri_frames(const lg_accel *, int enabled);
int lg_accel_last_tri_frames(const lg_accel *);
/* The table's plan for a scene, without a device (tests; lasgun_amd/csrc/tri_frames_host.h): returns the records an accel of the scene
 * would hold, 0 where it would hold no table; base[a] (may be NULL; at most `cap` written) is accel a's first record, 0xFFFFFFFF where
 * it has none; -1 on an error. */
int lg_scene_tri_frames_gate(const lg_scene *, uint32_t *base, int cap);
/* The table an accel holds, as its device made it (tests): up to `cap` records of 176 bytes into `records` (may be NULL) -- 21 doubles
 * c[3], ng0[3], ss[3], ns[2][3], ts[2][3] (the two variants: the triangle's normal as it is, and negated), then the material as an
 * int32 and a word of padding.  Returns the records the accel holds (0: no table), -1 on an error.  Synchronous. */
int lg_accel_read_tri_frames(const lg_accel *, void *records, int cap);
/* The LDS image lg_accel_from would make for this scene, without a device (tests): its 32-bit words into words[0 .. cap), info[8] = {16-byte
 * units, node offset, primref offset, leaf-record offset, accel-record offset (all in units), 1 if it holds pair records, accels, node
 * records of the flat tables}.  Returns the number of words, 0 when the tables do not fit in LDS, -1 on an error. */
int64_t lg_scene_lds_image(const lg_scene *, int pairs, uint32_t *words, size_t cap, uint32_t *info);
int lg_accel_get_prune(const lg_accel *); /* the effective setting (accel default, LASGUN_PRUNE, lg_accel_set_prune, fast mode): 0 / 1 */

/* Kernel organisation (same arithmetic, same bytes either way).  1 (default): the organisation of a launch is MEASURED -- the SECOND
 * API CALL that launches a kind in the process (the scene's shape, the device, the launch's size class and addressing mode) renders with
 * every organisation that can take it, on the caller's stream WITH THE HOST WAITING (this is the one place where a *_device entry point
 * blocks: once per kind; never on a stream that is being captured into a graph; pin choices with lg_tune_import, or set
 * LASGUN_AUTOTUNE=0, where that cannot be had), and the fastest is kept for the process (capture() rebuilds its accel per frame, so the
 * memory is keyed by the scene's shape); later launches of the kind only enqueue.  An organisation that cannot run (no memory for its
 * buffers) drops out of the measurement instead of failing the render.  The FIRST call that launches a kind -- all of its launches: the
 * four row bands of a big lg_capture, the shares of lg_multi_* -- takes the fitted rule's choice, so that a program that renders one
 * frame and exits pays nothing for a measurement worth 30-50 frames (LASGUN_AUTOTUNE=2: measure at the first call already --
 * benchmarks).  LASGUN_AUTOTUNE=0 keeps
 * the fitted rule of rounds 2-4 throughout: level by level in the WAVEFRONT pipeline (below) for scenes with <= 32 lights and at least
 * 512 spheres / boxes from 2^21 pixels a launch, and for a scene small enough to live in LDS glass / mirror frames of up to 2^20
 * pixels and plain frames of one sample per pixel from 2^18; the queue organisation for glass / mirror over a big mesh; the single
 * persistent megakernel for everything else.  0 = the megakernel only.
 * 2 = use the pipeline wherever it is possible (tests).
 * 3 = the QUEUE organisation wherever it is possible (reference traversal, <= 32 lights, recursion depth <= 7): ONE persistent
 * launch per chunk of the film whose waves pull 64-ray packets from per-level ray queues -- level 0's packets are the 8x8 pixel
 * tiles, level d + 1's are filled by level d's glass / mirror hits -- deepest level first, each packet taken through closest hit,
 * shadow rays and shading by the wave that claimed it; the levels are combined bottom-up as in the wavefront pipeline.  It is
 * the default for scenes with glass / mirror over a big mesh (long, uneven walks; sparse deep levels), where the megakernel
 * runs deep levels with a few lanes per wave and the level-by-level pipeline ends every launch with its slowest wave's tail.
 * Returns non-zero (lg_last_error) for any other value. */
int lg_accel_set_streaming(const lg_accel *, int enabled);
/* The table of measured choices from outside.  An entry is a kind of launch (twelve opaque words) and the choice remembered for it (the
 * encoding of lg_accel_last_organisation).  lg_tune_export writes up to `capacity` entries and returns how many the table holds
 * (out = NULL: just the count); lg_tune_import pins entries -- a kind that has one is never measured, and an entry the launch cannot
 * take (another build, less memory) falls back to the fitted rule's choice instead of failing; lg_tune_clear forgets every choice and
 * every first sight.  A caller that knows its workload exports once and imports at start-up; a test runs on a fixed table.
 * LASGUN_TUNE_FILE=<path> does the same without a line of code: the table is read from the file before the first look-up and rewritten after every
 * choice that is remembered, so a program that renders one frame and exits -- and therefore never measures -- runs on what an earlier run
 * (LASGUN_AUTOTUNE=2, or any program that rendered the kind twice) measured. */
typedef struct lg_tune_entry { uint64_t key[12]; int32_t choice; int32_t reserved; } lg_tune_entry;
size_t lg_tune_export(lg_tune_entry *out, size_t capacity);
int lg_tune_import(const lg_tune_entry *entries, size_t count);
void lg_tune_clear(void);
int lg_accel_last_organisation(const lg_accel *); /* what the accel's last launch ran as: 0 megakernel, 1 level by level, 2 queue, + 16 when its tiles were claimed bottom-up, + 64 when from the middle row outwards, + 128 when the megakernel handed its tiles out in parts, + 32 when the megakernel took a supersampled pixel's samples one after the other (otherwise side by side: every organisation's way since round 5); -1: none yet */
/* The direction in which the megakernel and the queue organisation claim a launch's 8x8 tiles: 0 = from the film's top (row order), 1 = from
 * its bottom, 2 = from its middle row outwards (what a frame shows tends to sit in its middle, and a launch should END on cheap tiles: the
 * 100k-triangle glass torus 36.2 -> 32.8 ms in the megakernel, profiles/r05_ab_tile_middle.jsonl), -1 (default) = middle-out unless the
 * measurement above finds another faster (a launch ends with the recursion trees of its last tiles: 6-9 % either way on scenes with
 * mirrors / glass, profiles/r05_ab_tile_order.jsonl).  Which tile is rendered when never changes a pixel. */
int lg_accel_set_tile_order(const lg_accel *, int order);
/* A supersampled pixel's samples (Camera::sample, camera.rs:113-146; integrate.rs:17-20 sums them in their order): 0 = SIDE BY SIDE -- a
 * launch's level-0 work items are (8x8 tile, sample) pairs, every sample's li() is parked as three doubles and a resolve pass sums each
 * pixel's samples in the reference's order, so the film is the same bytes; a 9-sample 512^2 frame then fills the machine nine times over
 * instead of running nine thin launch chains (level by level, queue) or nine samples in a row on each wave (megakernel): 1.2 - 10 x on the
 * reference's example scenes at their own sizes (profiles/r05_ss_par.jsonl).  1 = one sample after the other (rounds 1-4).  -1 (default) =
 * side by side, except that the megakernel's form is one more thing the measurement above times (frames of 1024^2 and more of a cheap
 * scene run faster with the samples in a row: a ninth of the tile claims). */
int lg_accel_set_sample_order(const lg_accel *, int order);
/* The work item of the megakernel and of the queue organisation's level 0: a whole 8x8 tile per wave (1), or a tile in 2 / 4 / 8 parts of
 * 32 / 16 / 8 lanes each.  A launch of fewer tiles than the grid has waves is as slow as its slowest tile's recursion tree; a part is a shorter
 * tree, four times the waves are at work, and the queue organisation's deeper packets stay as narrow (the 100k-triangle glass torus at 256^2
 * 8.46 -> 5.42 ms in the queue organisation, the metal torus 2.19 -> 1.81 in the megakernel; cheap scenes and big frames lose:
 * profiles/r05_ab_split.jsonl, r05_ab_split_orgs.jsonl).  -1 (default) = whole tiles unless the measurement above finds quarters faster for a small launch
 * (lg_accel_last_organisation: + 128).  Same bytes either way. */
int lg_accel_set_tile_parts(const lg_accel *, int parts);

/* The WAVEFRONT pipeline is li() level by level: per recursion level a closest-hit pass (hits compacted into a queue, misses
 * finished on the spot), an any-hit shadow pass and a shade pass that appends the specular children to the next level's ray
 * queue, then the levels are combined bottom-up in the reference's (output + reflected) + refracted order.  It serves every
 * scene, glass / mirror included.  (lg_accel_set_wavefront and lg_accel_set_packet -- the switches of round 1's three-kernel
 * pipeline and of the packet walk, both slower than this on every measured scene -- left the ABI in round 4.) */

/* Wavefront pipeline, launches of 2 Mpixel and more: cut the launch into `bands` row bands (2..8) rendered on internal streams,
 * each with launch state of its own, so one band's closest pass fills the tails of another band's shadow and shade passes
 * and the sparse deeper levels of a recursive scene run beside other bands' level 0; the caller's stream forks into them
 * and joins them, results are unchanged.  0 = the default (LASGUN_WF_SPLIT, else 1 = off).  Worth it for a caller that
 * renders one frame at a time (headline frame 7.79 -> 7.50 ms with 4 bands); a caller that keeps several frames in
 * flight on streams of its own already has that overlap and loses with it (7.20 -> 7.46 ms).  The internal streams overlap
 * only if the HIP runtime gives them hardware queues of their own (GPU_MAX_HW_QUEUES, default 4, counts every stream of
 * the process).  No counterpart in the reference. */
int lg_accel_set_wf_split(const lg_accel *, int bands);

/* LDS-resident scene (reference traversal; streaming pipeline and megakernel): when the scene's node,
 * primref, sphere and cuboid tables fit beside 1024 per-lane stacks in one CU's 160 KB of LDS, the
 * kernels that traverse run as one 1024-lane workgroup per CU that copies those tables into LDS once
 * and walks them there (same records, same arithmetic, same bytes out).  On by default; returns
 * 1 when the accel's scene qualifies, 0 when it does not (the setting is then without effect). */
int lg_accel_set_lds_scene(const lg_accel *, int enabled);


/* Kernel timing with HIP events on the launch stream: enable, render, then read. */
void lg_profile_enable(const lg_accel *, int enabled);
int lg_profile_read(const lg_accel *, double *total_ms, uint64_t *launches); /* synchronises; resets the tally */
/* Per-kernel HIP-event time.  kind 0 closest-hit trace (+ shading frame), 1 combine, 2 shadow trace, 3 shade; 4 = the megakernel
 * or the queue organisation's persistent kernel. */
int lg_profile_read_kinds(const lg_accel *, double ms[5], uint64_t launches[5]);
/* lg_capture_stats restricted to one kind of traversal: 0 all, 1 closest-hit (primary/secondary), 2 shadow. */
int lg_capture_stats_kind(const lg_accel *, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1, int kind, lg_stats *out);

/* Scene-structure introspection (tests) */
int lg_accel_dump(const lg_accel *, const double **f, size_t *nf, const int64_t **i, size_t *ni);
int lg_accel_info(const lg_accel *, uint64_t out[8]); /* nodes, primrefs, spheres, cuboids, triangles, accels, max_stack, bytes */
void lg_aggregate_get_transform(lg_aggregate *, double m[16], double minv[16]);
/* Host-only HLBVH build + flatten of a scene, no device needed: structure dump + counts
 * (nodes, primrefs, spheres, cuboids, triangles, accels, max_stack, has_specular). */
int lg_host_build_dump(const lg_scene *, const double **f, size_t *nf, const int64_t **i, size_t *ni, uint64_t info[8]);
/* Host-only self-check of the fast mode's wide node records against the binary fast trees they are collapsed from (no device):
 * out = { records, children, leaves reached, deepest stack of a walk that pushes every child but one, violations, the stack
 * depth the flattening reserved, 0, 0 }.  Violations: a child box not containing its node's box, a leaf reached twice or
 * never, a dangling link. */
int lg_host_check_wide_records(const lg_scene *, uint64_t out[8]);
/* Host-only self-check of the triangle strips the pruned walk's leaf loop streams (no device): out = { mesh leaves with culling
 * records, runs, triangles, strip entries, violations, FNV-1a of the culling records and the leaves' record words, FNV-1a of the strip
 * entries, 0 } (the hashes: the tables must not depend on how many host threads made them, LASGUN_HOST_THREADS).  Violations: a triangle of such a leaf that is not exactly one
 * strip triangle, a strip triangle whose three vertices are not its slot's three vertices, a run whose counts disagree. */
int lg_host_check_strips(const lg_scene *, uint64_t out[8]);

/* One pixel traced by a single lane (sample 0): out = { t, primref, accel instance, number of lights, then per light
 * the shadow ray's { t, primref }, then the shadow rays' origin (3) } -- primref is 4294967295 for "no hit"; out_len >=
 * 7 + 2 * lights.  `fast` selects the traversal mode.
 * With out_len >= 7 + 2 * lights + 16001 the event log of the primary ray's walk follows: a count, then up to 4000
 * events of 4 doubles (code, a, b, c: node pairs / nodes visited, primitive tests, accel entries and returns; the codes
 * are listed at lasgun_amd.HipApi.trace_pixel_log).  A debugging / test hook: it is how a film difference is traced
 * back to the ray, and the ray to the box, that caused it. */
int lg_trace_pixel(const lg_accel *, uint32_t width, uint32_t height, uint32_t x, uint32_t y, int fast, double *out, size_t out_len);

/* Ray queries: the caller's own rays through the render's BVH walk, in the accel's traversal mode (reference, pruned --
 * lg_accel_set_prune --, LDS-resident scene -- lg_accel_set_lds_scene --, opt-in fast mode) exactly as a capture walks them; no switch of
 * their own.  One ray = 6 doubles: origin xyz, direction xyz (Ray3::new, ray.rs:28-33; the direction is used as given, not normalised).
 * No counterpart among the reference's public items: its Accel and Primitive::intersect are pub (lib.rs:34,42), its Ray and RayIntersection
 * are not. */
typedef struct lg_hit {
    double t;           /* closest hit's parameter, o + t*d; +INFINITY = no hit (then p / ng / ns are 0, kind 0, prim and instance
                           0xFFFFFFFF, material -1) */
    double p[3];        /* o + d*t in world space: the shading frame's point before the 2^-36 offset shading adds */
    double ng[3];       /* unit geometric normal faced toward -d */
    double ns[3];       /* unit shading normal (mesh smoothing, the cuboid's face normal, the sphere's) */
    uint32_t kind;      /* 0 none, 1 sphere, 2 box / cube, 3 mesh triangle */
    uint32_t prim;      /* sphere / box: its ordinal among the scene's spheres / boxes in scene-graph order (depth first, insertion
                           order); triangle: its face number in its OBJ (triangle.rs:425-427) */
    uint32_t instance;  /* the (nested) accel the primitive sits in: 0 = root, groups and mesh instances in scene-graph order */
    int32_t material;   /* the material shading uses (integrate.rs:29-30, bvh.rs:513-515): an index for lg_accel_material */
} lg_hit;               /* 96 bytes, no padding */

/* Closest hit of every ray: hit i is what root.intersect(&Ray3::new(o, d), &mut isect) returns (bvh.rs:461-522), resolved to world space
 * as shading sees it; t and the winning primitive are the reference's bit for bit, exact ties included (its visit order decides them).
 * Any f64 input is accepted as it is (zero, infinite and NaN components included). */
int lg_intersect(const lg_accel *, const double *rays, size_t n, lg_hit *hits);                  /* host arrays; synchronous */
/* occluded[i] = 1 iff ray i's closest hit has t < 1.0 -- the segment o -> o + d is blocked: the shadow test of point.rs:49, run through
 * the any-hit walk of the render's shadow passes. */
int lg_occluded(const lg_accel *, const double *rays, size_t n, uint8_t *occluded);              /* host arrays; synchronous */
/* Device forms: they only enqueue on hip_stream (NULL = HIP's default stream; one stream at a time per accel, as lg_capture_subset_device).
 * dev_rays must be 8-byte aligned, dev_hits 16-byte aligned, and both device memory of the accel's device (hipPointerGetAttributes):
 * anything else is an error before any launch.  n == 0 is a successful no-op. */
int lg_intersect_device(const lg_accel *, const double *dev_rays, size_t n, lg_hit *dev_hits, void *hip_stream);
int lg_occluded_device(const lg_accel *, const double *dev_rays, size_t n, uint8_t *dev_occluded, void *hip_stream);
/* Visibility matrices: occlusion between two point sets, bit-packed -- "which of these n_from points see which of those n_to points"
 * (surface samples against lights or sky samples for a bake, patch against patch for form factors, sensors against targets) without
 * the caller writing n_from * n_to rays of 48 bytes: the segments are made in the kernel, as the render makes its shadow rays.
 * from is n_from x 3 doubles, to is n_to x 3 doubles; any f64 is accepted as it is, NaN and infinities included.
 * Segment (i, j) is the ray with origin from[i] and direction to[j] - from[i] -- three separate f64 subtractions, no contraction -- and it
 * is occluded iff lg_occluded answers 1 for that ray: the shadow test of point.rs:49 (t < 1) run through the any-hit walk.  Traversal is
 * the accel's mode exactly as for the other queries (reference, pruned, LDS-resident scene, fast mode); no switch of its own.
 * lg_accel_set_query_order plays no part: there is no ray array to sort.  A wave walks an 8 x 8 block of the matrix -- 8 consecutive from
 * points against 8 consecutive to points --, so callers who want coherence order their points so that neighbours in the array are
 * neighbours in space.
 * bits: n_from rows of row_bytes bytes, row_bytes >= ceil(n_to / 8).  Bit j of row i is (bits[i*row_bytes + (j >> 3)] >> (j & 7)) & 1,
 * 1 iff segment (i, j) is occluded: least significant bit first, numpy's packbits(..., bitorder="little") per row.  The padding bits of
 * a row's last used byte are written as 0; bytes of a row beyond ceil(n_to / 8) are never touched.
 * blocked (may be NULL): blocked[i] = the number of set bits of row i.  It is WRITTEN, NOT ACCUMULATED: whatever the buffer held before is
 * gone.  bits may be NULL when blocked is given; both NULL is an error.
 * n_from == 0 or n_to == 0 is a successful no-op that writes nothing.  ceil(n_from / 8) * ceil(n_to / 8) > 2^32 - 1 is an error before
 * any launch (8 x 8 blocks are counted in 32 bits, as the other queries' tiles are).
 * Errors (non-zero, lg_last_error, nothing launched, no output touched): a NULL accel, a NULL point set with a non-zero count, both
 * outputs NULL, row_bytes too small; in the device form also a pointer that is not device memory of the accel's device or is misaligned
 * (dev_from and dev_to 8-byte aligned, dev_blocked 4, dev_bits 1), or a buffer that ends beyond its allocation.
 * Device form: it only enqueues on hip_stream (the zeroing of dev_blocked that precedes the kernel included); one stream at a time per
 * accel.  Host form (synchronous): the points go up, the rows come back compact and are placed into the caller's stride, so the bytes of a
 * row behind its used part stay untouched; blocked comes back.  No counterpart in the reference. */
int lg_visibility(const lg_accel *, const double *from, size_t n_from, const double *to, size_t n_to, uint8_t *bits, size_t row_bytes,
                  uint32_t *blocked);                                                             /* host arrays; synchronous */
int lg_visibility_device(const lg_accel *, const double *dev_from, size_t n_from, const double *dev_to, size_t n_to, uint8_t *dev_bits,
                         size_t row_bytes, uint32_t *dev_blocked, void *hip_stream);
/* Direction sets: which of n_dirs shared directions are open above each of n_points points -- ambient occlusion, sky visibility and
 * sky-light bakes, sun hours (the directions are the sun's positions over a year), hemispherical form factors, antenna line of sight --
 * without the caller writing n_points * n_dirs rays of 48 bytes: n_points + n_dirs vectors describe all of them.  An EXTRA; no
 * counterpart in the reference.
 * points is n_points x 3 doubles; normals is n_points x 3 doubles and MAY BE NULL; dirs is n_dirs x 3 doubles.  Any f64 is accepted as it
 * is, NaN and infinities included.
 * Pair (i, k) is the ray with origin points[i] and direction dirs[k], both bit for bit as given: no arithmetic makes the ray.  The
 * direction's length is the reach: as for lg_occluded the segment p -> p + d is what is tested (t < 1), so the caller scales the directions
 * by the AO radius, or by more than the scene's diameter for "sky".  The library does not offset the origin: a caller starting from
 * surface hits offsets them as shading does, p + ng * 2^-36.
 * above(i, k): true for every pair when normals is NULL; otherwise s = (n.x*d.x + n.y*d.y) + n.z*d.z in f64, in this order, with no
 * contraction, and above = s > 0.0 -- a NaN s, a zero direction and a perpendicular direction are therefore not above.
 * open(i, k) = above(i, k) and lg_occluded answers 0 for the pair's ray, in the accel's traversal mode exactly as for the other queries
 * (reference, pruned, LDS-resident scene, fast mode); no switch of its own.  lg_accel_set_query_order plays no part: there is no ray
 * array to sort.  A pair that is not above is NOT WALKED.  A wave walks 64 consecutive points against 8 consecutive directions, one
 * direction at a time -- 64 parallel rays --, so callers who want coherence order their points so that neighbours in the array are
 * neighbours in space (with similar normals).
 * Outputs; each may be NULL, all three NULL is an error:
 * bits: n_points rows of row_bytes bytes, row_bytes >= ceil(n_dirs / 8).  Bit k of row i is (bits[i*row_bytes + (k >> 3)] >> (k & 7)) & 1,
 * 1 iff open(i, k): least significant bit first, numpy's packbits(..., bitorder="little") per row.  The padding bits of a row's last used
 * byte are written as 0; bytes of a row beyond ceil(n_dirs / 8) are never touched.
 * open: open[i] = the number of open directions at point i.  above: above[i] = the number of directions above, n_dirs when normals is
 * NULL.  Both counts are WRITTEN, NOT ACCUMULATED: whatever the buffers held before is gone.  open[i] / above[i] is the ambient-occlusion
 * value for a uniform direction set, the cosine-weighted one for cosine-distributed directions.
 * n_points == 0 or n_dirs == 0 is a successful no-op that writes nothing.
 * Errors (non-zero, lg_last_error, nothing launched, no output touched): a NULL accel; NULL points or dirs with non-zero counts; all
 * outputs NULL; row_bytes too small; n_dirs > 2^32 - 1; ceil(n_points / 64) * ceil(n_dirs / 8) > 2^32 - 1 (tiles of 64 points x 8
 * directions are counted in 32 bits, as the other queries' tiles are); bits rows that do not fit the address space -- all checked before
 * any HIP call --; in the device form also a pointer that is not device memory of the accel's device or is misaligned (dev_points,
 * dev_normals and dev_dirs 8-byte aligned, dev_open and dev_above 4, dev_bits 1), or a buffer that ends beyond its allocation.
 * Device form: it only enqueues on hip_stream (the zeroing of dev_open and dev_above that precedes the kernel included); one stream at a
 * time per accel.  Host form (synchronous): the tables go up, the rows come back compact and are placed into the caller's stride, so the
 * bytes of a row behind its used part stay untouched; rows and counts are staged, so an error on the way leaves the caller's arrays as
 * they were. */
int lg_open_directions(const lg_accel *, const double *points, const double *normals, size_t n_points, const double *dirs, size_t n_dirs,
                       uint8_t *bits, size_t row_bytes, uint32_t *open, uint32_t *above);       /* host arrays; synchronous */
int lg_open_directions_device(const lg_accel *, const double *dev_points, const double *dev_normals, size_t n_points,
                              const double *dev_dirs, size_t n_dirs, uint8_t *dev_bits, size_t row_bytes, uint32_t *dev_open,
                              uint32_t *dev_above, void *hip_stream);
/* Range scans: the first hits along n_beams shared beams from each of n_poses sensor poses -- a simulated lidar or depth sensor, a probe
 * grid that samples clearance for a distance-field bake, a cube-map depth pass, a height field -- without the caller writing
 * n_poses * n_beams rays of 48 bytes and reading back lg_hit records of 96: n_poses + n_beams vectors describe all the rays, and only the
 * planes asked for come back.  An EXTRA; no counterpart in the reference.
 * Inputs: origins is n_poses x 3 doubles; frames is n_poses x 9 doubles, a row-major 3 x 3 matrix M per pose whose columns are the
 * sensor's axes in world space, and MAY BE NULL; beams is n_beams x 3 doubles, shared by all poses.  Any f64 is accepted as it is, NaN and
 * infinities included.
 * Ray (i, k): the origin is origins[i] bit for bit.  With frames == NULL the direction is beams[k] bit for bit: no arithmetic makes the
 * ray.  Otherwise, with M = frames + 9*i and b = beams[k], d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z for c = 0, 1, 2, in f64, in
 * this order, with no contraction.  An identity frame is therefore NOT the same as NULL for -0.0, infinite and NaN beam components:
 * -0.0 comes out as +0.0 unless both other products are -0.0 too, an infinite component makes the other two components of d NaN (0 * inf), and a
 * NaN component all three.
 * The direction is not normalised: range is the hit's parameter t, which is the distance when the beams are unit vectors and the frames
 * rotations.
 * Hit: what lg_intersect returns for that ray, bit for bit, in the accel's traversal mode exactly as for the other queries (reference,
 * pruned, LDS-resident scene, fast mode); no switch of its own.  lg_accel_set_query_order plays no part: there is no ray array to sort.
 * Planes (lg_scan_out): element (i, k) is at i*n_beams + k.  range = (float)t, +INF on a miss.  point[c] = (float)p[c].  normal[c] =
 * (float)ng[c]: the geometric normal faced toward the sensor, the one an incidence angle wants -- not ns.  id is as in lg_features: kind,
 * prim, instance, material in one 16-byte store, 0, ~0, ~0, -1 on a miss.  point and normal are zeros on a miss, as lg_hit has them.
 * (float) rounds to nearest even.
 * Per-pose reductions, both WRITTEN, NOT ACCUMULATED: whatever the buffers held before is gone.  hits[i] = the number of beams with
 * kind != 0.  nearest[i] = the f32 range of pose i whose bit pattern, read as uint32, is smallest among the pose's hits; +INF where no
 * hit's pattern is below +INF's.  In words: the smallest non-negative finite range -- a hit whose range is NaN, negative or has overflowed
 * to +INF never wins.  It is an integer atomicMin on the bit pattern into a buffer pre-filled with 0x7F800000 (hits: an integer add into
 * zeros), both pre-fills on the same stream ahead of the kernel; integer minima and sums do not depend on the order tiles finish in.
 * lanes: the work item.  1: beam lanes -- a tile is one pose x 64 consecutive beams, a beam per lane; the rays share an origin, like a
 * camera's; the form for few poses and many beams.  2: pose lanes -- a tile is 64 consecutive poses x 8 consecutive beams, a pose per
 * lane and the beams in a loop, the direction sets' work item; with NULL frames the 64 rays are parallel.  0: auto -- pose lanes iff
 * n_poses >= n_beams, else beam lanes; a stated default, not a measured optimum.  Any other value is an error.  Every output is the same
 * bytes in either form.  Callers who want coherence order poses (pose lanes) or beams (beam lanes) so that neighbours in the array are
 * neighbours in space.
 * Limits, all checked before any HIP call: n_beams > 2^32 - 1 is an error; more tiles than 2^32 - 1 in the form chosen is an error:
 * n_poses * ceil(n_beams / 64) > 2^32 - 1 for beam lanes, ceil(n_poses / 64) * ceil(n_beams / 8) > 2^32 - 1 for pose lanes (tiles are
 * counted in 32 bits, as the other queries' are); planes that do not fit the address space are an error.  n_poses == 0 or n_beams == 0 is
 * a successful no-op that writes nothing, and it is answered BEFORE every other check: with an empty set a NULL accel or out, NULL
 * tables and a bad lanes are not looked at (as for the other structured queries).
 * Errors (non-zero, lg_last_error, nothing launched, no output touched), for non-zero counts: a NULL accel or out; NULL origins or beams
 * with non-zero counts; all six outputs NULL; a bad lanes; the limits above; in the device form also a pointer that is not device memory
 * of the accel's device or is misaligned (dev_origins, dev_frames and dev_beams 8-byte aligned, id 16, the float planes, hits and nearest
 * 4), or a buffer that ends beyond its allocation.
 * Device form: dev_out is a HOST struct of device pointers; it only enqueues on hip_stream (the two pre-fills that precede the kernel
 * included); one stream at a time per accel.  Host form (synchronous): the tables go up, the planes come back into staging and are
 * copied out at the end, so an error on the way leaves the caller's arrays as they were.
 * Out of scope: there is no maximum range inside the walk -- the caller thresholds range; no noise or intensity model; no multi-device
 * split.
 * lg_range_scan_lanes: the work item a call with these counts and this `lanes` would use -- 1 or 2; -1 for a bad `lanes`; no device is
 * touched. */
typedef struct lg_scan_out {
    float    *range;    /* [n_poses*n_beams]     */
    float    *point;    /* [n_poses*n_beams][3]  */
    float    *normal;   /* [n_poses*n_beams][3]  */
    uint32_t *id;       /* [n_poses*n_beams][4]: kind, prim, instance, material -- the last 16 bytes of an lg_hit */
    uint32_t *hits;     /* [n_poses]             */
    float    *nearest;  /* [n_poses]             */
} lg_scan_out;          /* 48 bytes; each pointer may be NULL, all NULL is an error */
int lg_range_scan(const lg_accel *, const double *origins, const double *frames, size_t n_poses, const double *beams, size_t n_beams,
                  int lanes, const lg_scan_out *out);                      /* host arrays; synchronous */
int lg_range_scan_device(const lg_accel *, const double *dev_origins, const double *dev_frames, size_t n_poses, const double *dev_beams,
                         size_t n_beams, int lanes, const lg_scan_out *dev_out, void *hip_stream);
int lg_range_scan_lanes(size_t n_poses, size_t n_beams, int lanes);        /* the work item a call would use: 1 or 2; -1 for a bad `lanes`; no device */
/* Radiance along every ray: the third query, for rays no camera of the scene generates (a fisheye or panorama, a light probe or cube
 * map, a lightmap bake from surface points, a caller's own path continuation, a second view of an accel without rebuilding it).
 * radiance[3*i ..] = what integrate() leaves for a pixel whose one sample is ray i: (Color::zero() + li(root, ray_i, depth 0)) * 1.0
 * (integrate.rs:16-20, 23-132) -- lights, shadow rays, ambient, specular reflection / transmission down to the scene's max recursion
 * depth, background on a miss -- before quantisation.  One ray = 6 doubles as for lg_intersect; direction used as given.
 * f64 RGB, n x 3, in the caller's order; the zero-plus-li and the times-one are kept so that the bytes are lg_capture_radiance's for the
 * render's own rays (lg_camera_rays).  The scene's camera and its supersampling play no part: a caller who wants a supersampled pixel
 * sums its samples' results in camera order and multiplies by 1.0 / S, which is the render's own arithmetic.
 * Traversal is the accel's mode, as for the other queries; lg_accel_set_query_order(1) is honoured (a query of 64 rays or fewer is
 * walked as given).  The organisation is always the level-by-level pipeline -- the caller's rays are its level 0 --, whatever
 * lg_accel_set_streaming says, cut into chunks by that pipeline's memory budget (LASGUN_WF_BUDGET_MB); nothing is measured or
 * remembered for it, and lg_profile_* credit its kernels as a render's.  That pipeline keeps a hit's light visibility in a 32-bit word:
 * a scene with MORE THAN 32 LIGHTS is an error before any launch (lg_last_error), as is a recursion depth of 20 or more.
 * n == 0 is a successful no-op; NULL arguments and n > 2^32 - 1 tiles of 64 rays are errors.
 * Device form: dev_rays and dev_radiance must be 8-byte aligned device memory of the accel's device, checked before anything is enqueued.
 * It only enqueues on hip_stream, with the exceptions the render and the sorted order have: the first query of a stream, and the first of
 * more rays than any launch before it, grows the launch context's level arrays (and, in mode 1, the sort's scratch) after a device-wide
 * synchronise.  One stream at a time per accel. */
int lg_radiance(const lg_accel *, const double *rays, size_t n, double *radiance);                         /* host arrays; synchronous */
int lg_radiance_device(const lg_accel *, const double *dev_rays, size_t n, double *dev_radiance, void *hip_stream);
/* Radiance gathers: li() along n_dirs shared directions from each of n_poses poses, reduced per pose by the caller's weights -- an
 * irradiance volume of SH probes, a cube map per probe, a lightmap final gather from surface points -- without the caller writing
 * n_poses * n_dirs rays of 48 bytes and reading back 24 bytes of radiance for each: n_poses + n_dirs vectors describe all the rays, and
 * n_weights RGB sums a pose come back.  The radiance half of what lg_open_directions is for occlusion.  An EXTRA; no counterpart in the
 * reference.
 * Inputs: origins is n_poses x 3 doubles; frames is n_poses x 9 doubles, a row-major 3 x 3 matrix M per pose, and MAY BE NULL; dirs is
 * n_dirs x 3 doubles, shared by all poses; weights is n_dirs x n_weights doubles, k-major: W[k*n_weights + c].  Any f64 is accepted as it
 * is, NaN and infinities included.
 * Ray (i, k): exactly the range scans' rule.  The origin is origins[i] bit for bit.  With frames == NULL the direction is dirs[k] bit for
 * bit.  Otherwise, with M = frames + 9*i and b = dirs[k], d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z for c = 0, 1, 2, in f64, in this
 * order, with no contraction (so an identity frame is NOT the same as NULL for -0.0, infinite and NaN components, as for lg_range_scan).
 * The direction is not normalised.
 * Radiance: L(i,k) is what lg_radiance returns for that ray, bit for bit: (0 + li) * 1.0, in the accel's traversal mode exactly as for
 * the other queries; no switch of its own.  lg_accel_set_query_order plays no part: there is no ray array to sort.  lg_radiance's
 * refusals hold: a scene with more than 32 lights, or a recursion depth of 20 or more, is an error before any launch.
 * Outputs (lg_gather_out), both WRITTEN, NOT ACCUMULATED: radiance[i*n_dirs + k] = L(i,k), three doubles.
 * sums[(i*n_weights + c)*3 + ch]: acc = +0.0; for k = 0 .. n_dirs-1 in that order acc = acc + L(i,k)[ch] * W[k*n_weights + c]; each step
 * is one f64 product then one f64 sum, nothing fused.  NaN and infinite weights and radiances follow IEEE (0 * inf is NaN); a zero weight
 * is not skipped.  Every element is written by exactly one lane; there are no atomics, so nothing depends on the order tiles finish in.
 * weights and n_weights are looked at only where sums is asked for.
 * lanes: the work item.  1: direction lanes -- a tile is one pose x 64 consecutive directions, tile = pose * ceil(n_dirs/64) + block; the
 * rays share an origin, like a camera's.  2: pose lanes -- a tile is 64 consecutive poses x one direction, tile = pose_block * n_dirs + k;
 * with NULL frames the 64 rays are parallel.  0: auto -- pose lanes iff n_poses >= n_dirs, else direction lanes; a stated default, not a
 * measured optimum.  Any other value is an error.  Every output is the same bytes in either form.
 * Limits, all checked before any HIP call: n_dirs > 2^32 - 1 is an error; more tiles than 2^32 - 1 in the form chosen is an error
 * (n_poses * ceil(n_dirs/64) for direction lanes, ceil(n_poses/64) * n_dirs for pose lanes); each of n_poses*n_dirs*24, n_poses*72 and,
 * with sums, n_dirs*n_weights*8 and n_poses*n_weights*24 bytes must fit size_t.  n_poses == 0 or n_dirs == 0 is a successful no-op that
 * writes nothing, and it is answered BEFORE every other check, as for the scans.
 * Errors (non-zero, lg_last_error, nothing launched, no output touched), for non-zero counts: a NULL accel, out, origins or dirs; both
 * outputs NULL; sums given with weights == NULL or n_weights == 0; a bad lanes; the limits above; lg_radiance's two refusals; in the
 * device form also any pointer that is not 8-byte aligned device memory of the accel's device, or that ends beyond its allocation.
 * Where li lives: with radiance given, li IS the caller's plane and the whole call is one level-0 query of the level-by-level pipeline
 * (cut into chunks by LASGUN_WF_BUDGET_MB, as lg_radiance is), then one reduction.  With sums alone, li is parked in a buffer of the
 * launch context: the call is cut into batches of whole consecutive poses that park at most LASGUN_GATHER_PARK_MB MiB each (read once;
 * default 1024, a stated default; never fewer than one pose a batch), and each batch is reduced before the next.  Batching cannot change
 * a bit: a sum never crosses a pose.  lg_profile_read_kinds credits the reduction as a combine pass, kind 1.
 * Device form: dev_out is a HOST struct of device pointers.  It only enqueues on hip_stream, with lg_radiance_device's exception: growing
 * the launch context's level arrays or the parked buffer synchronises the device first.  One stream at a time per accel.  Host form
 * (synchronous): the tables go up, the outputs come back into staging and are copied out at the end, so an error on the way leaves the
 * caller's arrays as they were.
 * Out of scope: a multi-device split, a sorted order, per-pose direction sets or weights, any other summation order, normal-dependent
 * culling of directions (callers use lg_open_directions' `above` rule, or zero weights).
 * lg_radiance_gather_lanes: the work item a call with these counts and this `lanes` would use -- 1 or 2; -1 for a bad `lanes`; no device
 * is touched. */
typedef struct lg_gather_out {
    double *radiance;  /* [n_poses*n_dirs][3], element (i,k) at i*n_dirs + k; may be NULL */
    double *sums;      /* [n_poses][n_weights][3]; may be NULL */
} lg_gather_out;       /* 16 bytes; both NULL is an error */
int lg_radiance_gather(const lg_accel *, const double *origins, const double *frames, size_t n_poses, const double *dirs, size_t n_dirs,
                       const double *weights, size_t n_weights, int lanes, const lg_gather_out *out);      /* host arrays; synchronous */
int lg_radiance_gather_device(const lg_accel *, const double *dev_origins, const double *dev_frames, size_t n_poses, const double *dev_dirs,
                              size_t n_dirs, const double *dev_weights, size_t n_weights, int lanes, const lg_gather_out *dev_out,
                              void *hip_stream);
int lg_radiance_gather_lanes(size_t n_poses, size_t n_dirs, int lanes);   /* the work item a call would use: 1 or 2; -1 for a bad `lanes`; no device */
/* The rays the render traces for the pixels [x0,x1) x [y0,y1) of a width x height film: row-major pixels and, per pixel, the camera's
 * samples in camera.rs order (idx = i*dim + j, camera.rs:137-146), 6 doubles each: (x1-x0) * (y1-y0) * supersamples rays. */
int lg_camera_rays(const lg_accel *, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *rays);
int lg_camera_rays_device(const lg_accel *, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                          double *dev_rays, void *hip_stream);
uint32_t lg_camera_samples(const lg_accel *); /* rays per pixel of lg_camera_rays: the camera's supersamples */
/* Ray films: the caller's rays rendered into a film -- what a custom camera (a fisheye or panorama, a cube-map face, a second view of an
 * accel) needs after lg_radiance: the reference's sample sum, its quantisation, and the bytes placed in a film, all on the device.
 * rays: pixels * samples rays of 6 doubles as for lg_intersect, PIXEL-MAJOR: the rays of pixel slot g are [g*samples, (g+1)*samples), in
 * the order they are summed.  Slot g is the film pixel at offset pixel_offsets[g] (offset = y*width + x), or g when pixel_offsets is NULL.
 * A slot whose offset is >= width*height writes nothing (as a k behind the film is an empty subset for lg_capture_subsets); a pixel no
 * slot names stays untouched, byte for byte; offsets are expected to be distinct -- with duplicates, which slot's value remains is
 * unspecified.  (The indirection is what lets rays arrive in 8 x 8-tile order -- row-major shadow rays cost 1.28 x the tile order's,
 * DESIGN.md section 3.7 --, a view be rendered a subset per call, and a crop be rendered at all.)
 * The pixel's value is integrate()'s (integrate.rs:16-20): color = Color::zero(); color = color + li(ray_s) for s = 0 .. samples-1 in that
 * order; color * (1.0 / (double)samples); then per channel to_byte (img.rs:65-67) with A = 255 into the RGBA8 film, and / or the three
 * doubles before quantisation into rgb (width*height*3 doubles, addressed like the film).  At least one output is required.  For the
 * scene's own camera -- lg_camera_rays, samples = lg_camera_samples -- that is lg_capture's film and lg_capture_radiance's doubles, bit
 * for bit.
 * Everything else is lg_radiance's contract: the accel's traversal mode, always the level-by-level pipeline whatever lg_accel_set_streaming
 * says, LASGUN_WF_BUDGET_MB chunks, lg_accel_set_query_order(1) honoured (it sorts rays, not pixels: a pixel's samples may be walked in
 * different chunks), MORE THAN 32 LIGHTS or a recursion depth of 20 or more an error before any launch.  samples == 1: a ray is finished
 * where lg_radiance finishes it, as one 4-byte store and / or three doubles at its pixel -- no parked radiance, no second pass.
 * samples > 1: every ray's li is parked in library scratch (24 bytes a ray, indexed by the ray, so neither chunk boundaries nor the
 * sorted order matter), then one resolve pass, a lane per slot, sums, scales, quantises and writes.
 * pixels == 0 is a successful no-op.  Errors (non-zero, lg_last_error, nothing launched, no output touched): a NULL accel or rays,
 * samples == 0, both outputs NULL, pixels * samples beyond what lg_radiance accepts, a film that is not width x height (host form).
 * Host form (synchronous): copies the rays to the device and copies back ONLY the named slots' pixels -- pixels * 4 and / or pixels * 24
 * bytes, compact -- which the host then places at their offsets; the film is never uploaded and never downloaded whole.
 * Device form: only enqueues on hip_stream.  dev_rays (pixels*samples*6 doubles), dev_pixel_offsets (pixels uint64, may be NULL), dev_rgba
 * (width*height*4 bytes, may be NULL) and dev_rgb (width*height*3 doubles, may be NULL) must be device memory of the accel's device,
 * dev_rays / dev_pixel_offsets / dev_rgb 8-byte aligned and dev_rgba 4-byte aligned: checked before anything is enqueued.  The one
 * exception is the other queries': the first call of a stream, or of a larger size, may grow scratch after a device-wide synchronise.
 * One stream at a time per accel.  No counterpart in the reference. */
int lg_capture_rays(const lg_accel *, const double *rays, size_t pixels, uint32_t samples, const uint64_t *pixel_offsets, lg_film *film,
                    double *rgb, uint32_t width, uint32_t height);
int lg_capture_rays_device(const lg_accel *, const double *dev_rays, size_t pixels, uint32_t samples, const uint64_t *dev_pixel_offsets,
                           uint32_t width, uint32_t height, void *dev_rgba, double *dev_rgb, void *hip_stream);
/* Feature buffers: the auxiliary images of the scene's own camera view -- first-hit depth, shading normal, albedo, coverage and object
 * ids, what a denoiser, a compositor, an edge-aware upsampler or a picking UI asks a renderer for -- without the caller writing
 * lg_camera_rays' rays (48 bytes each) and lg_intersect's hits (96 bytes each) and reducing the samples itself: the rays are made in the
 * kernel, in the render's 8 x 8-pixel tiles, and at most 48 bytes a pixel are written.  An EXTRA: the contract below is this library's own,
 * nothing of the reference is mirrored. */
typedef struct lg_features {
    float    *depth;     /* [width*height]     */
    float    *normal;    /* [width*height][3]  */
    float    *albedo;    /* [width*height][3]  */
    float    *coverage;  /* [width*height]     */
    uint32_t *id;        /* [width*height][4]: kind, prim, instance, material -- the last 16 bytes of an lg_hit */
} lg_features;           /* 40 bytes; each pointer may be NULL, all NULL is an error */
/* lg_features itself is always a host struct; in the device form its members are device pointers.
 * Pixels: [x0,x1) x [y0,y1) of a width x height film.  Every plane is addressed like the film: pixel y*width + x.  A pixel outside the
 * rectangle is never touched.
 * Rays: the rays of a pixel are the S = lg_camera_samples rays of lg_camera_rays for it, s = 0 .. S-1 in camera order.  Sample s's hit is
 * what lg_intersect returns for that ray, bit for bit, in the accel's traversal mode (reference, pruned, LDS-resident scene, fast mode);
 * no switch of its own.  lg_accel_set_query_order plays no part (there is no ray array to sort), and neither do the interleave, subset
 * and organisation settings of the captures.
 * Hit: sample s is a hit iff lg_intersect reports kind != 0 for it.
 * Accumulators: all f64, no contraction.  nhit counts the hits; tsum, nsum[3] and asum[3] start at +0.0.  For s ascending, a hit adds t to
 * tsum, ns (lg_hit::ns, per component) to nsum, and material_rgb[3*material + c] to asum[c].  A miss adds nothing.
 * material_rgb: lg_accel_material_count x 3 doubles, the caller's colour per material; required iff albedo is requested and ignored
 * otherwise.  A hit whose material is outside 0 .. count-1 adds nothing to asum -- which this library's tables cannot produce: every hit's
 * material is an index lg_accel_material accepts (the one shading itself reads); the rule is kept for a negative or stale index all the same.
 * Outputs: with inv = 1.0 / (double)S,
 *   normal[c] = (float)(nsum[c] * inv);  albedo[c] = (float)(asum[c] * inv);  coverage = (float)((double)nhit * inv);
 *   depth = nhit ? (float)(tsum * (1.0 / (double)nhit)) : +INFINITY;
 * (float) rounds to nearest even, as numpy's astype(float32).  Normal and albedo are therefore premultiplied by coverage; depth is the
 * mean over the samples that hit.
 * id: sample 0's kind, prim, instance, material exactly as lg_hit has them (0, ~0, ~0, -1 on a miss), written as one 16-byte store.
 * Errors (non-zero, lg_last_error, nothing launched, no output touched): a NULL accel or out; all five planes NULL; albedo without
 * material_rgb; a bad rectangle, with lg_capture_rect's rule; more 8 x 8 tiles than 2^32 - 1 (or x1 / y1 above 2^32 - 8: a tile's pixel coordinates are 32-bit); in the device form a plane or table that is
 * not device memory of the accel's device, is misaligned (id 16-byte aligned, material_rgb 8, the float planes 4) or ends beyond its
 * allocation.  An empty rectangle is a successful no-op.
 * Host form (synchronous): the table goes up and the rectangle's pixels come back compact; the host places them at their film offsets, so
 * nothing outside the rectangle is read or written.  Device form: it only enqueues on hip_stream; one stream at a time per accel. */
int lg_capture_features(const lg_accel *, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                        const lg_features *out, const double *material_rgb);                       /* host arrays; synchronous */
int lg_capture_features_device(const lg_accel *, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1,
                               const lg_features *dev_out, const double *dev_material_rgb, void *hip_stream);
size_t lg_accel_material_count(const lg_accel *);   /* indices 0 .. count-1 are valid for lg_accel_material */
/* Lens rays: the rays of two cameras the reference does not have, generated on the device in the layout lg_capture_rays takes.  An EXTRA:
 * every expression below is this library's own, nothing of the reference is mirrored. */
typedef struct lg_lens {
    int32_t kind;        /* 0 equirectangular panorama, 1 equidistant fisheye */
    int32_t reserved;    /* 0 */
    double origin[3], right[3], up[3], forward[3]; /* used as given: not normalised, not orthogonalised */
    double fov_deg;      /* kind 1: the full angle across the film's shorter side; kind 0: ignored */
} lg_lens;               /* 112 bytes, no padding */
/* Pixel slot g is the film pixel at offset pixel_offsets[g] (y*width + x), or g when pixel_offsets is NULL -- then pixels must be
 * width*height.  Per slot S = samples_root^2 rays, sample idx = i*samples_root + j at
 *   u = ((double)x + ((double)j + 0.5) / (double)samples_root) / (double)width,
 *   v = ((double)y + ((double)i + 0.5) / (double)samples_root) / (double)height;
 * rays is pixels * S * 6 doubles, slot-major, a slot's samples in idx order.  The origin is lens.origin, exactly.  A slot whose offset
 * is >= width*height gets origin and direction all zero (lg_capture_rays writes nothing for such a slot: offsets and rays line up).
 * The direction, in f64 with no contraction, sin / cos / atan2 the device's correctly rounded ones (the render's own, trig.h), evaluated
 * in exactly this order, per component c of the basis vectors:
 *   kind 0:  phi = (u - 0.5) * 6.283185307179586;  theta = (0.5 - v) * 3.141592653589793;
 *            d_c = (((cos theta * sin phi) * right_c) + (sin theta * up_c)) + ((cos theta * cos phi) * forward_c)
 *   kind 1:  m = min(width, height);  a = (2.0 * u - 1.0) * ((double)width / (double)m);  b = (1.0 - 2.0 * v) * ((double)height / (double)m);
 *            r = sqrt(a * a + b * b);  psi = atan2(b, a);  theta = r * ((fov_deg * 0.5) * 0.017453292519943295);
 *            d_c = (sin theta * ((cos psi * right_c) + (sin psi * up_c))) + (cos theta * forward_c)
 *            -- the formula continues outside the image circle; there are no special cases.
 * Errors: a NULL lens or rays, a kind other than 0 / 1, reserved != 0, an empty film, samples_root == 0, pixels != width*height without
 * offsets.  pixels == 0 is a successful no-op.  Host form: runs the same kernel on the current device (lg_set_device) and copies the rays
 * back; synchronous.  Device form: only enqueues on hip_stream of `device`; dev_rays and dev_pixel_offsets must be 8-byte aligned device
 * memory of that device, checked before the launch. */
int lg_lens_rays(const lg_lens *, uint32_t width, uint32_t height, uint32_t samples_root, const uint64_t *pixel_offsets, size_t pixels,
                 double *rays);
int lg_lens_rays_device(int device, const lg_lens *, uint32_t width, uint32_t height, uint32_t samples_root,
                        const uint64_t *dev_pixel_offsets, size_t pixels, double *dev_rays, void *hip_stream);
/* Views: one accel seen from other cameras than its scene's, K of them into K films in one call -- an orbit, a stereo pair, the six faces
 * of a cube map, a light field, thumbnails -- without rebuilding the scene and the accel per camera and without writing 48 bytes a ray
 * that a kernel makes from 15 doubles a view.  An EXTRA: no counterpart in the reference. */
typedef struct lg_view {            /* a camera as the kernels read it: Camera's derived fields (camera.rs:6-37), used AS GIVEN */
    double origin[3], view[3], up[3], aux[3];
    double image_plane_height, pixel_separation;
    uint32_t samples_root;          /* supersampling base + 1: samples per pixel = samples_root^2; 1 .. 256 */
    uint32_t reserved;              /* must be 0 */
} lg_view;                          /* 120 bytes, no padding */
/* lg_view_look_at: the scene camera's own host code -- Camera::init(perspective, param), Camera::look_at(origin, look, up),
 * Camera::set_supersampling(supersampling) -- run on a camera of its own; param is the fov in degrees for a perspective view and the
 * scale for an orthographic one.  The result is, byte for byte, what lg_scene_view reports for a scene that received
 * lg_scene_set_perspective_camera / lg_scene_set_orthographic_camera, lg_camera_look_at and lg_camera_set_supersampling, in this order,
 * with the same arguments.  (The aperture radius is stored by the scene and used by nothing: a view has none.)  Device-free; an error
 * (non-zero, lg_last_error) only for a NULL pointer.
 * lg_scene_view / lg_accel_view: the scene's own camera as a view (of the scene the accel was built from); device-free.
 * lg_view_rays*: lg_camera_rays* with the view in the camera's place -- the same pixel and sample order, the same 6 doubles, the same
 * errors, and a samples_root of 0 or above 256 or reserved != 0; (x1-x0) * (y1-y0) * samples_root^2 rays.
 * lg_capture_views*: film v starts at rgba + v*width*height*4 and its doubles at rgb + v*width*height*3; either output may be NULL, both
 * NULL is an error.  The ray of (v, x, y, s) is Camera::sample's expression (camera.rs:113-146) over view v's fields, all f64, nothing
 * contracted, in this order -- with winv = 1.0 / (double)width, hinv = 1.0 / (double)height, aspect = (double)width / (double)height
 * (film.rs:40-42) and ss_distance = 1.0 / (double)samples_root:
 *   plane_w = image_plane_height * aspect;  pixel = image_plane_height * hinv;  sep = ss_distance * pixel;
 *   sox = ((double)x * winv - 0.5) * plane_w;  soy = (0.5 - (double)(y + 1) * hinv) * image_plane_height;
 *   o = (origin + ((soy * pixel_separation) * up)) + ((sox * pixel_separation) * aux);
 *   d = (view + (soy * up)) + (sox * aux);  updiff = up * sep;  auxdiff = aux * sep;  half = updiff * 0.5 + auxdiff * 0.5;
 *   i = s / samples_root;  j = s % samples_root;  direction = ((d + ((double)j * updiff)) + ((double)i * auxdiff)) + half;  origin = o.
 * A pixel's value is integrate()'s (integrate.rs:16-20): the samples' li() summed from zero in camera order (s = 0 .. S-1, S =
 * samples_root^2), then multiplied by 1.0 / (double)S, then to_byte per channel with A = 255 (img.rs:65-67) and / or the three doubles
 * before quantisation.  li() is lg_radiance's value for that ray, in the accel's traversal mode.  So for lg_accel_view's view the film is
 * lg_capture's and the doubles are lg_capture_radiance(0, 1, ..)'s, bit for bit; for lg_view_look_at's view they are those of a scene
 * rebuilt with that camera.  Non-finite fields are accepted as they are.  Every pixel of every film is written exactly once; nothing
 * outside n_views*width*height elements is touched.
 * views is a HOST array in both forms: it is copied before the call returns (through pinned staging, on the stream).
 * Everything else is lg_capture_rays' contract: always the level-by-level pipeline, LASGUN_WF_BUDGET_MB chunks (of whole 8 x 8 pixel
 * tiles x S; with S > 1 each chunk parks its samples and resolves them itself), one stream at a time per accel, the device form only
 * enqueues, bar the usual growth of scratch.  lg_accel_set_query_order plays no part: there is no ray array.  n_views == 0 is a
 * successful no-op.
 * Errors (non-zero, lg_last_error, nothing launched, no output touched): a NULL accel; NULL views with n_views > 0; both outputs NULL;
 * width or height 0; a samples_root of 0 or above 256; reserved != 0; views of one call that differ in samples_root (the uniform-samples
 * rule); n_views * ceil(width/8) * ceil(height/8) * S > 2^32 - 1 (work tiles are counted in 32 bits, as the other queries' are); a byte
 * size beyond SIZE_MAX; MORE THAN 32 LIGHTS or a recursion depth of 20 or more.  The device form adds: a pointer that is not device
 * memory of the accel's device, dev_rgba not 4-byte aligned, dev_rgb not 8-byte aligned, a buffer that ends beyond its allocation. */
int lg_view_look_at(lg_view *out, int perspective, double param, const double origin[3], const double look[3],
                    const double up[3], uint8_t supersampling);
int lg_scene_view(const lg_scene *, lg_view *out);     /* the scene's own camera as a view; device-free */
int lg_accel_view(const lg_accel *, lg_view *out);     /* ... of the scene the accel was built from */
int lg_view_rays(const lg_accel *, const lg_view *, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1,
                 uint32_t y1, double *rays);
int lg_view_rays_device(const lg_accel *, const lg_view *, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0,
                        uint32_t x1, uint32_t y1, double *dev_rays, void *hip_stream);
int lg_capture_views(const lg_accel *, const lg_view *views, size_t n_views, uint32_t width, uint32_t height,
                     uint8_t *rgba, double *rgb);                                   /* host arrays; synchronous */
int lg_capture_views_device(const lg_accel *, const lg_view *views, size_t n_views, uint32_t width, uint32_t height,
                            void *dev_rgba, double *dev_rgb, void *hip_stream);
/* View features: lg_capture_features' planes for the K cameras of a view batch in one call -- first-hit depth, shading normal, albedo,
 * coverage and ids beside every film of lg_capture_views, for a denoiser, a compositor, a segmentation label --, and one plane more that
 * only matters once there is more than one view: the world-space hit POINT, which is what reprojects a pixel of view A into view B
 * (temporal and multi-view denoising, stereo consistency, label transfer).  Without rebuilding the scene and the accel per camera and
 * without writing lg_view_rays' rays (48 bytes each) and lg_intersect's hits (96 bytes each): the rays are made in the kernel and at most
 * 60 bytes a pixel are written.  An EXTRA: no counterpart in the reference.  It is the two contracts above joined; nothing in it is new
 * arithmetic except point. */
typedef struct lg_view_features {
    float    *depth;     /* [n_views*width*height]     */
    float    *normal;    /* [n_views*width*height][3]  */
    float    *albedo;    /* [n_views*width*height][3]  */
    float    *coverage;  /* [n_views*width*height]     */
    uint32_t *id;        /* [n_views*width*height][4]: kind, prim, instance, material -- the last 16 bytes of an lg_hit */
    float    *point;     /* [n_views*width*height][3]: world space */
} lg_view_features;      /* 48 bytes; each pointer may be NULL, all NULL is an error */
/* lg_view_features itself is always a host struct; in the device form its members are device pointers.
 * Addressing: the element of (v, x, y) is at v*width*height + y*width + x, times the plane's elements per pixel -- whole films, as
 * lg_capture_views has them; there is no rectangle.  Every pixel of every requested plane is written exactly once; nothing outside
 * n_views*width*height elements is touched; a plane that is not requested is not touched.
 * Rays: the S = samples_root^2 rays of (v, x, y) are lg_view_rays' rays for view v and that pixel, s = 0 .. S-1 in camera order: the
 * expression spelled out under lg_capture_views.
 * Hit: sample s's hit is what lg_intersect returns for that ray, bit for bit, in the accel's traversal mode (reference, pruned,
 * LDS-resident scene, fast mode); a hit iff kind != 0.  lg_accel_set_query_order plays no part (there is no ray array to sort), and neither
 * do the interleave, subset and organisation settings of the captures.
 * depth, normal, albedo, coverage, id: lg_capture_features' accumulators, order and roundings word for word -- all f64, from +0.0, s
 * ascending, a miss adds nothing; inv = 1.0 / (double)S; depth the mean over the hits and +INFINITY where there are none; id sample 0's.
 * material_rgb follows the same rule (lg_accel_material_count x 3 doubles; required iff albedo is requested, ignored otherwise).  For
 * lg_accel_view's view these five planes are lg_capture_features' bytes for the full film.
 * point: psum[3] starts at +0.0; a hit adds lg_hit::p per component, the value lg_intersect reports.
 *   point[c] = nhit ? (float)(psum[c] * (1.0 / (double)nhit)) : 0.0f
 * -- depth's divisor, and lg_hit's zeros on a miss.
 * views is a HOST array in both forms: it is copied before the call returns (through pinned staging, on the stream).
 * Host form (synchronous): the planes come back into staging and reach the caller's arrays after the synchronise, so an error on the way
 * leaves them as they were.  Device form: it only enqueues on hip_stream, ONE launch whatever the size; one stream at a time per accel.
 * n_views == 0 is a successful no-op, answered before every other check.
 * Errors (non-zero, lg_last_error, nothing launched, no output touched): a NULL accel, views or out; all six planes NULL; albedo without
 * material_rgb; width or height 0, or above 2^32 - 8 (a tile's pixel coordinates are 32-bit); a samples_root of 0 or above 256;
 * reserved != 0; views of one call that differ in samples_root (the uniform-samples rule); n_views * ceil(width/8) * ceil(height/8) >
 * 2^32 - 1 (8 x 8 pixel tiles are counted in 32 bits; the samples run in a loop and do not count); a plane's byte size beyond SIZE_MAX;
 * in the device form a plane or table that is not device memory of the accel's device, is misaligned (id 16-byte aligned, material_rgb 8,
 * the float planes 4) or ends beyond its allocation.  More than 32 lights or a deep recursion is NOT an error here: nothing is shaded. */
int lg_capture_view_features(const lg_accel *, const lg_view *views, size_t n_views, uint32_t width, uint32_t height,
                             const lg_view_features *out, const double *material_rgb);          /* host arrays; synchronous */
int lg_capture_view_features_device(const lg_accel *, const lg_view *views, size_t n_views, uint32_t width, uint32_t height,
                                    const lg_view_features *dev_out, const double *dev_material_rgb, void *hip_stream);
/* Hit layers: the first max_layers surfaces along each ray in one call -- an x-ray or thickness image, wall thickness for a printability
 * check, ordered transparency and depth peeling, multi-return lidar, inside / outside of a closed solid by crossing parity, picking
 * through a window -- without the caller's own loop of lg_intersect calls that reads back 96 bytes a ray, moves every origin to just
 * behind its hit, compacts the rays still alive and uploads 48 bytes a ray, max_layers times over.  One launch walks each ray up to
 * max_layers times; the ray stays in registers between the walks; only the planes asked for are written.  An EXTRA; no counterpart in
 * the reference.
 * Segments: ray i is 6 doubles as for lg_intersect; any f64 is accepted as it is.  Segment 0 of ray i is that ray, bit for bit.  Layer j
 * is what lg_intersect returns for segment j, bit for bit, exact ties included, in the accel's traversal mode exactly as for the other
 * queries (reference, pruned, LDS-resident scene, fast mode); no switch of its own.  If layer j has kind != 0 and j + 1 < max_layers,
 * segment j+1 has the origin o'[c] = p[c] - ng[c]*0x1p-36 for c = 0, 1, 2, with p and ng layer j's lg_hit::p and lg_hit::ng: one f64
 * product and one f64 subtraction per component, nothing fused -- the origin the render gives a glass hit's transmitted ray (the
 * reference's N::epsilon() * 2^16 step through the surface).  Segment j+1 keeps the direction of ray i bit for bit.  If layer j is a
 * miss, the ray is finished.
 * Planes (lg_layers_out) are LAYER-MAJOR: element (j, i) is at j*n + i, so each layer is a plane of n -- what depth peeling calls a
 * layer.  Every element of every plane asked for is written, whatever the buffers held before, by exactly one lane: no atomics, no
 * pre-fill.  hits = the whole lg_hit of layer j.  id = its kind, prim, instance, material.  along = the running parameter T_j: T_0 = t_0
 * and T_j = T_(j-1) + t_j, with t_j layer j's lg_hit::t, added sequentially in f64 -- the 2^-36 steps are NOT added, so T_j runs behind the
 * parameter of layer j on ray i by up to j steps.  A NaN stays: where T_(j-1) is NaN, T_j is T_(j-1) bit for bit, and so for inside (IEEE
 * leaves open which of two NaNs a sum returns).  Behind a ray's last layer: hits holds lg_intersect's miss record (t = +INF, zeros,
 * kind 0, prim and instance ~0, material -1), id holds 0, ~0, ~0, -1, along holds +INF.  count[i] = the number of layers with kind != 0,
 * 0 .. max_layers; count[i] == max_layers means the ray may have been cut short.  inside[i] = t_1 + t_3 + t_5 + ...: the sequential
 * f64 sum, from +0.0, of t_j over the odd j < count[i] -- for a ray that starts outside every closed solid, the length travelled
 * inside material, in units of |d|.
 * lg_accel_set_query_order(1) is honoured exactly as lg_intersect honours it: the tiles are cut from the sorted order of the GIVEN rays,
 * every answer lands in its own ray's slots, the same bytes as order 0 (a query of 64 rays or fewer is walked as given).
 * Limits and errors: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors (non-zero,
 * lg_last_error, nothing launched, no output touched), for n > 0: max_layers == 0; n > (2^32 - 1) * 64 (64-ray tiles are counted in 32
 * bits), and n > 2^32 - 1 with the sorted order; n * max_layers or a plane's byte size that does not fit size_t; a NULL accel, rays or
 * out; all five planes NULL; in the device form also a pointer that is not device memory of the accel's device or is misaligned (rays 8
 * bytes; hits and id 16; along and inside 8; count 4), or a buffer that ends beyond its allocation.
 * Device form: dev_out is a HOST struct of device pointers; it only enqueues on hip_stream; one stream at a time per accel.  Host form
 * (synchronous): the rays go up, the planes come back into staging and are copied out at the end, so an error on the way leaves the
 * caller's arrays as they were.
 * Out of scope: no maximum range and no material filter -- the caller thresholds along and reads id; lanes are not re-packed after
 * rays end (a wave walks while any of its rays is alive); no multi-device split.  Where |p[c]| is so large that ng[c]*2^-36 is absorbed,
 * a segment may find the same surface again: the contract is still the loop above, and max_layers bounds it. */
typedef struct lg_layers_out {
    lg_hit   *hits;    /* [max_layers][n]     the whole record of layer j of ray i, at j*n + i */
    double   *along;   /* [max_layers][n]     running parameter T_j, +INF behind the last layer */
    uint32_t *id;      /* [max_layers][n][4]  kind, prim, instance, material: the last 16 bytes of an lg_hit */
    uint32_t *count;   /* [n]                 layers found, 0 .. max_layers */
    double   *inside;  /* [n]                 t_1 + t_3 + t_5 + ... */
} lg_layers_out;       /* 40 bytes; each pointer may be NULL, all NULL is an error */
int lg_hit_layers(const lg_accel *, const double *rays, size_t n, uint32_t max_layers, const lg_layers_out *out); /* host arrays; synchronous */
int lg_hit_layers_device(const lg_accel *, const double *dev_rays, size_t n, uint32_t max_layers, const lg_layers_out *dev_out,
                         void *hip_stream);
/* Ray paths: follow each ray through up to max_bounces specular bounces in one call -- a laser or a lens bench through glass, room
 * acoustics and radio ray launching (K reflections with a gain per surface), a lidar's multipath returns, a caustic or photon pass from a
 * light, the specular chain of an integrator of one's own -- without the caller's own loop that traces, reads back 96 bytes a ray,
 * reflects or refracts on the host, offsets the origin by a guess, compacts the live rays and uploads 48 bytes a ray, max_bounces times
 * over.  One launch walks each ray up to max_bounces times; the ray stays in registers between the walks; only the planes asked for are
 * written.  This is NOT the path the render follows (its li() is a tree: glass spawns two children; its reflection goes through the
 * BSDF's local frame): it is a chain whose rule per material the caller gives.  An EXTRA; no counterpart in the reference.
 * The contract is a loop over lg_intersect:
 * Segments and vertices: ray i is 6 doubles as for lg_intersect; any f64 is accepted as it is.  Segment 0 of ray i is that ray, bit for
 * bit.  Vertex j is what lg_intersect returns for segment j, bit for bit, exact ties included, in the accel's traversal mode exactly as
 * for the other queries (reference, pruned, LDS-resident scene, fast mode); no switch of its own.  A miss ends the path with
 * LG_PATH_END_ESCAPED.
 * At a vertex: let p, ng, ns be the record's lg_hit::p, ::ng, ::ns, d the segment's direction and r = rules[material], with material the
 * record's lg_hit::material.  rules has exactly lg_accel_material_count entries (n_rules says so) and is a HOST array in both forms,
 * copied before the call returns: it may be freed on return.  A material outside 0 .. n_rules-1 is treated as LG_PATH_ABSORB.
 * LG_PATH_ABSORB: the path ends with LG_PATH_END_ABSORBED.  Otherwise gain = gain * r.gain (from 1.0, sequential in f64; a NaN stays:
 * where gain is NaN it is kept bit for bit, as along is), and then the next ray (o', d') is formed, all of it f64 with nothing fused and
 * dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z:
 *   N = normal ? ns : ng (normal: 0 uses lg_hit::ng, 1 uses lg_hit::ns).  s = dot(d, N).  If s > 0.0: N = -N and s = -s, per component.
 *   LG_PATH_REFLECT: k = 2.0*s; d'[c] = d[c] - k*N[c]; o'[c] = p[c] + ng[c]*0x1p-36.
 *   LG_PATH_PASS: d' is d's bits; o'[c] = p[c] - ng[c]*0x1p-36; medium ^= 1 -- the step of a hit layer.
 *   LG_PATH_REFRACT: L = sqrt(dot(d,d)), q = 1.0/L, u[c] = d[c]*q, ci = -dot(u,N).  eta = medium ? r.ior : 1.0/r.ior.
 *     sin2 = (eta*eta) * fmax(1.0 - ci*ci, 0.0), fmax the NaN-ignoring one.  If sin2 >= 1.0 (total internal reflection): REFLECT's two
 *     lines on d, no toggle.  Else ct = sqrt(1.0 - sin2), a = eta*ci - ct, w[c] = eta*u[c] + a*N[c], d'[c] = w[c]*L,
 *     o'[c] = p[c] - ng[c]*0x1p-36, medium ^= 1.
 * Inside or outside is the crossing parity in medium, not a normal's sign: lg_hit::ns of a sphere hit from inside faces the ray, so a
 * rule that reads the sign of d.ns never leaves a glass sphere.  medium starts at bit 0 of start_medium[i] (start_medium NULL: every ray
 * starts outside, 0); only bit 0 is read.  The offset is always along ng, the geometric normal, which faces -d.
 * After the next ray is formed: if any of the six components of (o', d') is not finite, the path ends with LG_PATH_END_DEGENERATE (gain
 * and medium as the forming left them).  Otherwise, if j + 1 == max_bounces, it ends with LG_PATH_END_CUT.  Otherwise segment j+1 is
 * (o', d').
 * Planes (lg_paths_out) per vertex are VERTEX-MAJOR: element (j, i) is at j*n + i.  hits = the whole lg_hit of vertex j.  point = its p
 * (3 doubles).  id = its kind, prim, instance, material.  along = the running sum of t: T_0 = t_0 and T_j = T_(j-1) + t_j, sequentially
 * in f64, the 2^-36 steps NOT added, in units of each segment's own |d|; a NaN stays (where T_(j-1) is NaN, T_j is T_(j-1) bit for bit).
 * Behind a path's last vertex: hits holds lg_intersect's miss record (t = +INF, zeros, kind 0, prim and instance ~0, material -1), id
 * holds 0, ~0, ~0, -1, point holds +0s, along holds +INF.
 * Planes per ray: count[i] = the number of vertices, 0 .. max_bounces.  end[i] = LG_PATH_END_*; LG_PATH_END_CUT goes with
 * count == max_bounces.  gain[i] as above.  medium[i] = the final bit.  last[i] = 6 doubles, origin then direction: for CUT the next ray
 * (o', d'); for ESCAPED the segment that missed; for ABSORBED and DEGENERATE the segment that found the last vertex.
 * Resuming: a call of a bounces, then a call of b bounces on last and medium of its CUT rays (as rays and start_medium), gives rows
 * a .. a+b-1 of one call of a+b, bit for bit, in hits, point and id; count (a + the second call's), end, last and medium agree too.
 * along and gain RESTART in the second call (from t_0 and from 1.0): the caller adds and multiplies.
 * Every element of every plane asked for is written, whatever the buffers held before, by exactly one lane: no atomics, no pre-fill.
 * lg_accel_set_query_order(1) is honoured exactly as lg_hit_layers honours it: the tiles are cut from the sorted order of the GIVEN
 * rays, every answer lands in its own ray's slots, the same bytes as order 0 (a query of 64 rays or fewer is walked as given).
 * Limits and errors, as for lg_hit_layers: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors
 * (non-zero, lg_last_error, nothing launched, no output touched), for n > 0: max_bounces == 0; n > (2^32 - 1) * 64, and n > 2^32 - 1
 * with the sorted order; n * max_bounces or a plane's byte size that does not fit size_t; a NULL accel, rays, rules or out; all nine
 * planes NULL; n_rules != lg_accel_material_count; an action above LG_PATH_REFRACT; reserved != 0; normal outside {0, 1}; in the device
 * form also a pointer that is not device memory of the accel's device or is misaligned (rays 8 bytes; hits and id 16; point, along, gain
 * and last 8; count, end, medium and start_medium 4), or a buffer that ends beyond its allocation.
 * Device form: dev_out is a HOST struct of device pointers, rules a HOST array; it only enqueues on hip_stream; one stream at a time per
 * accel.  Host form (synchronous): the rays go up, the planes come back into staging and are copied out at the end, so an error on the
 * way leaves the caller's arrays as they were.
 * Out of scope: branching (a glass vertex's two children: call twice with two tables); re-packing of lanes or re-sorting of rays between
 * bounces (a wave walks while any of its paths is alive); a maximum range; nested or overlapping media beyond the one parity bit;
 * multi-device. */
#define LG_PATH_ABSORB  0u   /* the path ends at this vertex */
#define LG_PATH_REFLECT 1u   /* mirror about the normal */
#define LG_PATH_PASS    2u   /* straight on, as a hit layer does */
#define LG_PATH_REFRACT 3u   /* Snell with `ior`; total internal reflection reflects */
typedef struct lg_path_rule {
    uint32_t action;    /* LG_PATH_* */
    uint32_t reserved;  /* 0 */
    double   ior;       /* LG_PATH_REFRACT: the material's index of refraction against the outside */
    double   gain;      /* multiplied into the path's gain at every vertex that does not absorb */
} lg_path_rule;         /* 24 bytes */
#define LG_PATH_END_CUT 0u        /* alive after max_bounces vertices: count == max_bounces */
#define LG_PATH_END_ESCAPED 1u    /* a segment missed */
#define LG_PATH_END_ABSORBED 2u
#define LG_PATH_END_DEGENERATE 3u /* the next ray had a non-finite component */
typedef struct lg_paths_out {
    lg_hit   *hits;    /* [max_bounces][n]     the whole record of vertex j of ray i, at j*n + i */
    double   *point;   /* [max_bounces][n][3]  its p, +0s behind the last vertex */
    uint32_t *id;      /* [max_bounces][n][4]  kind, prim, instance, material: the last 16 bytes of an lg_hit */
    double   *along;   /* [max_bounces][n]     running sum of t, +INF behind the last vertex */
    uint32_t *count;   /* [n]                  vertices found, 0 .. max_bounces */
    uint32_t *end;     /* [n]                  LG_PATH_END_* */
    double   *gain;    /* [n]                  product of the rules' gains */
    double   *last;    /* [n][6]               the ray to resume from, or the segment the path ended on */
    uint32_t *medium;  /* [n]                  the final parity bit */
} lg_paths_out;        /* 72 bytes; each pointer may be NULL, all NULL is an error */
int lg_trace_paths(const lg_accel *, const double *rays, size_t n, uint32_t max_bounces, const lg_path_rule *rules, size_t n_rules,
                   int normal, const uint32_t *start_medium, const lg_paths_out *out); /* host arrays; synchronous */
int lg_trace_paths_device(const lg_accel *, const double *dev_rays, size_t n, uint32_t max_bounces, const lg_path_rule *rules,
                          size_t n_rules, int normal, const uint32_t *dev_start_medium, const lg_paths_out *dev_out, void *hip_stream);
/* Light groups: li() of each ray split by subsets of the scene's lights, n_groups planes from one call -- light-group AOVs for
 * compositing, re-lighting a frame afterwards by changing intensities and colours, a light-mixing slider, a per-light contribution for
 * light placement -- without a scene and an accel rebuilt and a render repeated per group.  Nothing a walk finds depends on which
 * lights are counted, so every group shares ONE chain of closest-hit and shadow walks; only the sums over the lights and the combine
 * of the specular children carry n_groups planes.  li() is linear in the lights' intensities, so the planes of single lights, of the
 * ambient term alone and of the empty group re-light a frame without tracing again.  An EXTRA; no counterpart in the reference.
 * Groups: bit l of `lights` names light l, in lg_scene_add_point_light order; LG_GROUP_AMBIENT in `flags` makes the scene's ambient term
 * part of the group.  Groups may overlap, repeat and be empty.  The background belongs to every group.
 * Output: radiance is GROUP-MAJOR, element (g, r, c) at (g*n + r)*3 + c: n_groups * n * 3 doubles.  Every element is written, whatever
 * the buffer held before, by exactly one lane: no atomics, no pre-fill.
 * Value: plane g is lg_radiance's value for ray r, bit for bit and in the accel's traversal mode, on an accel built from the same scene
 * with only the lights of groups[g].lights added, in their original order, and with the ambient colour (+0, +0, +0) unless
 * LG_GROUP_AMBIENT is set.  As arithmetic, at every hit of every recursion level: the lights' terms are added in light order from zero,
 * a light outside the mask skipped exactly as an invisible light is; the ambient term is added last, with the ambient colour replaced
 * by zero for a group without the flag (the product with the BSDF is still formed: a NaN there stays a NaN); a hit's li is
 * (output + reflected) + refracted per group with the same weights; a finished ray is (0 + li) * 1.0.  So a group with ALL lights and
 * LG_GROUP_AMBIENT holds lg_radiance's very bytes, and a group with no lights and no flag holds the "base": the background and what the
 * specular chain carries of it.  The render's shadow-skip stays valid: a hit where every light is irrelevant is one where each subset's
 * lights are.
 * Shared with lg_radiance: lg_accel_set_query_order(1) and the LASGUN_WF_BUDGET_MB chunks (the chunk also carries 24 * (n_groups - 1)
 * bytes per ray of every level of a recursive scene), always the level-by-level pipeline, lg_profile_* credit its kernels as a render's
 * (closest 0, combine and the deepest level's spread pass 1, shade 3).
 * Limits and errors: n == 0 is a successful no-op whatever the pointers are.  Errors (non-zero, lg_last_error, nothing launched, no
 * output touched), for n > 0: n_groups == 0 or > LG_MAX_LIGHT_GROUPS; a `lights` bit at or above the scene's light count
 * (lg_accel_light_count); an unknown `flags` bit; a scene with more than 32 lights or a recursion depth of 20 or more (lg_radiance's two
 * refusals); n > (2^32 - 1) * 64, and n > 2^32 - 1 with the sorted order; n * n_groups * 24 that does not fit size_t; a NULL accel,
 * rays, groups or radiance; in the device form also rays or radiance that is not 8-byte aligned device memory of the accel's device or
 * ends beyond its allocation.  `groups` is a HOST array in both forms: it travels by value in the launches' arguments and may be freed
 * when the call returns.
 * Device form: it only enqueues on hip_stream, with lg_radiance_device's exceptions (growing the level arrays, the sort's scratch).
 * One stream at a time per accel.  Host form (synchronous): the planes come back into staging and are copied out at the end, so an
 * error on the way leaves the caller's array as it was.
 * Out of scope: films per group, groups for gathers, views and the render's own entry points, more than 32 lights, a background flag. */
typedef struct lg_light_group {
    uint32_t lights;   /* bit l: light l, in lg_scene_add_point_light order */
    uint32_t flags;    /* LG_GROUP_AMBIENT or 0 */
} lg_light_group;      /* 8 bytes */
#define LG_GROUP_AMBIENT 1u      /* the scene's ambient term is part of the group */
#define LG_MAX_LIGHT_GROUPS 64
int lg_radiance_groups(const lg_accel *, const double *rays, size_t n, const lg_light_group *groups, size_t n_groups,
                       double *radiance);                                   /* host arrays; synchronous */
int lg_radiance_groups_device(const lg_accel *, const double *dev_rays, size_t n, const lg_light_group *groups /* host */, size_t n_groups,
                              double *dev_radiance, void *hip_stream);
/* Surface scatter: one level of li()'s tree, opened -- for each ray its hit, the light and ambient sum at it, and the two specular
 * children with the factors the render multiplies their li by.  For an integrator of one's own over the render's own materials:
 * per-bounce AOVs (direct, first reflection, first refraction), a recursion depth chosen per call or per ray, Russian roulette, a path
 * tracer in torch over lasgun's plastic, metal and glass, a debugger that shows why a pixel is the colour it is -- without restating
 * the shading, which could never match bit for bit: the shading frame's tangents are in no record the library returns.  lg_trace_paths
 * is a chain with the caller's rules; this is the render's own tree, one level at a time.  An EXTRA; no counterpart in the reference.
 * Rays: ray i is 6 doubles as for lg_intersect; any f64 is accepted as it is.
 * hits[i] is lg_intersect's record of ray i, bit for bit, exact ties included, in the accel's traversal mode exactly as for the other
 * queries (reference, pruned, LDS-resident scene, fast mode); no switch of its own.
 * For a hit (kind != 0), with sh the render's shading record of it (p, ng, ns, the tangent ss, wo = -normalize(d)):
 *   direct[i] = the sum over the scene's lights, in lg_scene_add_point_light order from zero, of the visible lights' terms, then the
 *     ambient term added last (integrate.rs:47-67): the value the render's shade pass computes before any child is added.  A light is
 *     visible by the render's shadow test: the segment from p + ng*(2^-52 * 2^16) to the light is walked any-hit and the light counts iff
 *     !(t < 1.0).  The walk is the render's own shadow pass, shadow-skip included.
 *   The children are what the render's shade pass makes at a depth below the maximum (integrate.rs:69-77), whatever depth the accel
 *   has: only glass and mirror materials have any; the transmitted child exists iff the BSDF samples one and
 *   !(pdf <= 0 || spectrum == 0 || |wi . ns| == 0), the reflected child iff the BSDF samples one and
 *   !(pdf <= 0 || spectrum == 0 || wi . ns <= 0).  flags[i] = LG_SCATTER_HIT | LG_SCATTER_REFLECT and / or LG_SCATTER_REFRACT.
 *   reflect[i] = origin p + ng*(2^-52 * 2^16), direction -wo + 2 (wo . ns) ns (f64, nothing fused); reflect_weight[i] = the sample's
 *     spectrum (integrate.rs:103).
 *   refract[i] = origin p - ng*(2^-52 * 2^16) (= p - ng*2^-36), direction the sample's wi; refract_weight[i] = spectrum[3], |wi . ns|,
 *     pdf (integrate.rs:129).  These are the eight doubles the render parks per hit for its combine pass, and the six per child it
 *     appends to the next level's rays, the same bits.
 * For a miss: hits[i] is lg_intersect's miss record, direct[i] = background(normalize(d)) -- the value li() returns --, flags[i] = 0.
 * An absent child's ray and weight elements are +0.0.
 * The scene's max_recursion_depth plays no part: the same scene built at two depths gives the same bytes.
 * Composition -- what makes the planes usable.  With D a depth of the caller's choosing, + and * componentwise in f64, nothing fused:
 *   L(ray, d) = direct                                   for a miss;
 *             = (direct + 0) + 0                         for a hit with d == D;
 *             = (direct + R) + T                         otherwise, with
 *       R = reflect_weight * L(reflect, d+1), or +0 if the child is absent,
 *       T = ((spectrum * L(refract, d+1)) * cos) / pdf, or +0 if absent  (cos, pdf: refract_weight[3], [4]).
 *   (0 + L(ray, 0)) * 1.0 is lg_radiance's value for that ray on an accel of the same scene built at max_recursion_depth D, bit for bit
 *   (the sum from zero and the product by one are the reference's pixel sum of one sample; they turn a -0.0 into +0.0).  A scene
 *   without glass or mirror has no children at any depth.
 * NaNs: where an input makes the hit's geometry NaN (a ray with a NaN or infinite component, a degenerate primitive), an element that
 * is NaN in the render's own arithmetic is SOME NaN here: its sign and payload are not part of the contract (IEEE leaves open which
 * of two NaNs an operation returns, and the compiler may order commutative operands differently per kernel).  Every finite element,
 * every +-INF and every zero's sign is bit for bit.
 * Every element of every plane asked for is written, whatever the buffers held before, by exactly one lane: no atomics, no pre-fill.
 * lg_accel_set_query_order(1) is honoured exactly as lg_radiance honours it: the chunks are cut from the sorted order of the GIVEN
 * rays, every answer lands in its own ray's rows, the same bytes as order 0 (a query of 64 rays or fewer is walked as given).
 * Shared with lg_radiance: always the level-by-level pipeline, as a chain of one level; the LASGUN_WF_BUDGET_MB chunks (a chunk parks
 * its hits' frames and visibility words; the planes are the caller's); lg_profile_* credit its kernels as a render's (closest 0,
 * shadow 2, the emit pass 3).
 * Limits and errors, as for lg_hit_layers: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors
 * (non-zero, lg_last_error, nothing launched, no output touched), for n > 0: n > (2^32 - 1) * 64, and n > 2^32 - 1 with the sorted
 * order; a plane's byte size that does not fit size_t; a NULL accel, rays or out; all seven planes NULL; a scene with more than 32
 * lights (lg_radiance's refusal; the accel's recursion depth is never a reason to refuse); in the device form also a pointer that is
 * not device memory of the accel's device or is misaligned (rays 8 bytes; hits 16; direct, reflect, reflect_weight, refract and
 * refract_weight 8; flags 4), or a buffer that ends beyond its allocation.
 * Device form: dev_out is a HOST struct of device pointers; it only enqueues on hip_stream, with lg_radiance_device's exceptions
 * (growing the chunk's arrays, the sort's scratch); one stream at a time per accel.  Host form (synchronous): the rays go up, the planes
 * come back into staging and are copied out at the end, so an error on the way leaves the caller's arrays as they were.
 * Out of scope: the visibility word as a plane; BSDF evaluation for a caller-supplied wi; non-specular sampling; a multi-device split;
 * re-packing of lanes (the emit pass runs over the render's hit queue as it is). */
#define LG_SCATTER_HIT     1u   /* the ray hit a surface: hits[i].kind != 0 */
#define LG_SCATTER_REFLECT 2u   /* the reflected child is present */
#define LG_SCATTER_REFRACT 4u   /* the transmitted child is present */
typedef struct lg_scatter_out {
    lg_hit   *hits;            /* [n]     lg_intersect's record of ray i */
    double   *direct;          /* [n][3]  hit: lights in order + ambient (integrate.rs:47-67); miss: the background li() returns */
    uint32_t *flags;           /* [n]     LG_SCATTER_HIT 1, LG_SCATTER_REFLECT 2, LG_SCATTER_REFRACT 4 */
    double   *reflect;         /* [n][6]  the reflected child's ray */
    double   *reflect_weight;  /* [n][3]  its spectrum (integrate.rs:103) */
    double   *refract;         /* [n][6]  the transmitted child's ray */
    double   *refract_weight;  /* [n][5]  spectrum[3], |wi . ns|, pdf (integrate.rs:129) */
} lg_scatter_out;              /* 56 bytes; each pointer may be NULL, all NULL is an error */
int lg_scatter(const lg_accel *, const double *rays, size_t n, const lg_scatter_out *out);           /* host arrays; synchronous */
int lg_scatter_device(const lg_accel *, const double *dev_rays, size_t n, const lg_scatter_out *dev_out, void *hip_stream);
/* Lit scatter: lg_scatter under lights that come with the CALL.  lg_scatter's `direct` counts the at most 32 point lights the scene held
 * when lg_accel_from ran; here the call brings K point lights (0 .. LG_MAX_CALL_LIGHTS), one table shared by every ray or a table per ray,
 * and an ambient colour, and hands out every light's own term and the visibility bits beside the sum.  For what an integrator of one's own
 * needs of the render's BSDF: area and environment lights as samples (a new set per call, or per vertex for next-event estimation: each
 * ray brings its own), more than 32 lights, and a light that moves -- no scene and no accel is rebuilt, the closest-hit walks do not
 * depend on the lights at all.  An EXTRA; no counterpart in the reference.
 * Lights: lg_light is lg_scene_add_point_light's arguments (position, intensity, falloff[3]: constant, linear, quadratic), 72 bytes; any
 * f64 is accepted as it is.  per_ray == 0: lights[count], shared by every ray; per_ray == 1: lights[n][count], ray i's lights at
 * lights[i * count ..].  `ambient` stands where the scene's ambient colour stands.
 * Scatter planes: hits, flags, reflect, reflect_weight, refract and refract_weight are lg_scatter's, bit for bit -- the traversal mode, the
 * exact ties, the NaN rule and the +0.0 of an absent child all as there.  The scene's own lights and ambient colour play no part in any
 * plane; a scene with more than 32 lights is accepted.
 * For a hit, with sh the render's shading record, L_k ray i's light k, all arithmetic f64 with nothing fused:
 *   light k is visible iff the any-hit walk of the segment from sh.p (= p + ng * 2^-36) with direction L_k.position - sh.p answers
 *     !(t < 1.0): lg_occluded of that ray, negated;
 *   term_k = mul_ew(PI * intensity, bsdf_f(..)) * wi_dot_n / f_att, the render's expression for a point light (integrate.rs:53-62), and it
 *     is added iff the light is visible and f_att != 0.0;
 *   direct[i] = the sequential sum over k = 0 .. K-1 from +0.0 of the added terms, then mul_ew(ambient, bsdf_f(.., ns, ..)) added last: on
 *     an accel of the same scene rebuilt with exactly these lights and this ambient, lg_scatter's direct, the same bytes;
 *   terms[i][k] = +0.0 + term_k where the term is added, +0.0 otherwise (the sum from zero turns a -0.0 into +0.0: the plane equals a
 *     single-light group of lg_radiance_groups at depth 0);
 *   visible[i][k >> 5] bit k & 31 is set iff light k is visible by the test above, whatever its f_att and whether or not its term could
 *     matter; W = ceil(K / 32) words a ray; bits at or above K are 0.
 * For a miss: direct[i] is the background, as lg_scatter's; its terms are +0.0 and its visible words 0.
 * K == 0: no shadow pass runs, direct is the ambient term alone; terms and visible have no elements (their pointers are not looked at).
 * Where `visible` is not asked for, the shadow pass may leave out the walk of a (hit, light) whose term cannot depend on it (the light is
 * on the other side of the surface for the BSDF and PI * intensity is finite: the term is a zero either way; or f_att == 0): direct and
 * terms are the same bytes with and without `visible`.
 * Every element of every plane asked for is written, whatever the buffers held before, by exactly one lane: no atomics, no pre-fill.
 * lg_accel_set_query_order(1) is honoured as lg_scatter honours it; a per-ray light row follows its ray's index, not its slot.  The
 * LASGUN_WF_BUDGET_MB chunks are the pipeline's own (a chunk parks its hits' frames and W visibility words a hit); lg_profile_* credit the
 * kernels as lg_scatter's (closest 0, shadow 2, the emit pass 3).
 * Limits and errors: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors (non-zero,
 * lg_last_error, nothing launched, no output touched), for n > 0: lg_scatter's own except the scene's light count; a NULL `lights`;
 * count > LG_MAX_CALL_LIGHTS; per_ray not 0 or 1; count > 0 with a NULL table; all nine planes NULL (with K == 0: all seven scatter
 * planes); n * K * 72, n * K * 24 or n * W * 4 that does not fit size_t; in the device form also a pointer that is not device memory of
 * the accel's device, is misaligned (lg_scatter's; terms and a per-ray table 8 bytes, visible 4) or ends beyond its allocation.
 * Device form: dev_out is a HOST struct of device pointers.  lights->lights is DEVICE memory when per_ray == 1 (it is as large as the
 * rays); when per_ray == 0 it is a HOST table, staged into a table of the call's own on the stream: it may be freed on return.  It only
 * enqueues on hip_stream, with lg_scatter_device's exceptions; one stream at a time per accel.  Host form (synchronous): everything is
 * host memory; the planes come back into staging and are copied out at the end, so an error on the way leaves the caller's arrays as
 * they were.
 * Out of scope: lights for the other radiance entry points; emitters that are not points (the caller samples them: the emitter's cosine
 * and pdf are applied to `terms` by the caller); sampling the lights on the device; a multi-device split. */
#define LG_MAX_CALL_LIGHTS 1024u
typedef struct lg_light { double position[3], intensity[3], falloff[3]; } lg_light;   /* 72 bytes: lg_scene_add_point_light's arguments */
typedef struct lg_light_set {
    const lg_light *lights;  /* per_ray == 0: [count], shared by every ray; per_ray == 1: [n][count], ray i's lights at lights[i*count ..] */
    uint32_t count;          /* K, 0 .. LG_MAX_CALL_LIGHTS */
    uint32_t per_ray;        /* 0 or 1 */
    double ambient[3];       /* stands where the scene's ambient colour stands */
} lg_light_set;              /* 40 bytes */
typedef struct lg_lit_out {
    lg_scatter_out scatter;  /* the seven planes of lg_scatter; `direct` is under the CALL's lights and ambient */
    double   *terms;         /* [n][K][3] */
    uint32_t *visible;       /* [n][W], W = ceil(K/32): bit k&31 of word k>>5 */
} lg_lit_out;                /* 72 bytes; each pointer may be NULL, all nine NULL is an error */
int lg_scatter_lit(const lg_accel *, const double *rays, size_t n, const lg_light_set *lights, const lg_lit_out *out);   /* host arrays; synchronous */
int lg_scatter_lit_device(const lg_accel *, const double *dev_rays, size_t n, const lg_light_set *lights, const lg_lit_out *dev_out, void *hip_stream);
/* Hit attributes: where on the primitive a ray's hit lies, and the frame the render shades it in.  lg_hit says which primitive was hit
 * (kind, prim, instance); these planes say where on it: the barycentrics of a triangle hit (to interpolate vertex attributes of the
 * caller's own: colours, labels, skinning weights, flow), a surface parameter (u, v) to texture the hit with, the hit point in the
 * primitive's own space (a procedural texture that sticks to an instanced, rotated or scaled object) and the tangents of the render's
 * BSDF (an anisotropic lobe of the caller's own; lg_scatter's transmitted direction restated).  The render computes all of it for every
 * shaded hit; this hands it out.  An EXTRA; no counterpart in the reference.  Everything is f64, nothing is fused.
 * Two forms.  The WALKING form (lg_hit_attributes*) finds each ray's closest hit and resolves it: hits[i] is lg_intersect's record of
 * ray i, bit for bit, exact ties included, in the accel's traversal mode exactly as for the other queries (reference, pruned,
 * LDS-resident scene, fast mode); lg_accel_set_query_order(1) is honoured as lg_intersect honours it (the same bytes, each answer in
 * its own ray's rows; a query of 64 rays or fewer is walked as given).  flags[i] = 0 for a miss, LG_ATTR_HIT for a hit.  A miss writes
 * +0.0 into every other plane.  The _OF form (lg_hit_attributes_of*) walks nothing: it resolves the primitive a record NAMES -- a
 * record of lg_intersect, of a layer of lg_hit_layers, of a vertex of lg_trace_paths, or a compacted subset of them -- for the ray given
 * with it.  Only kind, prim and instance of each record are read; out->hits must be NULL.
 * The attributes are a pure function of (ray, kind, prim, instance).  With lr = the ray taken into the primitive's accel-local space by
 * the inverse transforms of the accels on the chain root .. instance, in order (bvh.rs:462), the primitive's own intersector is run on
 * lr as the render's hit resolution runs it, giving t.  Then:
 *   local = lr.o + lr.d * t; for a sphere taken before the centre is subtracted and before the pole nudge.
 *   bary  = e0*invdet, e1*invdet, e2*invdet of Triangle::intersect (triangle.rs:161-251): the weights of the face's first, second and
 *     third vertex; +0.0 for a sphere or a box.
 *   uv, triangle: u = (b0*u0 + b1*u1) + b2*u2 and v likewise, (u_k, v_k) the face's texture coordinates widened from f32; where the
 *     mesh has none, the reference's default (0,0), (1,0), (1,1) (triangle.rs:257-262).
 *   uv, sphere: u = phi / (2.0*PI), v = theta / PI, phi and theta Sphere::intersect's own (sphere.rs:79-123), the p.x = 1e-5*r nudge at
 *     a pole and the +2*PI wrap of a negative phi included, in the library's portable atan2 and acos (lg_math_eval ops 4 and 5).
 *   uv, box: with j and k the axes the hit face's two differentials point along (cuboid.rs:126-130, in the order the intersector
 *     returns them), u = (local[j] - min[j]) / (max[j] - min[j]) and v likewise with k; a flat box gives whatever IEEE gives.
 *   bary, uv and local are primitive-local: no transform and no swap_backface changes them.
 *   dp    = gu, gv: the geometric dpdu and dpdv after transform_ray_intersection of every accel on the way up (transform.rs:243-264)
 *     and the backface swaps (surface.rs:88-99): what the render's shading receives.  lg_hit::ng is
 *     face_forward(normalize(cross(gu, gv)), -normalize(d)).
 *   frame = ss, ts: ss = normalize(the surface dpdu carried up the same way), ts = cross(ns, ss) with ns lg_hit's: the tangents of the
 *     render's BSDF (bsdf.rs:34-35).
 * _of form, per record: kind == 0 gives flags 0 and +0.0 in every plane.  A record that names no primitive of this accel gives
 * LG_ATTR_BAD_RECORD and +0.0, and nothing is dereferenced through it: kind > 3; instance >= the accel's instance count; prim >= the
 * count of its kind, or for a triangle >= the face count of the mesh that `instance` is; a sphere or box that does not sit in
 * `instance`.  A named primitive whose own test rejects the ray gives LG_ATTR_NO_HIT and +0.0: a triangle where Triangle::intersect's
 * tests up to t fail, a box where Bounds::intersect misses, a sphere with t < 0 (as bvh.rs accepts).  No comparison with another
 * primitive's t is made.  Every other record gives LG_ATTR_HIT and the attributes above.  Given lg_intersect's own records of the same
 * rays, the planes are the walking form's, the same bytes.
 * NaNs: SOME NaN, as for lg_scatter -- an element that is NaN in the render's own arithmetic is a NaN here, its sign and payload no
 * part of the contract; every finite element, every +-INF and every zero's sign is bit for bit.
 * Every element of every plane asked for is written, whatever the buffers held before, by exactly one lane: no atomics, no pre-fill.
 * Nothing is shaded: lights, materials and the recursion depth play no part, and a scene of 40 lights is accepted.
 * Limits and errors, as for lg_hit_layers: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors
 * (non-zero, lg_last_error, nothing launched, no output touched), for n > 0: n > (2^32 - 1) * 64, and in the walking form n > 2^32 - 1
 * with the sorted order; a plane's byte size that does not fit size_t; a NULL accel, rays or out; all planes NULL; in the _of form a
 * NULL `hits` argument or a non-NULL out->hits; in the device forms also a pointer that is not device memory of the accel's device or
 * is misaligned (rays 8 bytes; hits 16; flags 4; bary, uv, local, frame and dp 8), or a buffer that ends beyond its allocation.
 * Device forms: dev_out is a HOST struct of device pointers; they only enqueue on hip_stream (the walking form with lg_intersect_device's
 * exception for the sort's scratch); one stream at a time per accel.  Host forms (synchronous): the rays (and records) go up, the
 * planes come back into staging and are copied out at the end, so an error on the way leaves the caller's arrays as they were.
 * Out of scope: texture lookup itself; ray differentials; a maximum range in the walk; a multi-device split. */
#define LG_ATTR_HIT        1u   /* resolved: the planes hold the attributes */
#define LG_ATTR_NO_HIT     2u   /* _of form: the record names a primitive this ray does not hit */
#define LG_ATTR_BAD_RECORD 4u   /* _of form: the record names no primitive of this accel */
typedef struct lg_attr_out {
    lg_hit   *hits;            /* [n]     lg_intersect's record of ray i (walking form only; must be NULL in the _of form) */
    uint32_t *flags;           /* [n]     0, LG_ATTR_HIT 1, LG_ATTR_NO_HIT 2, LG_ATTR_BAD_RECORD 4 */
    double   *bary;            /* [n][3]  triangle: b0, b1, b2; otherwise +0.0 */
    double   *uv;              /* [n][2] */
    double   *local;           /* [n][3]  the hit point in the primitive's accel-local space */
    double   *frame;           /* [n][6]  ss, ts: the BSDF's tangents (bsdf.rs:34-35) */
    double   *dp;              /* [n][6]  gu, gv: world-space geometric dpdu, dpdv as the render's shading receives them */
} lg_attr_out;                 /* 56 bytes; each pointer may be NULL, all NULL is an error */
int lg_hit_attributes(const lg_accel *, const double *rays, size_t n, const lg_attr_out *out);         /* host arrays; synchronous */
int lg_hit_attributes_device(const lg_accel *, const double *dev_rays, size_t n, const lg_attr_out *dev_out, void *hip_stream);
int lg_hit_attributes_of(const lg_accel *, const double *rays, const lg_hit *hits, size_t n, const lg_attr_out *out);   /* host arrays; synchronous */
int lg_hit_attributes_of_device(const lg_accel *, const double *dev_rays, const lg_hit *dev_hits, size_t n, const lg_attr_out *dev_out,
                                void *hip_stream);

/* Closest points: for each of n POINTS, the nearest surface point of the scene, its distance and the primitive it lies on -- the query
 * that starts from a point and not from a ray (collision and clearance probes, lidar and robotics pipelines, probe placement; with
 * lg_hit_layers' parity, a signed distance).  An EXTRA; no counterpart in the reference: the contract is the arithmetic below, and the
 * answer is that arithmetic over ALL primitives of the scene, bit for bit -- it depends on neither the trees nor the visit order, and
 * the accel's traversal mode (reference, pruned, LDS-resident scene, fast mode) and lg_accel_set_query_order play no part: the same
 * bytes in every mode.  `points` is n x 3 f64, world space.  All f64, nothing fused, dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * World position: W_A(x) takes a point of accel A's local space to world space: A's own transform applied as the library applies a
 *   transform to a point (((c0*x + c1*y) + c2*z) + c3*1.0 per component), then its parent's, and so on up to and including the root's.
 * Triangle (kind 3): the triangle the ray walk sees -- the first three vertices of a face, f32 positions widened -- with its vertices
 *   a, b, c taken through W_A, A the mesh instance.  Closest point x of q (Ericson, Real-Time Collision Detection, 5.1.5), in this order:
 *   1. ab=b-a, ac=c-a, ap=q-a; d1=dot(ab,ap), d2=dot(ac,ap).  d1<=0 && d2<=0: x = a.
 *   2. bp=q-b; d3=dot(ab,bp), d4=dot(ac,bp).  d3>=0 && d4<=d3: x = b.
 *   3. vc=d1*d4-d3*d2.  vc<=0 && d1>=0 && d3<=0: x = a+ab*(d1/(d1-d3)).
 *   4. cp=q-c; d5=dot(ab,cp), d6=dot(ac,cp).  d6>=0 && d5<=d6: x = c.
 *   5. vb=d5*d2-d1*d6.  vb<=0 && d2>=0 && d6<=0: x = a+ac*(d2/(d2-d6)).
 *   6. va=d3*d6-d5*d4.  va<=0 && (d4-d3)>=0 && (d5-d6)>=0: x = b+(c-b)*((d4-d3)/((d4-d3)+(d5-d6))).
 *   7. otherwise den=1/((va+vb)+vc), x = (a+ab*(vb*den))+ac*(vc*den).
 *   The candidate's squared distance is dot(q-x, q-x).
 * Box (kind 2): corner k (k = 0 .. 7) has the box's max on axis x / y / z where bit 0 / 1 / 2 of k is set and its min otherwise; the eight
 *   corners go through W_A.  The surface is twelve triangles of corners, in this order: -x (0,2,6) (0,6,4); +x (1,3,7) (1,7,5);
 *   -y (0,1,5) (0,5,4); +y (2,3,7) (2,7,6); -z (0,1,3) (0,3,2); +z (4,5,7) (4,7,6) -- each face cut by the diagonal from its lowest corner
 *   to its highest.  The lowest squared distance of the twelve wins, the first triangle a tie.  Under a general affine instance the box
 *   is a parallelepiped and this is exact for it.  A point inside a box gets the distance to its surface.
 * Sphere (kind 1), centre c and radius r: cw = W_A(c), pw = W_A(c + (r,0,0)), rw = sqrt(dot(pw-cw, pw-cw)); v = q-cw, l = sqrt(dot(v,v));
 *   d = fabs(l-rw), squared distance d*d; x = cw + v*(rw/l), and x = pw where l == 0.  A sphere is a sphere in world space only under a
 *   similarity: lg_scene_closest_gate below.  A point inside a sphere gets the distance to its surface.
 * Winner: a candidate is admissible iff its squared distance is <= radius*radius and < +INF (a NaN never wins).  The smallest squared
 *   distance among the admissible candidates wins; an exact tie goes to the smallest (instance, kind, prim) in lg_hit's numbering.
 *   distance = sqrt of the winner's squared distance, point = its x, id = kind, prim, instance, material -- lg_hit's last 16 bytes,
 *   material what lg_intersect reports for a hit on that primitive.  Where nothing is admissible, and for a point with a non-finite
 *   coordinate: distance = +INF, point = +0.0, id = 0, ~0, ~0, -1.
 * Every element of every plane asked for is written, whatever the buffers held, by exactly one lane: no atomics, no pre-fill.  Lights
 * and materials' parameters play no part; a scene of more than 32 lights is accepted.
 * lg_scene_closest_gate (no device is needed): -1 where every accel that holds a sphere has a cumulative linear part L (the 3 x 3 part
 *   of the composed transforms root .. accel) with L^T L within 2^-40, relative to its largest entry, of a multiple of the identity;
 *   otherwise the first accel (in lg_hit's instance numbering) that holds a sphere and fails it: lg_closest_points* then fail, naming
 *   that instance.  Meshes and boxes pass under any invertible affine chain.  -2 on an error.  shrink (may be NULL): shrink[a], for
 *   a < min(cap, instances), a proven lower bound of the smallest singular value of accel a's local -> world linear part (0 where
 *   nothing is proven: a singular or badly conditioned chain), which the kernel's pruning test uses.
 * Limits and errors: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors (non-zero,
 * lg_last_error, nothing launched, no output touched), for n > 0: a NULL accel, points or out; all three planes NULL; a radius that is
 * NaN or negative (+INF: no limit); n > (2^32 - 1) * 64, or a plane's byte size that does not fit size_t; a scene the gate refuses; a
 * scene whose trees are too deep for the kernel's per-lane stack (lg_scene_closest_depth; refused, never truncated); in the device form also a pointer that is
 * not device memory of the accel's device or is misaligned (points, distance and point 8 bytes; id 16), or a buffer that ends beyond
 * its allocation.  The device form only enqueues on hip_stream (dev_out is a HOST struct of device pointers; one stream at a time per
 * accel), except that an accel's first call builds and uploads the query's own tables after a synchronise.  The host form is
 * synchronous: the points go up, the planes come back into staging and are copied out at the end, so an error on the way leaves the
 * caller's arrays as they were.
 * Out of scope: per-point radii, the k nearest, a normal at the closest point, the sorted order, a multi-device split (per-point radii
 * and the k nearest are lg_nearest's, below). */
typedef struct lg_closest_out {
    double   *distance;        /* [n]     sqrt(d2) of the winner, +INF where nothing is admissible */
    double   *point;           /* [n][3]  the winner's closest point, world space; +0.0 for a miss */
    uint32_t *id;              /* [n][4]  kind, prim, instance, material: lg_hit's last 16 bytes; miss: 0, ~0, ~0, -1 */
} lg_closest_out;              /* 24 bytes; each pointer may be NULL, all NULL is an error */
int lg_closest_points(const lg_accel *, const double *points, size_t n, double radius, const lg_closest_out *out);   /* host arrays; synchronous */
int lg_closest_points_device(const lg_accel *, const double *dev_points, size_t n, double radius, const lg_closest_out *dev_out, void *hip_stream);
int lg_scene_closest_gate(const lg_scene *, double *shrink, int cap);
/* The entries of the kernel's per-lane stack that lg_closest_points* need for this scene, without a device: up to 32 fit the default 64 KiB
 * of dynamic LDS, up to LG_CLOSEST_MAX_DEPTH the 128 KiB the call raises the kernel's limit to; a scene that needs more is refused by the
 * call.  -1 on an error. */
#define LG_CLOSEST_MAX_DEPTH 64
int lg_scene_closest_depth(const lg_scene *);

/* Proximity queries: for each of n POINTS, under a radius of its own, the k NEAREST primitives of the scene in order, how many
 * primitives lie within the radius at all, and whether any does -- sphere-set collision checks (a robot or a character as spheres of
 * different radii against the world: `touch` alone), contact generation and clearance (a probe near an edge or a corner touches several
 * primitives: all of the nearest few, and how many lie within the margin).  An EXTRA, as lg_closest_points is; the contract is that
 * query's arithmetic kept for more than one winner, and the answer is that arithmetic over ALL primitives of the scene, bit for bit.
 * Candidates: one candidate per primitive of the scene: its (d2, x, key) exactly as lg_closest_points defines them -- W_A, Ericson's
 *   steps 1-7 for a triangle, a box as the best of its twelve triangles (ONE candidate per box), a sphere by centre and pole.  The key is
 *   instance << 34 | kind << 32 | prim in lg_hit's numbering.  The sphere gate (lg_scene_closest_gate) and the depth rule
 *   (lg_scene_closest_depth) are lg_closest_points' own.
 * Radius: the radius r_i of point i is radii[i] where `radii` is not NULL, otherwise `radius`.  Where radii is given, radius is not read
 *   and not checked.  A per-point radius that is NaN or < 0 makes that point a miss -- not an error: a device array cannot be checked
 *   before the launch, and the host form behaves the same.  -0.0 is zero.  A shared radius that is NaN or negative is an error, as in
 *   lg_closest_points.
 * Admissible and order: a candidate is admissible iff d2 <= r_i*r_i && d2 < +INF, r_i*r_i one f64 product (a NaN never is).  A point
 *   with a non-finite coordinate has no admissible candidate.  The admissible candidates are ordered ascending by (d2, key): the squared
 *   distance first, an exact tie by the key.
 * Slots: slot j (0-based) holds the j-th candidate of that order for j < min(count, k): distance = sqrt(d2), point = x, id = kind, prim,
 *   instance, material as in lg_closest_points, its material rule included.  Every other slot holds the miss row: distance = +INF,
 *   point = +0.0, id = 0, ~0, ~0, -1.  Hence, for a shared radius, slot 0 is lg_closest_points' planes byte for byte.  The slot planes are
 *   slot-major: element (j, i) at j*n + i, as lg_hit_layers' planes are layer-major.
 * count is the number of admissible candidates -- ALL of them, not capped at k; touch is 1 iff count > 0, else 0.
 * Writes: every element of every plane asked for is written, whatever the buffers held, by exactly one lane: no atomics, no pre-fill.
 * Traversal: the accel's traversal mode, lg_accel_set_query_order, lights and materials' parameters play no part: the same bytes in every
 *   mode; a scene of more than 32 lights is accepted.
 * k: 0 .. LG_NEAREST_MAX_K.  k == 0 is legal iff no slot plane (distance, point, id) is asked for; k > 0 with no slot plane is legal, and
 *   k then plays no part.
 * What it costs follows from the planes asked for.  touch alone: a point's walk ends at its first admissible candidate.  Slot planes
 *   without count: the walk leaves out what provably lies beyond the k-th best so far and beyond r_i.  count, with or without slot
 *   planes: every admissible candidate has to be met, so only r_i prunes -- at an infinite radius this visits every primitive for every
 *   point, by definition.
 * Limits and errors: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors (non-zero,
 *   lg_last_error, nothing launched, no output touched), for n > 0, in this order: a NULL accel, points or out; all five planes NULL; a
 *   shared radius that is NaN or negative (+INF: no limit); k > LG_NEAREST_MAX_K, or k == 0 with a slot plane; n > (2^32 - 1) * 64; n * k
 *   or a plane's byte size that does not fit size_t; a scene the gate refuses; a scene whose trees are too deep for the per-lane stack;
 *   a scene whose stack plus lists exceed the LDS a workgroup may have (below; refused, never truncated); in the device form also a
 *   pointer that is not device memory of the accel's device or is misaligned (touch 1 byte, count 4, points, radii, distance and point 8;
 *   id 16), or a buffer that ends beyond its allocation.
 * LDS: a workgroup of 256 lanes keeps per lane a stack of lg_scene_closest_depth entries of 8 bytes and, with a slot plane, a list of k
 *   entries of 20 bytes (d2, key, the primitive's leaf slot: a winner's x is evaluated again from it at the end, the same bits):
 *   lg_scene_nearest_lds(scene, k) = 256 * (8 * depth + 20 * k) bytes; no device is needed; 0 on an error (a NULL scene, k beyond
 *   LG_NEAREST_MAX_K).  The limit is 160 KiB on gfx950, and the call refuses exactly where lg_scene_nearest_lds(scene, k) exceeds it, k
 *   taken as 0 where no slot plane is asked for.  LG_NEAREST_MAX_K is 8 because 64 stack entries of 8 bytes and 8 list entries of 16
 *   bytes fill 160 KiB for 256 lanes; this list entry is 4 bytes wider, so a scene of depth 64 is answered up to k = 6, one of depth 60
 *   or less at every k.
 * Stream: the device form only enqueues on hip_stream (dev_out is a HOST struct of device pointers; one stream at a time per accel),
 *   with the one exception lg_closest_points_device already has: an accel's first call of either builds and uploads the query's own
 *   tables after a synchronise.  The host form is synchronous: points and radii go up, the planes come back into staging and are copied
 *   out at the end, so an error on the way leaves the caller's arrays as they were.
 * Out of scope: de-duplicating coplanar neighbours (two triangles that share an edge both answer a point nearest that edge, with the same
 *   d2); a normal at the point; world-space vertex tables or run skipping inside fat leaves -- the known remedy for slow meshes stays a
 *   separate piece of work --; the sorted order; a multi-device split. */
#define LG_NEAREST_MAX_K 8
typedef struct lg_nearest_out {
    uint8_t  *touch;           /* [n]        1 iff count > 0, else 0 */
    uint32_t *count;           /* [n]        the number of admissible candidates -- ALL of them, not capped at k */
    double   *distance;        /* [k][n]     slot-major: element (j, i) at j*n + i; sqrt(d2), +INF for an empty slot */
    double   *point;           /* [k][n][3]  the candidate's closest point, world space; +0.0 for an empty slot */
    uint32_t *id;              /* [k][n][4]  kind, prim, instance, material; empty slot: 0, ~0, ~0, -1 */
} lg_nearest_out;              /* 40 bytes; each pointer may be NULL, all NULL is an error */
int lg_nearest(const lg_accel *, const double *points, const double *radii, size_t n, double radius, uint32_t k, const lg_nearest_out *out);   /* host arrays; synchronous */
int lg_nearest_device(const lg_accel *, const double *dev_points, const double *dev_radii, size_t n, double radius, uint32_t k, const lg_nearest_out *dev_out,
                      void *hip_stream);
size_t lg_scene_nearest_lds(const lg_scene *, uint32_t k);

/* Segment proximity: for each of n SEGMENTS p0 .. p1, under a radius of its own, the nearest surface point of the scene to the segment,
 * the parameter of the segment's own closest point, the distance and the primitive -- a capsule (a robot link: a segment with a radius)
 * against the world, and a sphere swept from one pose to the next: "did it touch anything on the way from p0 to p1", the discrete form
 * of continuous collision detection, which sampled spheres miss for thin geometry and a ray, having no thickness, cannot answer.  An
 * EXTRA, as lg_closest_points and lg_nearest are; the contract is the arithmetic below, and the answer is that arithmetic over ALL
 * primitives of the scene, bit for bit.  `segments` is n x 6 f64, world space: p0, then p1.  All f64, nothing fused,
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x).
 * Candidates: one candidate (d2, s, x) per primitive: d2 the squared distance, s the segment's parameter -- the segment's own closest
 *   point is p0 + (p1-p0)*s --, x the point ON THE PRIMITIVE.  The primitive's world geometry is formed exactly as lg_closest_points forms
 *   it (W_A; f32 vertices widened; a box's eight corners; a sphere's cw and pw).  clamp(v) = v<=0 ? +0.0 : (v>=1 ? 1.0 : v); every s leaves
 *   through clamp or is a literal, so it is never -0.0.  The key is lg_nearest's: instance << 34 | kind << 32 | prim.
 * Degenerate segment (p0 == p1 in all three components): the candidate is lg_closest_points' own for p0, with s = +0.0: such a segment
 *   answers with lg_nearest's k = 1 bytes.
 * Triangle a, b, c: six sub-candidates in this order; the lowest d2 wins, the first a tie, a NaN d2 never replaces anything.
 *   1. Crossing (Ericson 5.3.6, two-sided): ab=b-a, ac=c-a, qp=p0-p1; n=cross(ab,ac); d=dot(qp,n); ap=p0-a; t=dot(ap,n); e=cross(qp,ap);
 *      v=dot(ac,e); w=-dot(ab,e); where d<0 all of d, t, v, w are negated.  Verdict: d>0 && d<+INF && t>=0 && t<=d && v>=0 && w>=0 &&
 *      v+w<=d; then s = clamp(t/d), y = p0+(p1-p0)*s, and the verdict is CONFIRMED iff the squared distance of y from the triangle by
 *      lg_closest_points' steps 1-7 is <= g*g, g = 2^-46 * the largest |component| of y, a, b, c (fmax).  Crosses iff both: d2 = +0.0,
 *      x = y.  (For a segment in the triangle's plane the signs are noise; the confirmation ties a false "crosses" to formed points.  A
 *      true crossing at a grazing angle may fail it and is then answered by 2-6 with a small d2 above zero.)
 *   2. lg_closest_points' triangle steps 1-7 for p0, s = 0.     3. The same for p1, s = 1.
 *   4. The segment against edge a .. b (Ericson 5.1.9 with EPSILON = 0), e0=a, e1=b: d1=p1-p0, d2v=e1-e0, r=p0-e0; A=dot(d1,d1),
 *      E=dot(d2v,d2v), f=dot(d2v,r).  A<=0 && E<=0: s=0, t=0.  Else A<=0: s=0, t=clamp(f/E).  Else c=dot(d1,r), and E<=0: t=0,
 *      s=clamp(-c/A); else b=dot(d1,d2v), den=A*E-b*b, s = den!=0 ? clamp((b*f-c*E)/den) : 0, t=(b*s+f)/E, then t<0: t=0, s=clamp(-c/A);
 *      t>1: t=1, s=clamp((b-c)/A).  c1=p0+d1*s, c2=e0+d2v*t, w=c1-c2: d2 = dot(w,w), x = c2.
 *   5. The same against edge b .. c.     6. The same against edge c .. a.
 *   Apart from the crossing's exact +0.0 every d2 is the squared length between a formed point of the segment and a formed point of the
 *   primitive, never an algebraic shortcut.
 * Box: its twelve triangles in lg_closest_points' order, each by the triangle rule; the lowest d2 wins, the first triangle a tie, a NaN
 *   never replaces anything.  A segment wholly inside a box gets the distance to its surface.
 * Sphere: pc=pw-cw, rw=sqrt(dot(pc,pc)); u=p1-p0, uu=dot(u,u); v0=p0-cw, v1=p1-cw; tt=dot(cw-p0,u); s* = uu>0 ? clamp(tt/uu) : 0;
 *   m=p0+u*s*, vm=m-cw, lmin=sqrt(dot(vm,vm)); l0=sqrt(dot(v0,v0)), l1=sqrt(dot(v1,v1)); the far endpoint is p1 iff l1>l0 (p0 on a tie), lmax
 *   its l and v its v0 or v1.
 *   lmin>rw: d=lmin-rw, d2=d*d, x=cw+vm*(rw/lmin), s=s*.   Else lmax<rw: d=rw-lmax, d2=d*d, x=cw+v*(rw/lmax) (pw where lmax==0), s=0 or 1.
 *   Else, where lmin<=rw && lmax>=rw && lmax<+INF, the segment crosses the surface: d2 = +0.0; B=dot(v0,u), C=dot(v0,v0)-rw*rw,
 *   disc=B*B-uu*C, q=sqrt(disc), s1=(-B-q)/uu, s2=(-B+q)/uu; s = clamp(s1) where 0<=s1<=1, else clamp(s2) where 0<=s2<=1, and x=p0+u*s;
 *   where rounding leaves neither root in range: s=s*, x=m.  Otherwise (a NaN): no candidate.
 * Radius, admissible, winner, material, writes, traversal: lg_nearest's rules, word for word.  radii may be NULL, and the shared radius
 *   then holds; a per-segment radius that is NaN or < 0 makes that segment a miss, not an error; a shared radius that is NaN or negative
 *   is an error; -0.0 is zero.  A candidate is admissible iff d2 <= r_i*r_i && d2 < +INF.  A segment with a non-finite coordinate is a
 *   miss.  The winner is the smallest (d2, key).  touch = 1 iff an admissible candidate exists; distance = sqrt(d2) of the winner, param its
 *   s, point its x, id = kind, prim, instance, material by lg_nearest's material rule; a miss: touch 0, distance +INF, param +0.0, point
 *   +0.0, id 0, ~0, ~0, -1.  Every element of every plane asked for is written by exactly one lane.  The accel's traversal mode,
 *   lg_accel_set_query_order and lights play no part; a scene of more than 32 lights is accepted.
 * What it costs: `touch` alone asked for: a segment's walk ends at its first admissible candidate.  Every other plane set keeps the best.
 * Limits and errors: n == 0 is a successful no-op that writes nothing, answered BEFORE every other check.  Errors (non-zero,
 *   lg_last_error, nothing launched, no output touched), for n > 0, in this order: a NULL accel, segments or out; all five planes NULL; a
 *   shared radius that is NaN or negative (+INF: no limit); n > (2^32 - 1) * 64; a byte size that does not fit size_t; a scene the gate
 *   refuses (lg_scene_closest_gate); a scene whose trees are too deep for the per-lane stack (lg_scene_closest_depth); in the device form
 *   also a pointer that is not device memory of the accel's device or is misaligned (touch 1 byte; segments, radii, distance, param and
 *   point 8; id 16), or a buffer that ends beyond its allocation.  LDS is the stack alone, 256 * 8 * depth bytes.
 * Stream: the device form only enqueues on hip_stream (dev_out is a HOST struct of device pointers; one stream at a time per accel), with
 *   the one exception its siblings have: an accel's first call of any of them builds and uploads the query's own tables after a
 *   synchronise.  The host form is synchronous and stages: an error on the way leaves the caller's arrays as they were.
 * Out of scope: k > 1 and counts; a time of impact along the segment (a true sphere cast: the FIRST s at which a sphere of radius r_i
 *   touches, where this gives the s of the closest approach); world-space vertex tables for fat leaves; a multi-device split. */
typedef struct lg_segments_out {
    uint8_t  *touch;           /* [n]     1 iff an admissible candidate exists */
    double   *distance;        /* [n]     sqrt(d2) of the winner, +INF for a miss */
    double   *param;           /* [n]     s in [0, 1]: the segment's own closest point is p0 + (p1 - p0) * s; +0.0 for a miss */
    double   *point;           /* [n][3]  the winner's point ON THE SURFACE, world space; +0.0 for a miss */
    uint32_t *id;              /* [n][4]  kind, prim, instance, material; miss: 0, ~0, ~0, -1 */
} lg_segments_out;             /* 40 bytes; each pointer may be NULL, all NULL is an error */
int lg_closest_segments(const lg_accel *, const double *segments /* [n][6]: p0, p1 */, const double *radii, size_t n, double radius, const lg_segments_out *out);
int lg_closest_segments_device(const lg_accel *, const double *dev_segments, const double *dev_radii, size_t n, double radius, const lg_segments_out *dev_out,
                               void *hip_stream);
/* The scene's point lights, the number of mask bits a light group may use; -1 for a NULL accel. */
int lg_accel_light_count(const lg_accel *);
/* Order in which a query's rays are walked: 0 (default) = as given; 1 = sorted on the device by a coherence key.
 * Results are identical bytes either way, in the caller's order. Any other value: non-zero return, lg_last_error.
 * The walk keeps a wave's 64 rays in step; rays that arrive in no particular order (collision probes, visibility between arbitrary
 * points, a caller's secondary rays) cost it 5-11 x what the same rays cost in camera order.  Mode 1 gives every
 * ray a 32-bit key -- its origin's cell in a grid over the scene's bounds, then its direction's cell in an octahedral map -- sorts
 * (key, index) pairs with a stable radix sort and walks the rays in that order, each answer written to its own ray's slot.  The sort is
 * enqueued ahead of the walk on the same stream and is part of the call's time: rays that are already coherent (lg_camera_rays in
 * their own order) pay for it and gain nothing -- 4096^2 camera rays in camera order: 3.07 -> 3.89 ms on the 1024-sphere headline scene,
 * 5.24 -> 6.66 ms on the glass torus, 7.13 -> 8.61 ms on the mixed scene; the same rays shuffled: 15.9 -> 4.6, 59.4 -> 7.8, 77.5 -> 10.1 ms
 *  --, which is why the default is 0.  A query of at most 64 rays is one wave's tile whatever
 * the order, and is walked as given.
 * The device forms still only enqueue, with one exception (like the measured choice's first calls): the first sorted query of a
 * stream, and the first one of more rays than any before it, grows the sort's scratch (16 bytes a ray) after a device-wide synchronise.
 * In mode 1 a query of more than 2^32 - 1 rays is an error before any launch (the order's indices are 32-bit). */
int lg_accel_set_query_order(const lg_accel *, int order);
int lg_accel_get_query_order(const lg_accel *);
/* The order mode 1 would walk these rays in:
 * perm[s] = index of the ray walked in slot s (a permutation of 0 .. n-1);
 * keys[i] (may be NULL) = ray i's 32-bit key.
 * perm is exactly the stable ascending sort of keys (for every n, one-tile queries included).
 * Device form: dev_perm and dev_keys must be 4-byte aligned device memory of the accel's device, checked like the query buffers before
 * anything is enqueued; it may grow the sort's scratch as a sorted query does.  n == 0 is a successful no-op; n > 2^32 - 1 an error. */
int lg_query_order(const lg_accel *, const double *rays, size_t n, uint32_t *perm, uint32_t *keys);
int lg_query_order_device(const lg_accel *, const double *dev_rays, size_t n, uint32_t *dev_perm, uint32_t *dev_keys, void *hip_stream);
/* The material behind lg_hit::material: the POD as the caller passed it (or lg_material_default()). */
int lg_accel_material(const lg_accel *, int32_t index, lg_material *out);
/* The accel behind lg_hit::instance: its parent (-1 for the root) and, for a mesh instance, the ObjRef it was added with (-1 for a group). */
int lg_accel_instance(const lg_accel *, uint32_t instance, int32_t *parent, int64_t *obj_ref);

/* Known-answer and arithmetic probes: run the DEVICE intersectors / math on one thread. */
int lg_kat_intersect(int kind, const double *params, const char *obj_text, size_t obj_len, const double origin[3],
                     const double d[3], double out[8]);
int lg_kat_surface_interaction(const double origin[3], const double d[3], double t, const double dpdu[3],
                               const double dpdv[3], double out_ng[3]);
int lg_math_eval(int op, size_t n, const double *a, const double *b, double *out);
/* Measured rates of the current device in GB/s: what 0 = HBM copy (16 bytes per lane, 1 GiB, read + written bytes),
 * 1 = aggregate LDS read rate (ds_read_b128, every CU streaming): the measured denominators of bench.py's roofline. */
int lg_probe_rate(int what, double *gbps);

#ifdef __cplusplus
}
#endif
#endif /* LASGUN_HIP_H */
