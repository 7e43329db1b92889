// include/lasgun.hpp -- header-only C++ host API over the C ABI (include/lasgun_hip.h).
//
// The reference's own toolchain (Rust) is absent from this pipeline, so the host side above
// the C ABI is C++: the same names, argument meaning and ownership rules as the reference's
// public surface, so a scene written against nfrasser/lasgun ports line by line:
//
//   lasgun::Scene      src/scene.rs:49-143        lasgun::Aggregate  src/scene/node.rs:35-115
//   lasgun::Material   src/material/mod.rs:15-46  lasgun::Camera     src/camera.rs:75-102
//   lasgun::Film       src/film.rs:22-45          lasgun::Accel      src/lib.rs:42
//   lasgun::capture / capture_subset / render     src/lib.rs:46-56,110
//
// Rust panics and `Result`s become exceptions (lasgun::Error, lasgun::ObjError).
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <algorithm>
#include <vector>
#include <utility>

#include "lasgun_hip.h"

namespace lasgun {

using Vec3 = std::array<double, 3>;

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct ObjError : Error { // obj::ObjError of scene.rs:120-130
    using Error::Error;
};

class Material { // Copy POD (material/mod.rs:3-4)
  public:
    lg_material m;
    static Material default_() { return {lg_material_default()}; }
    static Material matte(Vec3 kd, double sigma) { return {lg_material_matte(kd.data(), sigma)}; }
    static Material plastic(Vec3 kd, Vec3 ks, double roughness) { return {lg_material_plastic(kd.data(), ks.data(), roughness)}; }
    static Material metal(Vec3 eta, Vec3 k, double u, double v) { return {lg_material_metal(eta.data(), k.data(), u, v)}; }
    static Material glass(Vec3 kr, Vec3 kt, double eta) { return {lg_material_glass(kr.data(), kt.data(), eta)}; }
    static Material mirror(Vec3 kr) { return {lg_material_mirror(kr.data())}; }
};

using ObjRef = uint32_t; // scene.rs:44

class Aggregate {
  public:
    Aggregate() : h_(lg_aggregate_new()), owned_(true) {}
    Aggregate(const Aggregate &) = delete;
    Aggregate &operator=(const Aggregate &) = delete;
    Aggregate(Aggregate &&o) noexcept : h_(o.h_), owned_(o.owned_) { o.h_ = nullptr; }
    ~Aggregate() { if (h_ && owned_) lg_aggregate_free(h_); }

    void add_group(Aggregate &&child) { lg_aggregate_add_group(h_, child.release()); } // moves, as in Rust
    void add_sphere(Vec3 center, double radius, Material m) { lg_aggregate_add_sphere(h_, center.data(), radius, &m.m); }
    void add_cube(Vec3 origin, double dim, Material m) { lg_aggregate_add_cube(h_, origin.data(), dim, &m.m); }
    void add_box(Vec3 mn, Vec3 mx, Material m) { lg_aggregate_add_box(h_, mn.data(), mx.data(), &m.m); }
    void add_obj(ObjRef mesh) { lg_aggregate_add_obj(h_, mesh); }
    void add_obj_of(ObjRef mesh, Material m) { lg_aggregate_add_obj_of(h_, mesh, &m.m); }
    void swap_backface() { lg_aggregate_swap_backface(h_); }
    Aggregate &translate(Vec3 d) { lg_aggregate_translate(h_, d.data()); return *this; }
    Aggregate &scale(double x, double y, double z) { lg_aggregate_scale(h_, x, y, z); return *this; }
    Aggregate &rotate_x(double deg) { lg_aggregate_rotate_x(h_, deg); return *this; }
    Aggregate &rotate_y(double deg) { lg_aggregate_rotate_y(h_, deg); return *this; }
    Aggregate &rotate_z(double deg) { lg_aggregate_rotate_z(h_, deg); return *this; }
    Aggregate &rotate(double deg, Vec3 axis) { lg_aggregate_rotate(h_, deg, axis.data()); return *this; }

  private:
    friend class Scene;
    Aggregate(lg_aggregate *borrowed, bool owned) : h_(borrowed), owned_(owned) {}
    lg_aggregate *release() {
        if (!owned_) throw Error("cannot move a borrowed Aggregate");
        lg_aggregate *h = h_;
        h_ = nullptr;
        return h;
    }
    lg_aggregate *h_;
    bool owned_;
};

class Scene;
class Camera { // a view of scene.camera (the Rust setters hand out &mut Camera)
  public:
    void look_at(Vec3 origin, Vec3 look, Vec3 up) { lg_camera_look_at(s_, origin.data(), look.data(), up.data()); }
    void set_supersampling(uint8_t base) { lg_camera_set_supersampling(s_, base); }
    void set_aperture_radius(double r) { lg_camera_set_aperture_radius(s_, r); }

  private:
    friend class Scene;
    explicit Camera(lg_scene *s) : s_(s) {}
    lg_scene *s_;
};

class Scene {
  public:
    Scene() : h_(lg_scene_new()) {}
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;
    Scene(Scene &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~Scene() { if (h_) lg_scene_free(h_); }

    Aggregate root() { return Aggregate(lg_scene_root(h_), false); } // `scene.root` (pub field)
    Camera set_perspective_camera(double fov) { lg_scene_set_perspective_camera(h_, fov); return Camera(h_); }
    Camera set_orthographic_camera(double scale) { lg_scene_set_orthographic_camera(h_, scale); return Camera(h_); }
    void set_solid_background(Vec3 c) { lg_scene_set_solid_background(h_, c.data()); }
    void set_radial_background(Vec3 inner, Vec3 outer, double scale) { lg_scene_set_radial_background(h_, inner.data(), outer.data(), scale); }
    void set_ambient_light(Vec3 c) { lg_scene_set_ambient_light(h_, c.data()); }
    void set_mesh_smoothing(bool enabled) { lg_scene_set_mesh_smoothing(h_, enabled ? 1 : 0); }
    void set_max_recursion_depth(uint32_t d) { lg_scene_set_max_recursion_depth(h_, d); }
    void set_threads(size_t t) { lg_scene_set_threads(h_, t); }
    void add_point_light(Vec3 position, Vec3 intensity, Vec3 falloff) { lg_scene_add_point_light(h_, position.data(), intensity.data(), falloff.data()); }
    ObjRef parse_obj(const std::string &text) {
        ObjRef r = 0;
        if (lg_scene_parse_obj(h_, text.data(), text.size(), &r)) throw ObjError(lg_last_error());
        return r;
    }
    ObjRef load_obj(const std::string &path) {
        ObjRef r = 0;
        if (lg_scene_load_obj(h_, path.c_str(), &r)) throw ObjError(lg_last_error());
        return r;
    }
    void set_root(Aggregate &&node) { lg_scene_set_root(h_, node.release()); }
    const lg_scene *handle() const { return h_; }

  private:
    lg_scene *h_;
};

class Film {
  public:
    Film(uint32_t w, uint32_t h) : h_(lg_film_new(w, h)) {}
    Film(uint32_t w, uint32_t h, uint8_t *rgba) : h_(lg_film_wrap(w, h, rgba)) {} // Film::new_with_output
    explicit Film(lg_film *adopt) : h_(adopt) {}
    Film(const Film &) = delete;
    Film &operator=(const Film &) = delete;
    Film(Film &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~Film() { if (h_) lg_film_free(h_); }
    uint32_t w() const { return lg_film_width(h_); }
    uint32_t h() const { return lg_film_height(h_); }
    const uint8_t *pixels() const { return lg_film_pixels(h_); }
    lg_film *handle() { return h_; }

  private:
    lg_film *h_;
};

class Accel { // `Accel::from(&scene)`: borrows the scene, which must outlive it
  public:
    static Accel from(const Scene &scene) {
        lg_accel *a = lg_accel_from(scene.handle());
        if (!a) throw Error(lg_last_error());
        return Accel(a);
    }
    Accel(const Accel &) = delete;
    Accel &operator=(const Accel &) = delete;
    Accel(Accel &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~Accel() { if (h_) lg_accel_free(h_); }
    const lg_accel *handle() const { return h_; }
    // ray queries (lasgun_hip.h, lg_intersect / lg_occluded / lg_visibility / lg_open_directions / lg_range_scan / lg_radiance / lg_radiance_gather): rays are origin xyz, direction xyz
    std::vector<lg_hit> intersect(const std::vector<std::array<double, 6>> &rays) const {
        std::vector<lg_hit> hits(rays.size());
        if (lg_intersect(h_, rays.empty() ? nullptr : rays[0].data(), rays.size(), hits.data())) throw Error(lg_last_error());
        return hits;
    }
    std::vector<bool> occluded(const std::vector<std::array<double, 6>> &rays) const {
        std::vector<uint8_t> occ(rays.size());
        if (lg_occluded(h_, rays.empty() ? nullptr : rays[0].data(), rays.size(), occ.data())) throw Error(lg_last_error());
        return std::vector<bool>(occ.begin(), occ.end());
    }
    // visibility matrix (lg_visibility): bit j of row i -- (bits[i * row_bytes + (j >> 3)] >> (j & 7)) & 1, row_bytes = ceil(to.size() / 8) --
    // is 1 iff the segment from[i] -> to[j] is blocked; *blocked (if asked for): the number of set bits of every row
    std::vector<uint8_t> visibility(const std::vector<std::array<double, 3>> &from, const std::vector<std::array<double, 3>> &to,
                                    std::vector<uint32_t> *blocked = nullptr) const {
        const size_t row_bytes = (to.size() + 7) / 8;
        std::vector<uint8_t> bits(from.size() * row_bytes);
        if (blocked) blocked->assign(from.size(), 0u);
        if (lg_visibility(h_, from.empty() ? nullptr : from[0].data(), from.size(), to.empty() ? nullptr : to[0].data(), to.size(),
                          bits.empty() ? nullptr : bits.data(), row_bytes, blocked && !blocked->empty() ? blocked->data() : nullptr))
            throw Error(lg_last_error());
        return bits;
    }
    // direction set (lg_open_directions): bit k of row i -- (bits[i * row_bytes + (k >> 3)] >> (k & 7)) & 1, row_bytes = ceil(dirs.size() / 8) --
    // is 1 iff dirs[k] is above the horizon of points[i] ((n.x*d.x + n.y*d.y) + n.z*d.z > 0.0; every direction without normals) and the ray
    // (points[i], dirs[k]) is not occluded; *open / *above (if asked for): the numbers of open directions and of directions above per point
    std::vector<uint8_t> open_directions(const std::vector<std::array<double, 3>> &points, const std::vector<std::array<double, 3>> &dirs,
                                         const std::vector<std::array<double, 3>> *normals = nullptr, std::vector<uint32_t> *open = nullptr,
                                         std::vector<uint32_t> *above = nullptr) const {
        if (normals && normals->size() != points.size()) throw Error("open_directions: one normal per point");
        const size_t row_bytes = (dirs.size() + 7) / 8;
        std::vector<uint8_t> bits(points.size() * row_bytes);
        if (open) open->assign(points.size(), 0u);
        if (above) above->assign(points.size(), 0u);
        if (lg_open_directions(h_, points.empty() ? nullptr : points[0].data(), normals && !normals->empty() ? (*normals)[0].data() : nullptr, points.size(),
                               dirs.empty() ? nullptr : dirs[0].data(), dirs.size(), bits.empty() ? nullptr : bits.data(), row_bytes,
                               open && !open->empty() ? open->data() : nullptr, above && !above->empty() ? above->data() : nullptr))
            throw Error(lg_last_error());
        return bits;
    }
    // range scan (lg_range_scan): the first hits along beams[k] from origins[i], ray (i, k) at i * beams.size() + k of every plane asked for
    // (a null member is not asked for; not all six).  frames: one row-major 3 x 3 matrix per pose whose columns are the sensor's axes in
    // world space -- d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z --, or null: the beams are the directions, bit for bit.  range = the
    // hit's t (+inf: a miss); normal = the geometric normal faced toward the sensor; id = kind, prim, instance, material; hits[i] = the
    // beams of pose i that hit; nearest[i] = its smallest non-negative finite range (+inf: none).  lanes: 0 auto, 1 beam lanes, 2 pose lanes
    struct Scan {
        std::vector<float> *range = nullptr;                  // [poses*beams]
        std::vector<std::array<float, 3>> *point = nullptr;
        std::vector<std::array<float, 3>> *normal = nullptr;
        std::vector<std::array<uint32_t, 4>> *id = nullptr;
        std::vector<uint32_t> *hits = nullptr;                // [poses]
        std::vector<float> *nearest = nullptr;
    };
    void range_scan(const std::vector<std::array<double, 3>> &origins, const std::vector<std::array<double, 3>> &beams, const Scan &out,
                    const std::vector<std::array<double, 9>> *frames = nullptr, int lanes = 0) const {
        static_assert(sizeof(lg_scan_out) == 48, "lg_scan_out: six pointers");
        if (frames && frames->size() != origins.size()) throw Error("range_scan: one frame per pose");
        const size_t n = origins.size() * beams.size();
        lg_scan_out o{};
        if (out.range) { out.range->assign(n, 0.0f); o.range = out.range->data(); }
        if (out.point) { out.point->assign(n, {0.0f, 0.0f, 0.0f}); o.point = n ? (*out.point)[0].data() : nullptr; }
        if (out.normal) { out.normal->assign(n, {0.0f, 0.0f, 0.0f}); o.normal = n ? (*out.normal)[0].data() : nullptr; }
        if (out.id) { out.id->assign(n, {0u, 0u, 0u, 0u}); o.id = n ? (*out.id)[0].data() : nullptr; }
        if (out.hits) { out.hits->assign(origins.size(), 0u); o.hits = out.hits->data(); }
        if (out.nearest) { out.nearest->assign(origins.size(), 0.0f); o.nearest = out.nearest->data(); }
        if (lg_range_scan(h_, origins.empty() ? nullptr : origins[0].data(), frames && !frames->empty() ? (*frames)[0].data() : nullptr, origins.size(),
                          beams.empty() ? nullptr : beams[0].data(), beams.size(), lanes, &o))
            throw Error(lg_last_error());
    }
    void range_scan_device(const double *dev_origins, const double *dev_frames, size_t n_poses, const double *dev_beams, size_t n_beams, int lanes,
                           const lg_scan_out &dev_out, void *hip_stream) const {
        if (lg_range_scan_device(h_, dev_origins, dev_frames, n_poses, dev_beams, n_beams, lanes, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // hit layers (lg_hit_layers): the first max_layers surfaces along each ray, layer j of ray i at j * rays.size() + i of every layer plane
    // asked for (a null member is not asked for; not all five).  Segment j + 1 starts at layer j's p - ng * 2^-36 and keeps the ray's
    // direction.  hits = lg_intersect's record of the segment (the miss record behind a ray's last layer); along = t_0 + .. + t_j (+inf
    // behind the last layer); id = kind, prim, instance, material; count[i] = the layers found (== max_layers: the ray may have been cut
    // short); inside[i] = t_1 + t_3 + ..: the length inside material of a ray that starts outside every closed solid
    struct Layers {
        std::vector<lg_hit> *hits = nullptr;                  // [max_layers*rays]
        std::vector<double> *along = nullptr;
        std::vector<std::array<uint32_t, 4>> *id = nullptr;
        std::vector<uint32_t> *count = nullptr;               // [rays]
        std::vector<double> *inside = nullptr;
    };
    void hit_layers(const std::vector<std::array<double, 6>> &rays, uint32_t max_layers, const Layers &out) const {
        static_assert(sizeof(lg_layers_out) == 40, "lg_layers_out: five pointers");
        if (max_layers && rays.size() > SIZE_MAX / max_layers) throw Error("hit_layers: rays.size() * max_layers does not fit size_t");
        const size_t n = rays.size() * max_layers;
        lg_layers_out o{};
        if (out.hits) { out.hits->assign(n, lg_hit{}); o.hits = out.hits->data(); }
        if (out.along) { out.along->assign(n, 0.0); o.along = out.along->data(); }
        if (out.id) { out.id->assign(n, {0u, 0u, 0u, 0u}); o.id = n ? (*out.id)[0].data() : nullptr; }
        if (out.count) { out.count->assign(rays.size(), 0u); o.count = out.count->data(); }
        if (out.inside) { out.inside->assign(rays.size(), 0.0); o.inside = out.inside->data(); }
        if (lg_hit_layers(h_, rays.empty() ? nullptr : rays[0].data(), rays.size(), max_layers, &o)) throw Error(lg_last_error());
    }
    void hit_layers_device(const double *dev_rays, size_t n, uint32_t max_layers, const lg_layers_out &dev_out, void *hip_stream) const {
        if (lg_hit_layers_device(h_, dev_rays, n, max_layers, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // light groups (lg_radiance_groups): radiance() split by subsets of the scene's lights, groups.size() planes from one chain of walks,
    // group-major: plane g of ray r at g * rays.size() + r.  Plane g is what radiance() returns on an accel rebuilt with the lights of
    // groups[g].lights alone (bit l: light l in add order) and, without LG_GROUP_AMBIENT in its flags, no ambient term -- bit for bit
    int light_count() const { return lg_accel_light_count(h_); }
    std::vector<std::array<double, 3>> radiance_groups(const std::vector<std::array<double, 6>> &rays, const std::vector<lg_light_group> &groups) const {
        static_assert(sizeof(lg_light_group) == 8, "lg_light_group: two 32-bit words");
        if (!groups.empty() && rays.size() > SIZE_MAX / groups.size()) throw Error("radiance_groups: rays.size() * groups.size() does not fit size_t");
        std::vector<std::array<double, 3>> out(rays.size() * groups.size());
        if (rays.empty()) return out;
        if (lg_radiance_groups(h_, rays[0].data(), rays.size(), groups.data(), groups.size(), out.empty() ? nullptr : out[0].data())) throw Error(lg_last_error());
        return out;
    }
    void radiance_groups_device(const double *dev_rays, size_t n, const std::vector<lg_light_group> &groups, double *dev_radiance, void *hip_stream) const {
        if (lg_radiance_groups_device(h_, dev_rays, n, groups.data(), groups.size(), dev_radiance, hip_stream)) throw Error(lg_last_error());
    }
    // ray paths (lg_trace_paths): every ray followed through up to max_bounces vertices, the rule per material the caller's (rules.size() ==
    // material_count(); path_rule() makes one).  Vertex j of ray i at j * rays.size() + i of every vertex plane asked for (a null member is
    // not asked for; not all nine): hits = lg_intersect's record of segment j (the miss record behind a path's last vertex), point = its p,
    // id = kind, prim, instance, material, along = the running sum of t (+inf behind the last vertex).  Per ray: count = the vertices found,
    // end = LG_PATH_END_*, gain = the product of the rules' gains, last = the ray a cut path resumes from (or the segment the path ended
    // on), medium = the final crossing parity.  normal: 0 lg_hit::ng, 1 lg_hit::ns; start_medium: bit 0 per ray, or null (all outside)
    struct Paths {
        std::vector<lg_hit> *hits = nullptr;                  // [max_bounces*rays]
        std::vector<std::array<double, 3>> *point = nullptr;
        std::vector<std::array<uint32_t, 4>> *id = nullptr;
        std::vector<double> *along = nullptr;
        std::vector<uint32_t> *count = nullptr;               // [rays]
        std::vector<uint32_t> *end = nullptr;
        std::vector<double> *gain = nullptr;
        std::vector<std::array<double, 6>> *last = nullptr;
        std::vector<uint32_t> *medium = nullptr;
    };
    static lg_path_rule path_rule(uint32_t action, double ior = 1.0, double gain = 1.0) { return lg_path_rule{action, 0u, ior, gain}; }
    void trace_paths(const std::vector<std::array<double, 6>> &rays, uint32_t max_bounces, const std::vector<lg_path_rule> &rules, const Paths &out, int normal = 0,
                     const std::vector<uint32_t> *start_medium = nullptr) const {
        static_assert(sizeof(lg_paths_out) == 72 && sizeof(lg_path_rule) == 24, "lg_paths_out: nine pointers; lg_path_rule: 24 bytes");
        if (max_bounces && rays.size() > SIZE_MAX / max_bounces) throw Error("trace_paths: rays.size() * max_bounces does not fit size_t");
        if (start_medium && start_medium->size() != rays.size()) throw Error("trace_paths: start_medium has one word per ray");
        const size_t n = rays.size() * max_bounces;
        lg_paths_out o{};
        if (out.hits) { out.hits->assign(n, lg_hit{}); o.hits = out.hits->data(); }
        if (out.point) { out.point->assign(n, {0.0, 0.0, 0.0}); o.point = n ? (*out.point)[0].data() : nullptr; }
        if (out.id) { out.id->assign(n, {0u, 0u, 0u, 0u}); o.id = n ? (*out.id)[0].data() : nullptr; }
        if (out.along) { out.along->assign(n, 0.0); o.along = out.along->data(); }
        if (out.count) { out.count->assign(rays.size(), 0u); o.count = out.count->data(); }
        if (out.end) { out.end->assign(rays.size(), 0u); o.end = out.end->data(); }
        if (out.gain) { out.gain->assign(rays.size(), 0.0); o.gain = out.gain->data(); }
        if (out.last) { out.last->assign(rays.size(), {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); o.last = rays.empty() ? nullptr : (*out.last)[0].data(); }
        if (out.medium) { out.medium->assign(rays.size(), 0u); o.medium = out.medium->data(); }
        if (lg_trace_paths(h_, rays.empty() ? nullptr : rays[0].data(), rays.size(), max_bounces, rules.data(), rules.size(), normal,
                           start_medium ? start_medium->data() : nullptr, &o))
            throw Error(lg_last_error());
    }
    void trace_paths_device(const double *dev_rays, size_t n, uint32_t max_bounces, const std::vector<lg_path_rule> &rules, int normal, const uint32_t *dev_start_medium,
                            const lg_paths_out &dev_out, void *hip_stream) const {
        if (lg_trace_paths_device(h_, dev_rays, n, max_bounces, rules.data(), rules.size(), normal, dev_start_medium, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // surface scatter (lg_scatter): one level of li()'s tree, opened -- row i of every plane asked for (a null member is not asked for; not
    // all seven) belongs to ray i: hits = lg_intersect's record, direct = the lights in order + ambient at a hit (the background li() returns
    // at a miss), flags = LG_SCATTER_HIT | LG_SCATTER_REFLECT | LG_SCATTER_REFRACT, reflect / refract = the specular children's rays,
    // reflect_weight = the reflected child's spectrum, refract_weight = spectrum[3], |wi . ns|, pdf; an absent child's elements are +0.0.
    // li() to a depth of the caller's is (direct + reflect_weight * L(reflect)) + ((spectrum * L(refract)) * cos) / pdf, level by level
    struct Scatter {
        std::vector<lg_hit> *hits = nullptr;                        // [rays]
        std::vector<std::array<double, 3>> *direct = nullptr;
        std::vector<uint32_t> *flags = nullptr;
        std::vector<std::array<double, 6>> *reflect = nullptr;
        std::vector<std::array<double, 3>> *reflect_weight = nullptr;
        std::vector<std::array<double, 6>> *refract = nullptr;
        std::vector<std::array<double, 5>> *refract_weight = nullptr;
    };
    void scatter(const std::vector<std::array<double, 6>> &rays, const Scatter &out) const {
        static_assert(sizeof(lg_scatter_out) == 56, "lg_scatter_out: seven pointers");
        const size_t n = rays.size();
        lg_scatter_out o{};
        if (out.hits) { out.hits->assign(n, lg_hit{}); o.hits = out.hits->data(); }
        if (out.direct) { out.direct->assign(n, {0.0, 0.0, 0.0}); o.direct = n ? (*out.direct)[0].data() : nullptr; }
        if (out.flags) { out.flags->assign(n, 0u); o.flags = out.flags->data(); }
        if (out.reflect) { out.reflect->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); o.reflect = n ? (*out.reflect)[0].data() : nullptr; }
        if (out.reflect_weight) { out.reflect_weight->assign(n, {0.0, 0.0, 0.0}); o.reflect_weight = n ? (*out.reflect_weight)[0].data() : nullptr; }
        if (out.refract) { out.refract->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); o.refract = n ? (*out.refract)[0].data() : nullptr; }
        if (out.refract_weight) { out.refract_weight->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0}); o.refract_weight = n ? (*out.refract_weight)[0].data() : nullptr; }
        if (lg_scatter(h_, rays.empty() ? nullptr : rays[0].data(), n, &o)) throw Error(lg_last_error());
    }
    void scatter_device(const double *dev_rays, size_t n, const lg_scatter_out &dev_out, void *hip_stream) const {
        if (lg_scatter_device(h_, dev_rays, n, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // hit attributes (lg_hit_attributes / lg_hit_attributes_of): where on its primitive each ray's hit lies and the frame it is shaded in --
    // row i of every plane asked for (a null member is not asked for; not all seven) belongs to ray i: hits = lg_intersect's record, flags =
    // LG_ATTR_*, bary = a triangle hit's barycentrics, uv = the surface parameter, local = the hit point in the primitive's own space, frame =
    // the BSDF's tangents ss, ts, dp = the world-space geometric dpdu, dpdv; a miss's rows are +0.0.  With `records` (one lg_hit per ray, of
    // which kind, prim and instance are read) nothing is walked: the named primitives are resolved, and `hits` must stay null
    struct Attributes {
        std::vector<lg_hit> *hits = nullptr;                        // [rays]
        std::vector<uint32_t> *flags = nullptr;
        std::vector<std::array<double, 3>> *bary = nullptr;
        std::vector<std::array<double, 2>> *uv = nullptr;
        std::vector<std::array<double, 3>> *local = nullptr;
        std::vector<std::array<double, 6>> *frame = nullptr;
        std::vector<std::array<double, 6>> *dp = nullptr;
    };
    void hit_attributes(const std::vector<std::array<double, 6>> &rays, const Attributes &out, const std::vector<lg_hit> *records = nullptr) const {
        static_assert(sizeof(lg_attr_out) == 56, "lg_attr_out: seven pointers");
        const size_t n = rays.size();
        if (records && records->size() != n) throw Error("hit_attributes: one record per ray");
        lg_attr_out o{};
        if (out.hits) { out.hits->assign(n, lg_hit{}); o.hits = out.hits->data(); }
        if (out.flags) { out.flags->assign(n, 0u); o.flags = out.flags->data(); }
        if (out.bary) { out.bary->assign(n, {0.0, 0.0, 0.0}); o.bary = n ? (*out.bary)[0].data() : nullptr; }
        if (out.uv) { out.uv->assign(n, {0.0, 0.0}); o.uv = n ? (*out.uv)[0].data() : nullptr; }
        if (out.local) { out.local->assign(n, {0.0, 0.0, 0.0}); o.local = n ? (*out.local)[0].data() : nullptr; }
        if (out.frame) { out.frame->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); o.frame = n ? (*out.frame)[0].data() : nullptr; }
        if (out.dp) { out.dp->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); o.dp = n ? (*out.dp)[0].data() : nullptr; }
        const double *r = rays.empty() ? nullptr : rays[0].data();
        if (records ? lg_hit_attributes_of(h_, r, records->data(), n, &o) : lg_hit_attributes(h_, r, n, &o)) throw Error(lg_last_error());
    }
    void hit_attributes_device(const double *dev_rays, size_t n, const lg_attr_out &dev_out, void *hip_stream, const lg_hit *dev_records = nullptr) const {
        if (dev_records ? lg_hit_attributes_of_device(h_, dev_rays, dev_records, n, &dev_out, hip_stream) : lg_hit_attributes_device(h_, dev_rays, n, &dev_out, hip_stream))
            throw Error(lg_last_error());
    }
    // closest points (lg_closest_points): for each point (world space) the nearest surface point of the scene -- row i of every plane asked
    // for (a null member is not asked for; not all three) belongs to point i: distance (+INF where no surface lies within `radius`), point =
    // the closest point in world space (+0.0 for a miss), id = kind, prim, instance, material as in lg_hit (0, ~0, ~0, -1 for a miss).  The
    // header's arithmetic over every primitive, bit for bit; a scene with a sphere under a non-uniform scale is refused (lg_scene_closest_gate)
    struct Closest {
        std::vector<double> *distance = nullptr;                    // [points]
        std::vector<std::array<double, 3>> *point = nullptr;
        std::vector<std::array<uint32_t, 4>> *id = nullptr;
    };
    void closest_points(const std::vector<std::array<double, 3>> &points, const Closest &out, double radius = INFINITY) const {
        static_assert(sizeof(lg_closest_out) == 24, "lg_closest_out: three pointers");
        const size_t n = points.size();
        lg_closest_out o{};
        if (out.distance) { out.distance->assign(n, INFINITY); o.distance = out.distance->data(); }
        if (out.point) { out.point->assign(n, {0.0, 0.0, 0.0}); o.point = n ? (*out.point)[0].data() : nullptr; }
        if (out.id) { out.id->assign(n, {0u, ~0u, ~0u, ~0u}); o.id = n ? (*out.id)[0].data() : nullptr; }
        if (lg_closest_points(h_, points.empty() ? nullptr : points[0].data(), n, radius, &o)) throw Error(lg_last_error());
    }
    void closest_points_device(const double *dev_points, size_t n, double radius, const lg_closest_out &dev_out, void *hip_stream) const {
        if (lg_closest_points_device(h_, dev_points, n, radius, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // proximity queries (lg_nearest): for each point (world space), under radii[i] (`radii` null: the shared `radius`), the k nearest
    // primitives in ascending (squared distance, key) order, slot-major -- element (j, i) at j * points + i --, the count of ALL primitives
    // within the radius and whether any is.  A null member is not asked for; not all five.  touch alone leaves at the first contact; count
    // has to meet every primitive within the radius.  One candidate per primitive, closest_points' own: slot 0 is its answer
    struct Nearest {
        std::vector<uint8_t> *touch = nullptr;                      // [points]
        std::vector<uint32_t> *count = nullptr;                     // [points]
        std::vector<double> *distance = nullptr;                    // [k * points]
        std::vector<std::array<double, 3>> *point = nullptr;        // [k * points]
        std::vector<std::array<uint32_t, 4>> *id = nullptr;         // [k * points]
    };
    void nearest(const std::vector<std::array<double, 3>> &points, const std::vector<double> *radii, uint32_t k, const Nearest &out, double radius = INFINITY) const {
        static_assert(sizeof(lg_nearest_out) == 40, "lg_nearest_out: five pointers");
        const size_t n = points.size();
        if (radii && radii->size() != n) throw Error("nearest: one radius per point");
        if (k > LG_NEAREST_MAX_K) throw Error("nearest: k is beyond LG_NEAREST_MAX_K");
        const size_t nk = n * k;
        lg_nearest_out o{};
        if (out.touch) { out.touch->assign(n, 0); o.touch = out.touch->data(); }
        if (out.count) { out.count->assign(n, 0u); o.count = out.count->data(); }
        if (out.distance) { out.distance->assign(nk, INFINITY); o.distance = out.distance->data(); }
        if (out.point) { out.point->assign(nk, {0.0, 0.0, 0.0}); o.point = nk ? (*out.point)[0].data() : nullptr; }
        if (out.id) { out.id->assign(nk, {0u, ~0u, ~0u, ~0u}); o.id = nk ? (*out.id)[0].data() : nullptr; }
        if (lg_nearest(h_, points.empty() ? nullptr : points[0].data(), radii ? radii->data() : nullptr, n, radius, k, &o)) throw Error(lg_last_error());
    }
    void nearest_device(const double *dev_points, const double *dev_radii, size_t n, double radius, uint32_t k, const lg_nearest_out &dev_out, void *hip_stream) const {
        if (lg_nearest_device(h_, dev_points, dev_radii, n, radius, k, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // segment proximity (lg_closest_segments): for each segment p0 .. p1 (world space), under (*radii)[i] (null: the shared `radius`), the
    // nearest surface point of the scene to the segment, the segment's parameter there (its own closest point is p0 + (p1 - p0) * param),
    // the distance and the primitive: capsules and swept spheres against the world.  A null member is not asked for; not all five.  touch
    // alone leaves at the first contact.  A segment with p0 == p1 answers as nearest() does at k = 1
    struct Segments {
        std::vector<uint8_t> *touch = nullptr;                      // [segments]
        std::vector<double> *distance = nullptr;                    // [segments]
        std::vector<double> *param = nullptr;                       // [segments]
        std::vector<std::array<double, 3>> *point = nullptr;        // [segments], ON THE SURFACE
        std::vector<std::array<uint32_t, 4>> *id = nullptr;         // [segments]
    };
    void closest_segments(const std::vector<std::array<double, 6>> &segments, const std::vector<double> *radii, const Segments &out, double radius = INFINITY) const {
        static_assert(sizeof(lg_segments_out) == 40, "lg_segments_out: five pointers");
        const size_t n = segments.size();
        if (radii && radii->size() != n) throw Error("closest_segments: one radius per segment");
        lg_segments_out o{};
        if (out.touch) { out.touch->assign(n, 0); o.touch = out.touch->data(); }
        if (out.distance) { out.distance->assign(n, INFINITY); o.distance = out.distance->data(); }
        if (out.param) { out.param->assign(n, 0.0); o.param = out.param->data(); }
        if (out.point) { out.point->assign(n, {0.0, 0.0, 0.0}); o.point = n ? (*out.point)[0].data() : nullptr; }
        if (out.id) { out.id->assign(n, {0u, ~0u, ~0u, ~0u}); o.id = n ? (*out.id)[0].data() : nullptr; }
        if (lg_closest_segments(h_, segments.empty() ? nullptr : segments[0].data(), radii ? radii->data() : nullptr, n, radius, &o)) throw Error(lg_last_error());
    }
    void closest_segments_device(const double *dev_segments, const double *dev_radii, size_t n, double radius, const lg_segments_out &dev_out, void *hip_stream) const {
        if (lg_closest_segments_device(h_, dev_segments, dev_radii, n, radius, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // lit scatter (lg_scatter_lit): scatter() under lights that come with the call -- `lights` shared by every ray (per_ray false: K records)
    // or a table per ray (per_ray true: rays.size() * K records, ray i's at i * K), `ambient` in the scene's ambient colour's place; the
    // scene's own lights play no part.  Beside scatter()'s planes: terms = every light's own term of direct ([ray * K + k], +0.0 where it is
    // not added), visible = ceil(K / 32) words a ray, bit k & 31 of word k >> 5 set iff light k is visible from the hit
    struct ScatterLit {
        Scatter scatter;
        std::vector<std::array<double, 3>> *terms = nullptr;        // [rays * K]
        std::vector<uint32_t> *visible = nullptr;                   // [rays * ceil(K / 32)]
    };
    void scatter_lit(const std::vector<std::array<double, 6>> &rays, const std::vector<lg_light> &lights, bool per_ray, const std::array<double, 3> &ambient,
                     const ScatterLit &out) const {
        static_assert(sizeof(lg_light) == 72 && sizeof(lg_light_set) == 40 && sizeof(lg_lit_out) == 72, "lg_light, lg_light_set, lg_lit_out");
        const size_t n = rays.size();
        if (per_ray && n && lights.size() % n) throw Error("scatter_lit: a per-ray table holds rays.size() * K lights");
        const size_t K = per_ray ? (n ? lights.size() / n : 0) : lights.size(), W = (K + 31) / 32;
        if (K > LG_MAX_CALL_LIGHTS) throw Error("scatter_lit: at most LG_MAX_CALL_LIGHTS lights");
        const Scatter &sc = out.scatter;
        lg_lit_out o{};
        if (sc.hits) { sc.hits->assign(n, lg_hit{}); o.scatter.hits = sc.hits->data(); }
        if (sc.direct) { sc.direct->assign(n, {0.0, 0.0, 0.0}); o.scatter.direct = n ? (*sc.direct)[0].data() : nullptr; }
        if (sc.flags) { sc.flags->assign(n, 0u); o.scatter.flags = sc.flags->data(); }
        if (sc.reflect) { sc.reflect->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); o.scatter.reflect = n ? (*sc.reflect)[0].data() : nullptr; }
        if (sc.reflect_weight) { sc.reflect_weight->assign(n, {0.0, 0.0, 0.0}); o.scatter.reflect_weight = n ? (*sc.reflect_weight)[0].data() : nullptr; }
        if (sc.refract) { sc.refract->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); o.scatter.refract = n ? (*sc.refract)[0].data() : nullptr; }
        if (sc.refract_weight) { sc.refract_weight->assign(n, {0.0, 0.0, 0.0, 0.0, 0.0}); o.scatter.refract_weight = n ? (*sc.refract_weight)[0].data() : nullptr; }
        if (out.terms) { out.terms->assign(n * K, {0.0, 0.0, 0.0}); o.terms = n * K ? (*out.terms)[0].data() : nullptr; }
        if (out.visible) { out.visible->assign(n * W, 0u); o.visible = out.visible->data(); }
        const lg_light_set ls{lights.empty() ? nullptr : lights.data(), (uint32_t)K, per_ray ? 1u : 0u, {ambient[0], ambient[1], ambient[2]}};
        if (lg_scatter_lit(h_, rays.empty() ? nullptr : rays[0].data(), n, &ls, &o)) throw Error(lg_last_error());
    }
    // ... on device memory: dev_out's planes are device pointers; lights.lights is a HOST table when shared, device memory when per ray
    void scatter_lit_device(const double *dev_rays, size_t n, const lg_light_set &lights, const lg_lit_out &dev_out, void *hip_stream) const {
        if (lg_scatter_lit_device(h_, dev_rays, n, &lights, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // radiance along every ray (lg_radiance): li() as the render computes it, f64 RGB before quantisation
    std::vector<std::array<double, 3>> radiance(const std::vector<std::array<double, 6>> &rays) const {
        std::vector<std::array<double, 3>> out(rays.size());
        if (lg_radiance(h_, rays.empty() ? nullptr : rays[0].data(), rays.size(), out.empty() ? nullptr : out[0].data())) throw Error(lg_last_error());
        return out;
    }
    // radiance gather (lg_radiance_gather): li() along dirs[k] from origins[i], what radiance() returns for that ray, at i * dirs.size() + k of
    // *out.radiance, and / or reduced per pose into *out.sums: sums[i * n_weights + c] = the sum over k, in order from +0.0, of
    // radiance(i, k) * weights[k * n_weights + c] (one product, one sum a step).  A null member is not asked for; not both.  weights:
    // dirs.size() * n_weights doubles, k-major; looked at only with sums.  frames: one row-major 3 x 3 matrix per pose --
    // d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z --, or null: the directions are used bit for bit.  lanes: 0 auto, 1 direction lanes, 2 pose lanes
    struct Gather {
        std::vector<std::array<double, 3>> *radiance = nullptr;  // [poses*dirs]
        std::vector<std::array<double, 3>> *sums = nullptr;      // [poses*n_weights]
    };
    void radiance_gather(const std::vector<std::array<double, 3>> &origins, const std::vector<std::array<double, 3>> &dirs, const Gather &out,
                         const std::vector<double> *weights = nullptr, size_t n_weights = 0, const std::vector<std::array<double, 9>> *frames = nullptr,
                         int lanes = 0) const {
        static_assert(sizeof(lg_gather_out) == 16, "lg_gather_out: two pointers");
        if (frames && frames->size() != origins.size()) throw Error("radiance_gather: one frame per pose");
        if (out.sums && (!weights || weights->size() != dirs.size() * n_weights)) throw Error("radiance_gather: dirs.size() * n_weights weights");
        lg_gather_out o{};
        if (out.radiance) { out.radiance->assign(origins.size() * dirs.size(), {0.0, 0.0, 0.0}); o.radiance = out.radiance->empty() ? nullptr : (*out.radiance)[0].data(); }
        if (out.sums) { out.sums->assign(origins.size() * n_weights, {0.0, 0.0, 0.0}); o.sums = out.sums->empty() ? nullptr : (*out.sums)[0].data(); }
        if (lg_radiance_gather(h_, origins.empty() ? nullptr : origins[0].data(), frames && !frames->empty() ? (*frames)[0].data() : nullptr, origins.size(),
                               dirs.empty() ? nullptr : dirs[0].data(), dirs.size(), weights && !weights->empty() ? weights->data() : nullptr, n_weights, lanes, &o))
            throw Error(lg_last_error());
    }
    void radiance_gather_device(const double *dev_origins, const double *dev_frames, size_t n_poses, const double *dev_dirs, size_t n_dirs, const double *dev_weights,
                                size_t n_weights, int lanes, const lg_gather_out &dev_out, void *hip_stream) const {
        if (lg_radiance_gather_device(h_, dev_origins, dev_frames, n_poses, dev_dirs, n_dirs, dev_weights, n_weights, lanes, &dev_out, hip_stream)) throw Error(lg_last_error());
    }
    // a film from the caller's rays (lg_capture_rays): pixel slot g's rays are [g*samples, (g+1)*samples), summed in that order, scaled by
    // 1 / samples, quantised and written at film offset offsets[g] (y*width + x), or g without offsets; *rgb (if asked for): width*height
    // f64 RGB before quantisation, addressed like the film.  Pixels no slot names keep their bytes.
    void capture_rays(const std::vector<std::array<double, 6>> &rays, uint32_t samples, Film &film, const std::vector<uint64_t> *offsets = nullptr,
                      std::vector<std::array<double, 3>> *rgb = nullptr) const {
        if (samples == 0 || rays.size() % samples) throw Error("capture_rays: pixel slots * samples rays");
        const size_t slots = rays.size() / samples;
        if (offsets && offsets->size() != slots) throw Error("capture_rays: one offset per pixel slot");
        if (rgb) rgb->resize((size_t)film.w() * film.h());
        if (lg_capture_rays(h_, rays.empty() ? nullptr : rays[0].data(), slots, samples, offsets ? offsets->data() : nullptr, film.handle(),
                            rgb && !rgb->empty() ? (*rgb)[0].data() : nullptr, film.w(), film.h()))
            throw Error(lg_last_error());
    }
    // views (lg_view, lg_capture_views): this accel from K cameras into K width x height films in ONE call -- film v at rgba[v*width*height*4],
    // its f64 RGB before quantisation at (*rgb)[v*width*height]; the views share samples_root.  view(): the scene's own camera, whose film is
    // capture()'s; lg_view_look_at makes others (View::look_at below).
    lg_view view() const {
        lg_view v{};
        if (lg_accel_view(h_, &v)) throw Error(lg_last_error());
        return v;
    }
    std::vector<std::array<double, 6>> view_rays(const lg_view &v, uint32_t width, uint32_t height) const {
        static_assert(sizeof(lg_view) == 120, "lg_view: 15 doubles and two words, no padding");
        std::vector<std::array<double, 6>> out((size_t)width * height * v.samples_root * v.samples_root);
        if (lg_view_rays(h_, &v, width, height, 0, 0, width, height, out.empty() ? nullptr : out[0].data())) throw Error(lg_last_error());
        return out;
    }
    void view_rays_device(const lg_view &v, uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, double *dev_rays, void *hip_stream) const {
        if (lg_view_rays_device(h_, &v, width, height, x0, y0, x1, y1, dev_rays, hip_stream)) throw Error(lg_last_error());
    }
    void capture_views(const std::vector<lg_view> &views, uint32_t width, uint32_t height, std::vector<uint8_t> *rgba, std::vector<std::array<double, 3>> *rgb = nullptr) const {
        const size_t n = views.size() * (size_t)width * height;
        if (rgba) rgba->resize(n * 4);
        if (rgb) rgb->resize(n);
        if (lg_capture_views(h_, views.data(), views.size(), width, height, rgba && n ? rgba->data() : nullptr, rgb && n ? (*rgb)[0].data() : nullptr)) throw Error(lg_last_error());
    }
    // the same films enqueued into device memory on hip_stream (lg_capture_views_device); `views` stays a host array, copied before the call returns
    void capture_views_device(const std::vector<lg_view> &views, uint32_t width, uint32_t height, void *dev_rgba, double *dev_rgb, void *hip_stream) const {
        if (lg_capture_views_device(h_, views.data(), views.size(), width, height, dev_rgba, dev_rgb, hip_stream)) throw Error(lg_last_error());
    }
    // feature buffers of the scene's own camera view (lg_capture_features): first-hit depth, shading normal, albedo, coverage and ids of the
    // pixels [x0,x1) x [y0,y1) of a width x height film, every plane addressed like the film (pixel y*width + x) and sized here when it is
    // too small; pixels outside the rectangle keep what the vectors held.  A null vector pointer = that plane is not asked for.
    // material_rgb: material_count() colours, summed per hit material into albedo (required with it).
    struct Features {
        std::vector<float> *depth = nullptr;                  // [width*height]
        std::vector<std::array<float, 3>> *normal = nullptr;  // mean over all samples: premultiplied by coverage
        std::vector<std::array<float, 3>> *albedo = nullptr;
        std::vector<float> *coverage = nullptr;
        std::vector<std::array<uint32_t, 4>> *id = nullptr;   // sample 0's kind, prim, instance, material
    };
    size_t material_count() const { return lg_accel_material_count(h_); }
    void capture_features(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const Features &out,
                          const std::vector<std::array<double, 3>> *material_rgb = nullptr) const {
        const size_t n = (size_t)width * height;
        if (material_rgb && material_rgb->size() != material_count()) throw Error("capture_features: material_count() colours");
        auto sized = [n](auto *v) { if (v && v->size() < n) v->resize(n); return v && n ? &(*v)[0] : nullptr; };
        lg_features f{};
        f.depth = sized(out.depth); f.coverage = sized(out.coverage);
        if (auto *p = sized(out.normal)) f.normal = p->data();
        if (auto *p = sized(out.albedo)) f.albedo = p->data();
        if (auto *p = sized(out.id)) f.id = p->data();
        if (lg_capture_features(h_, width, height, x0, y0, x1, y1, &f, material_rgb && !material_rgb->empty() ? (*material_rgb)[0].data() : nullptr))
            throw Error(lg_last_error());
    }
    // the same planes enqueued into device memory on hip_stream (lg_capture_features_device): dev_out's members are device pointers
    void capture_features_device(uint32_t width, uint32_t height, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, const lg_features &dev_out,
                                 const double *dev_material_rgb, void *hip_stream) const {
        if (lg_capture_features_device(h_, width, height, x0, y0, x1, y1, &dev_out, dev_material_rgb, hip_stream)) throw Error(lg_last_error());
    }
    // view features (lg_capture_view_features): the same planes and the world-space hit point for K views in ONE call, K whole films -- the
    // element of (v, x, y) at v*width*height + y*width + x, every vector sized here to n_views*width*height.  A null vector pointer = that
    // plane is not asked for.  depth and point are means over the samples that hit (+inf and (0, 0, 0): none); the views share samples_root.
    struct ViewFeatures : Features {
        std::vector<std::array<float, 3>> *point = nullptr;   // reprojects a pixel of one view into another
    };
    void capture_view_features(const std::vector<lg_view> &views, uint32_t width, uint32_t height, const ViewFeatures &out,
                               const std::vector<std::array<double, 3>> *material_rgb = nullptr) const {
        static_assert(sizeof(lg_view_features) == 48, "lg_view_features: six pointers");
        const size_t n = views.size() * (size_t)width * height;
        if (material_rgb && material_rgb->size() != material_count()) throw Error("capture_view_features: material_count() colours");
        auto sized = [n](auto *v) { if (v) v->resize(n); return v && n ? &(*v)[0] : nullptr; };
        lg_view_features f{};
        f.depth = sized(out.depth); f.coverage = sized(out.coverage);
        if (auto *p = sized(out.normal)) f.normal = p->data();
        if (auto *p = sized(out.albedo)) f.albedo = p->data();
        if (auto *p = sized(out.id)) f.id = p->data();
        if (auto *p = sized(out.point)) f.point = p->data();
        if (lg_capture_view_features(h_, views.data(), views.size(), width, height, &f, material_rgb && !material_rgb->empty() ? (*material_rgb)[0].data() : nullptr))
            throw Error(lg_last_error());
    }
    // the same planes enqueued into device memory on hip_stream (lg_capture_view_features_device): dev_out's members are device pointers;
    // `views` stays a host array, copied before the call returns
    void capture_view_features_device(const std::vector<lg_view> &views, uint32_t width, uint32_t height, const lg_view_features &dev_out,
                                      const double *dev_material_rgb, void *hip_stream) const {
        if (lg_capture_view_features_device(h_, views.data(), views.size(), width, height, &dev_out, dev_material_rgb, hip_stream)) throw Error(lg_last_error());
    }
    // the order a query's rays are walked in (lg_accel_set_query_order): 0 as given (default), 1 sorted on the device by a coherence key
    void set_query_order(int order) const {
        if (lg_accel_set_query_order(h_, order)) throw Error(lg_last_error());
    }
    int query_order() const { return lg_accel_get_query_order(h_); }
    // the order mode 1 walks `rays` in: perm[s] = the ray walked in slot s, the stable ascending sort of the rays' keys (*keys, if asked for)
    std::vector<uint32_t> query_order(const std::vector<std::array<double, 6>> &rays, std::vector<uint32_t> *keys = nullptr) const {
        std::vector<uint32_t> perm(rays.size());
        if (keys) keys->assign(rays.size(), 0u);
        if (lg_query_order(h_, rays.empty() ? nullptr : rays[0].data(), rays.size(), perm.data(), keys ? keys->data() : nullptr)) throw Error(lg_last_error());
        return perm;
    }

  private:
    explicit Accel(lg_accel *a) : h_(a) {}
    lg_accel *h_;
};

// A view for Accel::capture_views from a look-at camera (lg_view_look_at): what a scene's own camera holds after set_perspective_camera(fov) /
// set_orthographic_camera(scale), look_at and set_supersampling, byte for byte
struct View {
    static lg_view look_at(bool perspective, double param, Vec3 origin, Vec3 look, Vec3 up, uint8_t supersampling = 0) {
        lg_view v{};
        const double o[3] = {origin[0], origin[1], origin[2]}, l[3] = {look[0], look[1], look[2]}, u[3] = {up[0], up[1], up[2]};
        if (lg_view_look_at(&v, perspective ? 1 : 0, param, o, l, u, supersampling)) throw Error(lg_last_error());
        return v;
    }
    static lg_view of(const Scene &scene) {
        lg_view v{};
        if (lg_scene_view(scene.handle(), &v)) throw Error(lg_last_error());
        return v;
    }
};

// A lens camera the reference does not have (lg_lens, lg_lens_rays): an equirectangular panorama (kind 0) or an equidistant fisheye (kind 1)
// around `origin`, its basis used as given.  rays(): width*height*samples_root^2 rays in the layout Accel::capture_rays takes, row-major
// pixels -- or the pixel slots `offsets` names.
struct Lens {
    lg_lens c{};
    Lens(int kind, Vec3 origin, Vec3 right, Vec3 up, Vec3 forward, double fov_deg = 180.0) {
        c.kind = kind;
        for (int i = 0; i < 3; ++i) { c.origin[i] = origin[i]; c.right[i] = right[i]; c.up[i] = up[i]; c.forward[i] = forward[i]; }
        c.fov_deg = fov_deg;
    }
    std::vector<std::array<double, 6>> rays(uint32_t width, uint32_t height, uint32_t samples_root = 1, const std::vector<uint64_t> *offsets = nullptr) const {
        const size_t slots = offsets ? offsets->size() : (size_t)width * height;
        std::vector<std::array<double, 6>> out(slots * samples_root * samples_root);
        if (lg_lens_rays(&c, width, height, samples_root, offsets ? offsets->data() : nullptr, slots, out.empty() ? nullptr : out[0].data())) throw Error(lg_last_error());
        return out;
    }
};

// GPU-side counterpart of `scene.threads`: the devices capture() / render() split a host film over
// (empty = every visible device); see lg_set_devices.
inline void set_devices(const std::vector<int> &ids = {}) {
    if (lg_set_devices(ids.data(), (int)ids.size())) throw Error(lg_last_error());
}
inline void capture(const Scene &scene, Film &film) { // lib.rs:55
    if (lg_capture(scene.handle(), film.handle())) throw Error(lg_last_error());
}
inline void capture_subset(size_t k, size_t n, const Accel &root, Film &film) { // lib.rs:110
    if (lg_capture_subset(k, n, root.handle(), film.handle())) throw Error(lg_last_error());
}
// several subsets of one n as ONE render: the pixels of the calls capture_subset(k, n, ...) for k in ks (lasgun_hip.h, lg_capture_subsets)
inline void capture_subsets(const std::vector<size_t> &ks, size_t n, const Accel &root, Film &film) {
    if (lg_capture_subsets(ks.data(), ks.size(), n, root.handle(), film.handle())) throw Error(lg_last_error());
}
// the table of measured kernel-organisation choices (lasgun_hip.h, lg_tune_*): export it once, import it at start-up, and no launch of a known kind is measured again
inline std::vector<lg_tune_entry> tune_export() {
    std::vector<lg_tune_entry> v(lg_tune_export(nullptr, 0));
    v.resize(std::min(v.size(), lg_tune_export(v.data(), v.size())));
    return v;
}
inline void tune_import(const std::vector<lg_tune_entry> &entries) {
    if (lg_tune_import(entries.data(), entries.size())) throw Error(lg_last_error());
}
inline void tune_clear() { lg_tune_clear(); }
inline Film render(const Scene &scene, std::pair<uint32_t, uint32_t> resolution) { // lib.rs:46
    lg_film *f = lg_render(scene.handle(), resolution.first, resolution.second);
    if (!f) throw Error(lg_last_error());
    return Film(f);
}

} // namespace lasgun
