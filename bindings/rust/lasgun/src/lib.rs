//! `lasgun` over liblasgun_hip.so -- the reference's public surface for the render path, same names, same argument
//! meaning, rendering on an MI355X through the C ABI of include/lasgun_hip.h (crate `lasgun-hip-sys`).
//!
//! What is mirrored (file:line under nfrasser/lasgun):
//!   `Accel`, `render`, `capture`, `capture_subset`          src/lib.rs:42-56,110
//!   `scene::Scene`, `scene::ObjRef`                          src/scene.rs:11-143
//!   `scene::Aggregate`                                       src/scene/node.rs:25-115
//!   `Material`                                               src/material/mod.rs:3-46
//!   `Camera`                                                 src/camera.rs:75-102
//!   `Film`, `Img`, `Pixel`, `PixelBuffer`                    src/film.rs:7-45, src/img.rs:9-52
//!   `output::render`                                         src/output.rs:5-18 (PNG written by a small built-in encoder)
//!
//! Differences a port has to know about:
//!   * there is no CPU path: every render call needs a HIP device and panics with the library's message otherwise
//!     (the reference panics on a failed thread join, a missing mesh, a BVH deeper than 64, an empty aggregate);
//!   * `scene.camera` is reached through the `&mut Camera` the `set_*_camera` calls return, as in every example;
//!   * `scene.threads` caps the number of GPUs a `capture` is split over (`set_devices`), not CPU threads.
use std::ffi::{CStr, CString};
use std::marker::PhantomData;
use std::ops::{Index, IndexMut};
use std::path::Path;

use lasgun_hip_sys as sys;

fn last_error() -> String {
    unsafe { CStr::from_ptr(sys::lg_last_error()).to_string_lossy().into_owned() }
}

// ---------------------------------------------------------------------------------------------------------------
// Material (src/material/mod.rs:3-46): a Copy value
// ---------------------------------------------------------------------------------------------------------------
#[derive(Clone, Copy, Debug)]
pub struct Material(sys::lg_material);

impl Material {
    /// Default material for cases where a specific one may not be required (material/mod.rs:15)
    pub fn default() -> Material { Material(unsafe { sys::lg_material_default() }) }
    pub fn matte(kd: [f64; 3], sigma: f64) -> Material { Material(unsafe { sys::lg_material_matte(&kd, sigma) }) }
    pub fn plastic(kd: [f64; 3], ks: [f64; 3], roughness: f64) -> Material { Material(unsafe { sys::lg_material_plastic(&kd, &ks, roughness) }) }
    pub fn metal(eta: [f64; 3], k: [f64; 3], u_roughness: f64, v_roughness: f64) -> Material {
        Material(unsafe { sys::lg_material_metal(&eta, &k, u_roughness, v_roughness) })
    }
    pub fn glass(kr: [f64; 3], kt: [f64; 3], eta: f64) -> Material { Material(unsafe { sys::lg_material_glass(&kr, &kt, eta) }) }
    pub fn mirror(kr: [f64; 3]) -> Material { Material(unsafe { sys::lg_material_mirror(&kr) }) }
}

// ---------------------------------------------------------------------------------------------------------------
// Camera (src/camera.rs:75-102): lives in the scene; the setters take effect there
// ---------------------------------------------------------------------------------------------------------------
pub struct Camera {
    scene: *mut sys::lg_scene,
}

impl Camera {
    pub fn look_at(&mut self, origin: [f64; 3], look: [f64; 3], up: [f64; 3]) { unsafe { sys::lg_camera_look_at(self.scene, &origin, &look, &up) } }
    pub fn set_supersampling(&mut self, base: u8) { unsafe { sys::lg_camera_set_supersampling(self.scene, base) } }
    pub fn set_aperture_radius(&mut self, radius: f64) { unsafe { sys::lg_camera_set_aperture_radius(self.scene, radius) } }
}

// ---------------------------------------------------------------------------------------------------------------
// scene::{Scene, Aggregate, ObjRef} (src/scene.rs, src/scene/node.rs)
// ---------------------------------------------------------------------------------------------------------------
pub mod scene {
    use super::*;

    /// Opaque reference to a .obj-powered mesh in a scene (scene.rs:42-44)
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub struct ObjRef(pub(crate) u32);

    /// The one `Result` on the reference's path (obj::ObjError, scene.rs:120-130)
    #[derive(Debug)]
    pub struct ObjError(pub String);
    impl std::fmt::Display for ObjError {
        fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result { write!(f, "{}", self.0) }
    }
    impl std::error::Error for ObjError {}

    /// A collection of scene nodes under one transformation (node.rs:25-33).  Owned until it is moved into a scene
    /// or a parent group; `scene.root` is a borrowed view of the scene's own root.
    pub struct Aggregate {
        pub(crate) ptr: *mut sys::lg_aggregate,
        owned: bool,
    }

    impl Aggregate {
        pub fn new() -> Aggregate { Aggregate { ptr: unsafe { sys::lg_aggregate_new() }, owned: true } }
        pub(crate) fn borrowed(ptr: *mut sys::lg_aggregate) -> Aggregate { Aggregate { ptr, owned: false } }
        fn into_raw(mut self) -> *mut sys::lg_aggregate {
            assert!(self.owned, "the scene's root aggregate cannot be moved");
            self.owned = false; // ownership goes to the C side
            self.ptr
        }

        pub fn add_group(&mut self, aggregate: Aggregate) { unsafe { sys::lg_aggregate_add_group(self.ptr, aggregate.into_raw()) } }
        pub fn add_sphere(&mut self, center: [f64; 3], radius: f64, material: Material) { unsafe { sys::lg_aggregate_add_sphere(self.ptr, &center, radius, &material.0) } }
        pub fn add_cube(&mut self, origin: [f64; 3], dim: f64, material: Material) { unsafe { sys::lg_aggregate_add_cube(self.ptr, &origin, dim, &material.0) } }
        pub fn add_box(&mut self, minbound: [f64; 3], maxbound: [f64; 3], material: Material) { unsafe { sys::lg_aggregate_add_box(self.ptr, &minbound, &maxbound, &material.0) } }
        /// Add a mesh that provides its own material properties (or defaults to Material::default())
        pub fn add_obj(&mut self, mesh: ObjRef) { unsafe { sys::lg_aggregate_add_obj(self.ptr, mesh.0) } }
        /// Add a mesh that is made of a single material
        pub fn add_obj_of(&mut self, mesh: ObjRef, material: Material) { unsafe { sys::lg_aggregate_add_obj_of(self.ptr, mesh.0, &material.0) } }
        pub fn swap_backface(&mut self) { unsafe { sys::lg_aggregate_swap_backface(self.ptr) } }
        pub fn translate(&mut self, delta: [f64; 3]) -> &mut Self { unsafe { sys::lg_aggregate_translate(self.ptr, &delta) }; self }
        pub fn scale(&mut self, x: f64, y: f64, z: f64) -> &mut Self { unsafe { sys::lg_aggregate_scale(self.ptr, x, y, z) }; self }
        pub fn rotate_x(&mut self, theta: f64) -> &mut Self { unsafe { sys::lg_aggregate_rotate_x(self.ptr, theta) }; self }
        pub fn rotate_y(&mut self, theta: f64) -> &mut Self { unsafe { sys::lg_aggregate_rotate_y(self.ptr, theta) }; self }
        pub fn rotate_z(&mut self, theta: f64) -> &mut Self { unsafe { sys::lg_aggregate_rotate_z(self.ptr, theta) }; self }
        pub fn rotate(&mut self, theta: f64, axis: [f64; 3]) -> &mut Self { unsafe { sys::lg_aggregate_rotate(self.ptr, theta, &axis) }; self }
    }

    impl Drop for Aggregate {
        fn drop(&mut self) {
            if self.owned { unsafe { sys::lg_aggregate_free(self.ptr) } }
        }
    }

    /// Description of the world to render and how it should be rendered (scene.rs:11-40)
    pub struct Scene {
        pub(crate) ptr: *mut sys::lg_scene,
        /// The root node: `scene.root.add_sphere(..)` as in the reference's examples (scene.rs:14)
        pub root: Aggregate,
        camera: Camera,
    }

    impl Scene {
        pub fn new() -> Scene {
            let ptr = unsafe { sys::lg_scene_new() };
            Scene { ptr, root: Aggregate::borrowed(unsafe { sys::lg_scene_root(ptr) }), camera: Camera { scene: ptr } }
        }
        pub fn set_perspective_camera(&mut self, fov: f64) -> &mut Camera { unsafe { sys::lg_scene_set_perspective_camera(self.ptr, fov) }; &mut self.camera }
        pub fn set_orthographic_camera(&mut self, scale: f64) -> &mut Camera { unsafe { sys::lg_scene_set_orthographic_camera(self.ptr, scale) }; &mut self.camera }
        pub fn set_solid_background(&mut self, color: [f64; 3]) { unsafe { sys::lg_scene_set_solid_background(self.ptr, &color) } }
        pub fn set_radial_background(&mut self, inner: [f64; 3], outer: [f64; 3], scale: f64) { unsafe { sys::lg_scene_set_radial_background(self.ptr, &inner, &outer, scale) } }
        pub fn set_ambient_light(&mut self, color: [f64; 3]) { unsafe { sys::lg_scene_set_ambient_light(self.ptr, &color) } }
        pub fn set_mesh_smoothing(&mut self, enabled: bool) { unsafe { sys::lg_scene_set_mesh_smoothing(self.ptr, enabled as i32) } }
        pub fn set_max_recursion_depth(&mut self, max_depth: u32) { unsafe { sys::lg_scene_set_max_recursion_depth(self.ptr, max_depth) } }
        /// Zero: every GPU selected with `set_devices`; otherwise a cap on how many of them a capture is split over
        pub fn set_threads(&mut self, threads: usize) { unsafe { sys::lg_scene_set_threads(self.ptr, threads) } }
        pub fn add_point_light(&mut self, position: [f64; 3], intensity: [f64; 3], falloff: [f64; 3]) {
            unsafe { sys::lg_scene_add_point_light(self.ptr, &position, &intensity, &falloff) }
        }
        /// Triangle mesh from the string contents of a .obj file (scene.rs:120-123)
        pub fn parse_obj(&mut self, obj: &str) -> Result<ObjRef, ObjError> {
            let mut reference = 0u32;
            let rc = unsafe { sys::lg_scene_parse_obj(self.ptr, obj.as_ptr() as *const _, obj.len(), &mut reference) };
            if rc != 0 { Err(ObjError(last_error())) } else { Ok(ObjRef(reference)) }
        }
        /// Load the .obj file at the given path (scene.rs:127-130)
        pub fn load_obj(&mut self, obj_path: &Path) -> Result<ObjRef, ObjError> {
            let c = CString::new(obj_path.to_string_lossy().as_bytes()).map_err(|e| ObjError(e.to_string()))?;
            let mut reference = 0u32;
            let rc = unsafe { sys::lg_scene_load_obj(self.ptr, c.as_ptr(), &mut reference) };
            if rc != 0 { Err(ObjError(last_error())) } else { Ok(ObjRef(reference)) }
        }
        pub fn set_root(&mut self, node: Aggregate) {
            unsafe { sys::lg_scene_set_root(self.ptr, node.into_raw()) };
            self.root = Aggregate::borrowed(unsafe { sys::lg_scene_root(self.ptr) });
        }
    }

    impl Drop for Scene {
        fn drop(&mut self) { unsafe { sys::lg_scene_free(self.ptr) } }
    }
}

pub use crate::scene::Scene;

// ---------------------------------------------------------------------------------------------------------------
// Img / Film (src/img.rs:9-67, src/film.rs:7-45)
// ---------------------------------------------------------------------------------------------------------------
pub type Pixel = [u8; 4];

/// Store of pixels in row-major order that can be saved somewhere (img.rs:9-13)
pub trait PixelBuffer: Index<usize, Output = Pixel> + IndexMut<usize> {
    fn save(&self, filename: &str);
}
impl PixelBuffer for Vec<Pixel> {
    fn save(&self, _filename: &str) {}
}

/// What `capture_subset` writes to (img.rs:16-52)
pub trait Img {
    fn w(&self) -> u32;
    fn h(&self) -> u32;
    fn set(&mut self, x: u32, y: u32, color: &Pixel);
}

pub struct Film {
    pub w: u32,
    pub h: u32,
    pub winv: f64,
    pub hinv: f64,
    pub aspect: f64,
    output: Box<dyn PixelBuffer<Output = Pixel>>,
}

impl Film {
    /// A film of the given dimensions, every pixel black and transparent (film.rs:24)
    pub fn new(width: u32, height: u32) -> Film {
        let area = (width as usize) * (height as usize);
        Film::new_with_output(width, height, Box::new(vec![[0u8, 0, 0, 0]; area]))
    }
    /// A film over a pre-allocated pixel store of width * height pixels (film.rs:36)
    pub fn new_with_output(width: u32, height: u32, output: Box<dyn PixelBuffer<Output = Pixel>>) -> Film {
        Film { w: width, h: height, winv: 1. / width as f64, hinv: 1. / height as f64, aspect: width as f64 / height as f64, output }
    }
    pub fn save(&self, filename: &str) { self.output.save(filename) }
}
impl Index<usize> for Film {
    type Output = Pixel;
    fn index(&self, at: usize) -> &Pixel { &self.output[at] }
}
impl IndexMut<usize> for Film {
    fn index_mut(&mut self, at: usize) -> &mut Pixel { &mut self.output[at] }
}
impl Img for Film {
    fn w(&self) -> u32 { self.w }
    fn h(&self) -> u32 { self.h }
    fn set(&mut self, x: u32, y: u32, color: &Pixel) {
        let at = (y as usize) * (self.w as usize) + x as usize;
        self.output[at] = *color
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Lens cameras (no counterpart in the reference): rays for `Accel::capture_rays`
// ---------------------------------------------------------------------------------------------------------------
/// An equirectangular panorama (kind 0) or an equidistant fisheye (kind 1; `fov_deg` across the film's shorter side) around `origin`;
/// the basis is used as given.
pub use sys::lg_lens as Lens;
pub use sys::lg_features as Features;
pub use sys::lg_scan_out as ScanOut;
/// The work item a range scan of these counts would use (`lg_range_scan_lanes`): 1 beam lanes, 2 pose lanes; `lanes` 0 asks for the
/// stated default (pose lanes iff n_poses >= n_beams); -1 for a bad `lanes`.  No device is touched.
pub fn range_scan_lanes(n_poses: usize, n_beams: usize, lanes: i32) -> i32 { unsafe { sys::lg_range_scan_lanes(n_poses, n_beams, lanes) } }
pub use sys::lg_layers_out as LayersOut;
/// One rule of `Accel::trace_paths` (`lg_path_rule`, 24 bytes), indexed by a hit's material; `action` is one of `sys::LG_PATH_*`.
pub use sys::lg_path_rule as PathRule;
pub use sys::lg_paths_out as PathsOut;
/// The planes `Accel::trace_paths` fills: `None` = not asked for; not all nine.
#[derive(Default)]
pub struct Paths<'a> {
    pub hits: Option<&'a mut [sys::lg_hit]>,
    pub point: Option<&'a mut [[f64; 3]]>,
    pub id: Option<&'a mut [[u32; 4]]>,
    pub along: Option<&'a mut [f64]>,
    pub count: Option<&'a mut [u32]>,
    pub end: Option<&'a mut [u32]>,
    pub gain: Option<&'a mut [f64]>,
    pub last: Option<&'a mut [[f64; 6]]>,
    pub medium: Option<&'a mut [u32]>,
}
pub use sys::lg_scatter_out as ScatterOut;
/// The planes `Accel::scatter` fills, one row per ray: `None` = not asked for; not all seven.
#[derive(Default)]
pub struct Scatter<'a> {
    pub hits: Option<&'a mut [sys::lg_hit]>,
    pub direct: Option<&'a mut [[f64; 3]]>,
    pub flags: Option<&'a mut [u32]>,
    pub reflect: Option<&'a mut [[f64; 6]]>,
    pub reflect_weight: Option<&'a mut [[f64; 3]]>,
    pub refract: Option<&'a mut [[f64; 6]]>,
    pub refract_weight: Option<&'a mut [[f64; 5]]>,
}
pub use sys::lg_attr_out as AttrOut;
/// The planes `Accel::hit_attributes` / `hit_attributes_of` fill, one row per ray: `None` = not asked for; not all seven (`hits` stays
/// `None` for `hit_attributes_of`).
#[derive(Default)]
pub struct Attributes<'a> {
    pub hits: Option<&'a mut [sys::lg_hit]>,
    pub flags: Option<&'a mut [u32]>,
    pub bary: Option<&'a mut [[f64; 3]]>,
    pub uv: Option<&'a mut [[f64; 2]]>,
    pub local: Option<&'a mut [[f64; 3]]>,
    pub frame: Option<&'a mut [[f64; 6]]>,
    pub dp: Option<&'a mut [[f64; 6]]>,
}
pub use sys::lg_closest_out as ClosestOut;
/// The planes `Accel::closest_points` fills, one row per point: `None` = not asked for; not all three.  (Like the rest of this crate:
/// uncompiled here -- no Rust toolchain --, held to the C header textually by tests/test_rust_bindings.py and tests/test_closest_points_abi.py.)
#[derive(Default)]
pub struct Closest<'a> {
    pub distance: Option<&'a mut [f64]>,
    pub point: Option<&'a mut [[f64; 3]]>,
    pub id: Option<&'a mut [[u32; 4]]>,
}
pub use sys::lg_nearest_out as NearestOut;
/// The planes `Accel::nearest` fills: `touch` and `count` one row per point, `distance` / `point` / `id` slot-major (k * points rows, slot j
/// of point i at j * points + i); `None` = not asked for; not all five.  (Like the rest of this crate: uncompiled here -- no Rust toolchain --,
/// held to the C header textually by tests/test_rust_bindings.py and tests/test_nearest_abi.py.)
#[derive(Default)]
pub struct Nearest<'a> {
    pub touch: Option<&'a mut [u8]>,
    pub count: Option<&'a mut [u32]>,
    pub distance: Option<&'a mut [f64]>,
    pub point: Option<&'a mut [[f64; 3]]>,
    pub id: Option<&'a mut [[u32; 4]]>,
}
pub use sys::lg_segments_out as SegmentsOut;
/// The planes `Accel::closest_segments` fills, one row per segment: `touch`, `distance`, `param` (s in [0, 1]: the segment's own closest
/// point is p0 + (p1 - p0) * s), `point` (ON THE SURFACE) and `id`; `None` = not asked for; not all five.  (Like the rest of this crate:
/// uncompiled here -- no Rust toolchain --, held to the C header textually by tests/test_rust_bindings.py and tests/test_closest_segments_abi.py.)
#[derive(Default)]
pub struct Segments<'a> {
    pub touch: Option<&'a mut [u8]>,
    pub distance: Option<&'a mut [f64]>,
    pub param: Option<&'a mut [f64]>,
    pub point: Option<&'a mut [[f64; 3]]>,
    pub id: Option<&'a mut [[u32; 4]]>,
}
pub use sys::lg_light as Light;
pub use sys::lg_light_set as LightSet;
pub use sys::lg_lit_out as LitOut;
/// The planes `Accel::scatter_lit` fills: `scatter`'s seven, `terms` (rays * K rows) and `visible` (rays * ceil(K / 32) words); not all nine `None`.
#[derive(Default)]
pub struct ScatterLit<'a> {
    pub scatter: Scatter<'a>,
    pub terms: Option<&'a mut [[f64; 3]]>,
    pub visible: Option<&'a mut [u32]>,
}
pub use sys::lg_gather_out as GatherOut;
/// The work item a radiance gather of these counts would use (`lg_radiance_gather_lanes`): 1 direction lanes, 2 pose lanes; `lanes` 0 asks
/// for the stated default (pose lanes iff n_poses >= n_dirs); -1 for a bad `lanes`.  No device is touched.
pub fn radiance_gather_lanes(n_poses: usize, n_dirs: usize, lanes: i32) -> i32 { unsafe { sys::lg_radiance_gather_lanes(n_poses, n_dirs, lanes) } }
/// A camera as the kernels read it (`lg_view`, 120 bytes): what `Accel::capture_views` renders from.
pub use sys::lg_view as View;
/// The planes of `Accel::capture_view_features_device` (`lg_view_features`, 48 bytes): `Features`' five and the world-space hit point.
pub use sys::lg_view_features as ViewFeatures;
/// The view of a look-at camera (`lg_view_look_at`): what a scene's own camera holds after `set_perspective_camera(param)` (or
/// `set_orthographic_camera(param)` with `perspective` false), `look_at` and `set_supersampling`, byte for byte.  No device is touched.
pub fn view_look_at(perspective: bool, param: f64, origin: [f64; 3], look: [f64; 3], up: [f64; 3], supersampling: u8) -> View {
    const _: () = assert!(std::mem::size_of::<sys::lg_view>() == 120);
    let mut v: View = unsafe { std::mem::zeroed() };
    let rc = unsafe { sys::lg_view_look_at(&mut v, perspective as i32, param, &origin, &look, &up, supersampling) };
    if rc != 0 { panic!("lasgun: {}", last_error()) }
    v
}
/// The scene's own camera as a view (`lg_scene_view`).  No device is touched.
pub fn scene_view(scene: &Scene) -> View {
    let mut v: View = unsafe { std::mem::zeroed() };
    if unsafe { sys::lg_scene_view(scene.ptr, &mut v) } != 0 { panic!("lasgun: {}", last_error()) }
    v
}

/// The rays of a lens over a width x height film, row-major pixels (or over the pixel slots `offsets` names), samples_root^2 per slot in
/// idx = i*samples_root + j order: the layout `Accel::capture_rays` takes.  Generated on the current device.
pub fn lens_rays(lens: &Lens, width: u32, height: u32, samples_root: u32, offsets: Option<&[u64]>) -> Vec<[f64; 6]> {
    let slots = offsets.map_or((width as usize) * (height as usize), |o| o.len());
    let mut out = vec![[0f64; 6]; slots * (samples_root as usize) * (samples_root as usize)];
    if out.is_empty() { return out }
    let rc = unsafe { sys::lg_lens_rays(lens, width, height, samples_root, offsets.map_or(std::ptr::null(), |o| o.as_ptr()), slots, out.as_mut_ptr() as *mut f64) };
    if rc != 0 { panic!("lasgun: {}", last_error()) }
    out
}
/// `lens_rays` into device memory of `device`, enqueued on a HIP stream
///
/// # Safety
/// `dev_rays` must be device memory of `device` holding pixels * samples_root^2 * 6 doubles, `dev_offsets` null or `pixels` u64 there.
#[allow(clippy::too_many_arguments)]
pub unsafe fn lens_rays_device(device: i32, lens: &Lens, width: u32, height: u32, samples_root: u32, dev_offsets: *const u64, pixels: usize, dev_rays: *mut f64,
                               hip_stream: *mut std::ffi::c_void) {
    if sys::lg_lens_rays_device(device, lens, width, height, samples_root, dev_offsets, pixels, dev_rays, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
}

// ---------------------------------------------------------------------------------------------------------------
// Accel, render, capture, capture_subset (src/lib.rs:42-162)
// ---------------------------------------------------------------------------------------------------------------
/// The acceleration structure of a scene: the reference's nested HLBVH, built on the host exactly as the reference
/// builds it, flattened and resident in HBM.  Borrows the scene for its whole life (bvh.rs:45-46).
pub struct Accel<'s> {
    ptr: *mut sys::lg_accel,
    scene: PhantomData<&'s Scene>,
}

impl<'s> Accel<'s> {
    pub fn from(scene: &'s Scene) -> Accel<'s> {
        let ptr = unsafe { sys::lg_accel_from(scene.ptr) };
        if ptr.is_null() { panic!("lasgun: {}", last_error()) }
        Accel { ptr, scene: PhantomData }
    }
    /// false (default): the reference's own traversal over the reference's own BVH; true: the opt-in fast mode
    pub fn set_fast_mode(&self, fast: bool) {
        if unsafe { sys::lg_accel_set_mode(self.ptr, fast as i32) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// Closest hit of every ray (origin xyz, direction xyz): what the reference's `root.intersect` returns (bvh.rs:461-522), resolved to
    /// world space as shading sees it; `t` is +inf where a ray hits nothing.  No counterpart among the reference's public items.
    pub fn intersect(&self, rays: &[[f64; 6]]) -> Vec<sys::lg_hit> {
        let mut hits = vec![sys::lg_hit::default(); rays.len()];
        if rays.is_empty() { return hits }
        let rc = unsafe { sys::lg_intersect(self.ptr, rays.as_ptr() as *const f64, rays.len(), hits.as_mut_ptr()) };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        hits
    }
    /// Whether each segment o -> o + d is blocked (closest hit t < 1): the render's shadow test (point.rs:49)
    pub fn occluded(&self, rays: &[[f64; 6]]) -> Vec<bool> {
        let mut occ = vec![0u8; rays.len()];
        if rays.is_empty() { return Vec::new() }
        let rc = unsafe { sys::lg_occluded(self.ptr, rays.as_ptr() as *const f64, rays.len(), occ.as_mut_ptr()) };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        occ.into_iter().map(|b| b != 0).collect()
    }
    /// Visibility matrix of two point sets (`lg_visibility`): (bits, blocked) -- `from.len()` rows of ceil(to.len() / 8) bytes, bit j of row
    /// i (`(bits[i * row_bytes + (j >> 3)] >> (j & 7)) & 1`) set iff the segment from[i] -> to[j] is blocked, the test `occluded` makes for
    /// the ray (from[i], to[j] - from[i]); blocked[i] = the number of set bits of row i.  The segments are made on the device.
    pub fn visibility(&self, from: &[[f64; 3]], to: &[[f64; 3]]) -> (Vec<u8>, Vec<u32>) {
        let row_bytes = (to.len() + 7) / 8;
        let (mut bits, mut blocked) = (vec![0u8; from.len() * row_bytes], vec![0u32; from.len()]);
        if from.is_empty() || to.is_empty() { return (bits, blocked) }
        let rc = unsafe {
            sys::lg_visibility(self.ptr, from.as_ptr() as *const f64, from.len(), to.as_ptr() as *const f64, to.len(), bits.as_mut_ptr(), row_bytes,
                               blocked.as_mut_ptr())
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        (bits, blocked)
    }
    /// `visibility` for points in device memory (3 doubles each), enqueued on a HIP stream: n_from rows of `row_bytes` bytes at `dev_bits`
    /// and / or n_from u32 at `dev_blocked` (either may be null, not both)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of those sizes (the library checks what HIP can tell it).
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn visibility_device(&self, dev_from: *const f64, n_from: usize, dev_to: *const f64, n_to: usize, dev_bits: *mut u8, row_bytes: usize,
                                    dev_blocked: *mut u32, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_visibility_device(self.ptr, dev_from, n_from, dev_to, n_to, dev_bits, row_bytes, dev_blocked, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// Open directions above points (`lg_open_directions`): (bits, open, above) -- `points.len()` rows of ceil(dirs.len() / 8) bytes, bit k of
    /// row i (`(bits[i * row_bytes + (k >> 3)] >> (k & 7)) & 1`) set iff dirs[k] is above the horizon of points[i]
    /// (`(n.x*d.x + n.y*d.y) + n.z*d.z > 0.0`; every direction when `normals` is None) and `occluded` answers false for the ray
    /// (points[i], dirs[k]); open[i] / above[i] = the numbers of open directions and of directions above.  The rays are made on the device.
    pub fn open_directions(&self, points: &[[f64; 3]], normals: Option<&[[f64; 3]]>, dirs: &[[f64; 3]]) -> (Vec<u8>, Vec<u32>, Vec<u32>) {
        let row_bytes = (dirs.len() + 7) / 8;
        let (mut bits, mut open, mut above) = (vec![0u8; points.len() * row_bytes], vec![0u32; points.len()], vec![0u32; points.len()]);
        if points.is_empty() || dirs.is_empty() { return (bits, open, above) }
        if let Some(n) = normals { assert_eq!(n.len(), points.len(), "open_directions: one normal per point") }
        let rc = unsafe {
            sys::lg_open_directions(self.ptr, points.as_ptr() as *const f64, normals.map_or(std::ptr::null(), |n| n.as_ptr() as *const f64), points.len(),
                                    dirs.as_ptr() as *const f64, dirs.len(), bits.as_mut_ptr(), row_bytes, open.as_mut_ptr(), above.as_mut_ptr())
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        (bits, open, above)
    }
    /// `open_directions` for tables in device memory (3 doubles a vector), enqueued on a HIP stream: n_points rows of `row_bytes` bytes at
    /// `dev_bits` and / or n_points u32 at `dev_open` and `dev_above` (each may be null, not all three); `dev_normals` may be null
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of those sizes (the library checks what HIP can tell it).
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn open_directions_device(&self, dev_points: *const f64, dev_normals: *const f64, n_points: usize, dev_dirs: *const f64, n_dirs: usize,
                                         dev_bits: *mut u8, row_bytes: usize, dev_open: *mut u32, dev_above: *mut u32, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_open_directions_device(self.ptr, dev_points, dev_normals, n_points, dev_dirs, n_dirs, dev_bits, row_bytes, dev_open, dev_above, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// Range scan (`lg_range_scan`): the first hits along `beams[k]` from `origins[i]`, ray (i, k) at `i * beams.len() + k` of every plane
    /// given (`None` = not asked for; not all six).  `frames`: one row-major 3 x 3 matrix per pose whose columns are the sensor's axes in
    /// world space, `d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z`; `None`: the beams are the directions, bit for bit.  range = the hit's t
    /// (+inf: a miss), normal = the geometric normal faced toward the sensor, id = kind, prim, instance, material; `hits[i]` = the beams of
    /// pose i that hit, `nearest[i]` = its smallest non-negative finite range (+inf: none).  `lanes`: 0 auto, 1 beam lanes, 2 pose lanes.
    #[allow(clippy::too_many_arguments)]
    pub fn range_scan(&self, origins: &[[f64; 3]], frames: Option<&[[f64; 9]]>, beams: &[[f64; 3]], lanes: i32, range: Option<&mut [f32]>,
                      point: Option<&mut [[f32; 3]]>, normal: Option<&mut [[f32; 3]]>, id: Option<&mut [[u32; 4]]>, hits: Option<&mut [u32]>,
                      nearest: Option<&mut [f32]>) {
        const _: () = assert!(std::mem::size_of::<sys::lg_scan_out>() == 48);
        let pairs = origins.len().checked_mul(beams.len()).expect("range_scan: origins.len() * beams.len() overflows usize");
        assert!(frames.map_or(true, |m| m.len() == origins.len()), "range_scan: one frame per pose");
        assert!(range.as_ref().map_or(true, |p| p.len() == pairs) && point.as_ref().map_or(true, |p| p.len() == pairs)
                && normal.as_ref().map_or(true, |p| p.len() == pairs) && id.as_ref().map_or(true, |p| p.len() == pairs)
                && hits.as_ref().map_or(true, |p| p.len() == origins.len()) && nearest.as_ref().map_or(true, |p| p.len() == origins.len()),
                "range_scan: planes of origins.len() * beams.len() elements, hits and nearest of origins.len()");
        let out = sys::lg_scan_out {
            range: range.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            point: point.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f32),
            normal: normal.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f32),
            id: id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
            hits: hits.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            nearest: nearest.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
        };
        let rc = unsafe {
            sys::lg_range_scan(self.ptr, origins.as_ptr() as *const f64, frames.map_or(std::ptr::null(), |m| m.as_ptr() as *const f64), origins.len(),
                               beams.as_ptr() as *const f64, beams.len(), lanes, &out)
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `range_scan` for tables in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `range_scan` states (the library checks what HIP can tell it).
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn range_scan_device(&self, dev_origins: *const f64, dev_frames: *const f64, n_poses: usize, dev_beams: *const f64, n_beams: usize, lanes: i32,
                                    dev_out: &sys::lg_scan_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_range_scan_device(self.ptr, dev_origins, dev_frames, n_poses, dev_beams, n_beams, lanes, dev_out, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// Hit layers (`lg_hit_layers`): the first `max_layers` surfaces along each ray, layer j of ray i at `j * rays.len() + i` of every layer
    /// plane given (`None` = not asked for; not all five).  Segment j + 1 starts at layer j's `p - ng * 2^-36` and keeps the ray's direction.
    /// hits = `intersect`'s record of the segment (the miss record behind a ray's last layer), along = t_0 + .. + t_j (+inf behind the last
    /// layer), id = kind, prim, instance, material; `count[i]` = the layers found (== `max_layers`: the ray may have been cut short),
    /// `inside[i]` = t_1 + t_3 + ..: the length inside material of a ray that starts outside every closed solid.
    #[allow(clippy::too_many_arguments)]
    pub fn hit_layers(&self, rays: &[[f64; 6]], max_layers: u32, hits: Option<&mut [sys::lg_hit]>, along: Option<&mut [f64]>, id: Option<&mut [[u32; 4]]>,
                      count: Option<&mut [u32]>, inside: Option<&mut [f64]>) {
        const _: () = assert!(std::mem::size_of::<sys::lg_layers_out>() == 40);
        let total = rays.len().checked_mul(max_layers as usize).expect("hit_layers: rays.len() * max_layers overflows usize");
        assert!(hits.as_ref().map_or(true, |p| p.len() == total) && along.as_ref().map_or(true, |p| p.len() == total)
                && id.as_ref().map_or(true, |p| p.len() == total) && count.as_ref().map_or(true, |p| p.len() == rays.len())
                && inside.as_ref().map_or(true, |p| p.len() == rays.len()),
                "hit_layers: layer planes of rays.len() * max_layers elements, count and inside of rays.len()");
        let out = sys::lg_layers_out {
            hits: hits.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            along: along.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            id: id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
            count: count.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            inside: inside.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
        };
        let rc = unsafe { sys::lg_hit_layers(self.ptr, rays.as_ptr() as *const f64, rays.len(), max_layers, &out) };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `hit_layers` for rays in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `hit_layers` states (the library checks what HIP can tell it).
    pub unsafe fn hit_layers_device(&self, dev_rays: *const f64, n: usize, max_layers: u32, dev_out: &sys::lg_layers_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_hit_layers_device(self.ptr, dev_rays, n, max_layers, dev_out, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// Ray paths (`lg_trace_paths`): every ray followed through up to `max_bounces` vertices, the rule per material the caller's
    /// (`rules.len()` == the accel's material count).  Vertex j of ray i is at `j * rays.len() + i` of every vertex plane given: hits =
    /// `intersect`'s record of segment j (the miss record behind a path's last vertex), point = its p, id = kind, prim, instance, material,
    /// along = the running sum of t (+inf behind the last vertex).  Per ray: count = the vertices found, end = `sys::LG_PATH_END_*`, gain =
    /// the product of the rules' gains, last = the ray a cut path resumes from (or the segment the path ended on), medium = the final
    /// crossing parity.  `normal`: 0 the geometric, 1 the shading normal; `start_medium`: bit 0 per ray, `None` = all outside.
    pub fn trace_paths(&self, rays: &[[f64; 6]], max_bounces: u32, rules: &[PathRule], normal: i32, start_medium: Option<&[u32]>, out: Paths) {
        const _: () = assert!(std::mem::size_of::<sys::lg_paths_out>() == 72 && std::mem::size_of::<sys::lg_path_rule>() == 24);
        let n = rays.len();
        let total = n.checked_mul(max_bounces as usize).expect("trace_paths: rays.len() * max_bounces overflows usize");
        assert!(start_medium.map_or(true, |m| m.len() == n), "trace_paths: start_medium has one word per ray");
        assert!(out.hits.as_ref().map_or(true, |p| p.len() == total) && out.point.as_ref().map_or(true, |p| p.len() == total)
                && out.id.as_ref().map_or(true, |p| p.len() == total) && out.along.as_ref().map_or(true, |p| p.len() == total)
                && out.count.as_ref().map_or(true, |p| p.len() == n) && out.end.as_ref().map_or(true, |p| p.len() == n)
                && out.gain.as_ref().map_or(true, |p| p.len() == n) && out.last.as_ref().map_or(true, |p| p.len() == n)
                && out.medium.as_ref().map_or(true, |p| p.len() == n),
                "trace_paths: vertex planes of rays.len() * max_bounces elements, per-ray planes of rays.len()");
        let o = sys::lg_paths_out {
            hits: out.hits.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            point: out.point.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            id: out.id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
            along: out.along.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            count: out.count.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            end: out.end.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            gain: out.gain.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            last: out.last.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            medium: out.medium.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
        };
        let rc = unsafe {
            sys::lg_trace_paths(self.ptr, rays.as_ptr() as *const f64, n, max_bounces, rules.as_ptr(), rules.len(), normal,
                                start_medium.map_or(std::ptr::null(), |m| m.as_ptr()), &o)
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `trace_paths` for rays in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for);
    /// `rules` is a host slice, copied before the call returns
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `trace_paths` states (the library checks what HIP can tell it).
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn trace_paths_device(&self, dev_rays: *const f64, n: usize, max_bounces: u32, rules: &[PathRule], normal: i32, dev_start_medium: *const u32,
                                     dev_out: &sys::lg_paths_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_trace_paths_device(self.ptr, dev_rays, n, max_bounces, rules.as_ptr(), rules.len(), normal, dev_start_medium, dev_out, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// Surface scatter (`lg_scatter`): one level of li()'s tree, opened.  Row i of every plane given belongs to ray i: hits = `intersect`'s
    /// record, direct = the lights in order + ambient at a hit (the background li() returns at a miss), flags = `sys::LG_SCATTER_*`,
    /// reflect / refract = the specular children's rays, reflect_weight = the reflected child's spectrum, refract_weight = spectrum[3],
    /// |wi . ns|, pdf; an absent child's elements are +0.0.  li() to a depth of the caller's is
    /// (direct + reflect_weight * L(reflect)) + ((spectrum * L(refract)) * cos) / pdf, level by level; the scene's own depth plays no part.
    pub fn scatter(&self, rays: &[[f64; 6]], out: Scatter) {
        const _: () = assert!(std::mem::size_of::<sys::lg_scatter_out>() == 56);
        let n = rays.len();
        assert!(out.hits.as_ref().map_or(true, |p| p.len() == n) && out.direct.as_ref().map_or(true, |p| p.len() == n)
                && out.flags.as_ref().map_or(true, |p| p.len() == n) && out.reflect.as_ref().map_or(true, |p| p.len() == n)
                && out.reflect_weight.as_ref().map_or(true, |p| p.len() == n) && out.refract.as_ref().map_or(true, |p| p.len() == n)
                && out.refract_weight.as_ref().map_or(true, |p| p.len() == n),
                "scatter: every plane has rays.len() rows");
        let o = sys::lg_scatter_out {
            hits: out.hits.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            direct: out.direct.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            flags: out.flags.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            reflect: out.reflect.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            reflect_weight: out.reflect_weight.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            refract: out.refract.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            refract_weight: out.refract_weight.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
        };
        if unsafe { sys::lg_scatter(self.ptr, rays.as_ptr() as *const f64, n, &o) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `scatter` for rays in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `scatter` states (the library checks what HIP can tell it).
    pub unsafe fn scatter_device(&self, dev_rays: *const f64, n: usize, dev_out: &sys::lg_scatter_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_scatter_device(self.ptr, dev_rays, n, dev_out, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// Closest points (`lg_closest_points`): for each point (world space) the nearest surface point of the scene.  Row i of every plane
    /// given belongs to point i: distance (+inf where no surface lies within `radius`; `f64::INFINITY` = no limit), point = the closest
    /// point in world space (+0.0 for a miss), id = kind, prim, instance, material as in `lg_hit` (0, !0, !0, -1 for a miss).  The header's
    /// arithmetic over every primitive, bit for bit; a scene with a sphere under a non-uniform scale is refused (`sys::lg_scene_closest_gate` says which instance).
    pub fn closest_points(&self, points: &[[f64; 3]], radius: f64, out: Closest) {
        const _: () = assert!(std::mem::size_of::<sys::lg_closest_out>() == 24);
        let n = points.len();
        assert!(out.distance.as_ref().map_or(true, |p| p.len() == n) && out.point.as_ref().map_or(true, |p| p.len() == n)
                && out.id.as_ref().map_or(true, |p| p.len() == n), "closest_points: every plane has points.len() rows");
        let o = sys::lg_closest_out {
            distance: out.distance.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            point: out.point.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            id: out.id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
        };
        if unsafe { sys::lg_closest_points(self.ptr, points.as_ptr() as *const f64, n, radius, &o) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `closest_points` for points in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `closest_points` states (the library checks what HIP can tell it).
    pub unsafe fn closest_points_device(&self, dev_points: *const f64, n: usize, radius: f64, dev_out: &sys::lg_closest_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_closest_points_device(self.ptr, dev_points, n, radius, dev_out, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// Proximity queries (`lg_nearest`): for each point (world space), under `radii[i]` (`None`: the shared `radius`; `f64::INFINITY` = no
    /// limit), the `k` nearest primitives in ascending (squared distance, key) order, the count of ALL primitives within the radius and
    /// whether any is.  `touch` alone leaves a point's walk at its first contact; `count` has to meet every primitive within the radius.
    /// One candidate per primitive, `closest_points`' own: slot 0 under a shared radius is its answer, byte for byte.
    pub fn nearest(&self, points: &[[f64; 3]], radii: Option<&[f64]>, radius: f64, k: u32, out: Nearest) {
        const _: () = assert!(std::mem::size_of::<sys::lg_nearest_out>() == 40);
        let n = points.len();
        let nk = n * k as usize;
        assert!(k <= sys::LG_NEAREST_MAX_K && radii.map_or(true, |r| r.len() == n), "nearest: k <= LG_NEAREST_MAX_K, one radius per point");
        assert!(out.touch.as_ref().map_or(true, |p| p.len() == n) && out.count.as_ref().map_or(true, |p| p.len() == n)
                && out.distance.as_ref().map_or(true, |p| p.len() == nk) && out.point.as_ref().map_or(true, |p| p.len() == nk)
                && out.id.as_ref().map_or(true, |p| p.len() == nk), "nearest: touch and count have points.len() rows, a slot plane k times as many");
        let o = sys::lg_nearest_out {
            touch: out.touch.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            count: out.count.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            distance: out.distance.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            point: out.point.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            id: out.id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
        };
        let r = radii.map_or(std::ptr::null(), |r| r.as_ptr());
        if unsafe { sys::lg_nearest(self.ptr, points.as_ptr() as *const f64, r, n, radius, k, &o) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `nearest` for points (and radii, or null) in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `nearest` states (the library checks what HIP can tell it).
    pub unsafe fn nearest_device(&self, dev_points: *const f64, dev_radii: *const f64, n: usize, radius: f64, k: u32, dev_out: &sys::lg_nearest_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_nearest_device(self.ptr, dev_points, dev_radii, n, radius, k, dev_out, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// Segment proximity (`lg_closest_segments`): for each segment p0 .. p1 (world space, six numbers), under `radii[i]` (`None`: the
    /// shared `radius`; `f64::INFINITY` = no limit), the nearest surface point of the scene to the segment, the segment's parameter there,
    /// the distance and the primitive: capsules and swept spheres against the world.  `touch` alone leaves a segment's walk at its first
    /// contact.  A segment with p0 == p1 answers as `nearest` does at k = 1.
    pub fn closest_segments(&self, segments: &[[f64; 6]], radii: Option<&[f64]>, radius: f64, out: Segments) {
        const _: () = assert!(std::mem::size_of::<sys::lg_segments_out>() == 40);
        let n = segments.len();
        assert!(radii.map_or(true, |r| r.len() == n), "closest_segments: one radius per segment");
        assert!(out.touch.as_ref().map_or(true, |p| p.len() == n) && out.distance.as_ref().map_or(true, |p| p.len() == n)
                && out.param.as_ref().map_or(true, |p| p.len() == n) && out.point.as_ref().map_or(true, |p| p.len() == n)
                && out.id.as_ref().map_or(true, |p| p.len() == n), "closest_segments: every plane has segments.len() rows");
        let o = sys::lg_segments_out {
            touch: out.touch.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            distance: out.distance.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            param: out.param.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            point: out.point.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            id: out.id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
        };
        let r = radii.map_or(std::ptr::null(), |r| r.as_ptr());
        if unsafe { sys::lg_closest_segments(self.ptr, segments.as_ptr() as *const f64, r, n, radius, &o) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `closest_segments` for segments (and radii, or null) in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `closest_segments` states (the library checks what HIP can tell it).
    pub unsafe fn closest_segments_device(&self, dev_segments: *const f64, dev_radii: *const f64, n: usize, radius: f64, dev_out: &sys::lg_segments_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_closest_segments_device(self.ptr, dev_segments, dev_radii, n, radius, dev_out, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    fn attr_out(n: usize, out: Attributes, what: &str) -> sys::lg_attr_out {
        const _: () = assert!(std::mem::size_of::<sys::lg_attr_out>() == 56);
        assert!(out.hits.as_ref().map_or(true, |p| p.len() == n) && out.flags.as_ref().map_or(true, |p| p.len() == n)
                && out.bary.as_ref().map_or(true, |p| p.len() == n) && out.uv.as_ref().map_or(true, |p| p.len() == n)
                && out.local.as_ref().map_or(true, |p| p.len() == n) && out.frame.as_ref().map_or(true, |p| p.len() == n)
                && out.dp.as_ref().map_or(true, |p| p.len() == n),
                "{}: every plane has rays.len() rows", what);
        sys::lg_attr_out {
            hits: out.hits.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            flags: out.flags.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            bary: out.bary.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            uv: out.uv.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            local: out.local.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            frame: out.frame.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            dp: out.dp.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
        }
    }
    /// Hit attributes (`lg_hit_attributes`): every ray's closest hit with where on its primitive it lies and the frame it is shaded in.
    /// Row i of every plane given belongs to ray i: hits = `intersect`'s record, flags = `sys::LG_ATTR_HIT` or 0, bary = a triangle hit's
    /// barycentrics, uv = the surface parameter, local = the hit point in the primitive's own space, frame = the BSDF's tangents ss, ts,
    /// dp = the world-space geometric dpdu, dpdv; a miss's rows are +0.0.
    pub fn hit_attributes(&self, rays: &[[f64; 6]], out: Attributes) {
        let n = rays.len();
        let o = Self::attr_out(n, out, "hit_attributes");
        if unsafe { sys::lg_hit_attributes(self.ptr, rays.as_ptr() as *const f64, n, &o) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `hit_attributes` without a walk (`lg_hit_attributes_of`): the primitives that `records` NAME (kind, prim, instance of each are
    /// read) resolved for `rays`; flags also `sys::LG_ATTR_NO_HIT` and `sys::LG_ATTR_BAD_RECORD`; `out.hits` must be `None`.
    pub fn hit_attributes_of(&self, rays: &[[f64; 6]], records: &[sys::lg_hit], out: Attributes) {
        let n = rays.len();
        assert!(records.len() == n, "hit_attributes_of: one record per ray");
        let o = Self::attr_out(n, out, "hit_attributes_of");
        if unsafe { sys::lg_hit_attributes_of(self.ptr, rays.as_ptr() as *const f64, records.as_ptr(), n, &o) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `hit_attributes` for rays in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `hit_attributes` states (the library checks what HIP can tell it).
    pub unsafe fn hit_attributes_device(&self, dev_rays: *const f64, n: usize, dev_out: &sys::lg_attr_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_hit_attributes_device(self.ptr, dev_rays, n, dev_out, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `hit_attributes_of` for rays and records in device memory, enqueued on a HIP stream
    ///
    /// # Safety
    /// As `hit_attributes_device`; `dev_hits` holds n 16-byte aligned `lg_hit` records.
    pub unsafe fn hit_attributes_of_device(&self, dev_rays: *const f64, dev_hits: *const sys::lg_hit, n: usize, dev_out: &sys::lg_attr_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_hit_attributes_of_device(self.ptr, dev_rays, dev_hits, n, dev_out, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// Lit scatter (`lg_scatter_lit`): `scatter` under lights that come with the call.  `lights`: K records shared by every ray
    /// (`per_ray` false) or rays.len() * K records, ray i's at i * K (`per_ray` true); `ambient` stands where the scene's ambient colour
    /// stands; the scene's own lights play no part.  `terms[i * K + k]` is light k's own term of ray i's `direct` (+0.0 where it is not
    /// added), bit k & 31 of `visible[i * W + (k >> 5)]`, W = ceil(K / 32), is set iff light k is visible from the hit.
    pub fn scatter_lit(&self, rays: &[[f64; 6]], lights: &[Light], per_ray: bool, ambient: [f64; 3], out: ScatterLit) {
        const _: () = assert!(std::mem::size_of::<sys::lg_light>() == 72 && std::mem::size_of::<sys::lg_light_set>() == 40 && std::mem::size_of::<sys::lg_lit_out>() == 72);
        let n = rays.len();
        assert!(!per_ray || n == 0 || lights.len() % n == 0, "scatter_lit: a per-ray table holds rays.len() * K lights");
        let k = if per_ray { if n == 0 { 0 } else { lights.len() / n } } else { lights.len() };
        let w = (k + 31) / 32;
        assert!(k <= sys::LG_MAX_CALL_LIGHTS as usize, "scatter_lit: at most LG_MAX_CALL_LIGHTS lights");
        let sc = out.scatter;
        assert!(sc.hits.as_ref().map_or(true, |p| p.len() == n) && sc.direct.as_ref().map_or(true, |p| p.len() == n)
                && sc.flags.as_ref().map_or(true, |p| p.len() == n) && sc.reflect.as_ref().map_or(true, |p| p.len() == n)
                && sc.reflect_weight.as_ref().map_or(true, |p| p.len() == n) && sc.refract.as_ref().map_or(true, |p| p.len() == n)
                && sc.refract_weight.as_ref().map_or(true, |p| p.len() == n) && out.terms.as_ref().map_or(true, |p| p.len() == n * k)
                && out.visible.as_ref().map_or(true, |p| p.len() == n * w),
                "scatter_lit: every scatter plane has rays.len() rows, terms rays.len() * K, visible rays.len() * ceil(K / 32)");
        let o = sys::lg_lit_out {
            scatter: sys::lg_scatter_out {
                hits: sc.hits.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
                direct: sc.direct.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
                flags: sc.flags.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
                reflect: sc.reflect.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
                reflect_weight: sc.reflect_weight.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
                refract: sc.refract.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
                refract_weight: sc.refract_weight.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            },
            terms: out.terms.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            visible: out.visible.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
        };
        let ls = sys::lg_light_set { lights: if lights.is_empty() { std::ptr::null() } else { lights.as_ptr() }, count: k as u32, per_ray: per_ray as u32, ambient };
        if unsafe { sys::lg_scatter_lit(self.ptr, rays.as_ptr() as *const f64, n, &ls, &o) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `scatter_lit` for rays in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for);
    /// `lights.lights` is a HOST table when `per_ray` is 0 (staged by the call: it may be freed on return), device memory when it is 1
    ///
    /// # Safety
    /// The pointers must be memory of the kinds and sizes `scatter_lit` states (the library checks what HIP can tell it).
    pub unsafe fn scatter_lit_device(&self, dev_rays: *const f64, n: usize, lights: &sys::lg_light_set, dev_out: &sys::lg_lit_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_scatter_lit_device(self.ptr, dev_rays, n, lights, dev_out, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// Radiance along every ray (origin xyz, direction xyz): what the reference's `integrate` leaves for a pixel whose one sample is that
    /// ray (integrate.rs:16-20, 23-132) -- lights, shadows, ambient, specular recursion, background on a miss --, f64 RGB before quantisation.
    /// For rays no camera of the scene generates: probes, panoramas, bakes, a second view of one accel.
    pub fn radiance(&self, rays: &[[f64; 6]]) -> Vec<[f64; 3]> {
        let mut out = vec![[0f64; 3]; rays.len()];
        if rays.is_empty() { return out }
        let rc = unsafe { sys::lg_radiance(self.ptr, rays.as_ptr() as *const f64, rays.len(), out.as_mut_ptr() as *mut f64) };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        out
    }
    /// The scene's point lights: the mask bits a light group may use (`lg_accel_light_count`).
    pub fn light_count(&self) -> usize {
        let n = unsafe { sys::lg_accel_light_count(self.ptr) };
        if n < 0 { panic!("lasgun: {}", last_error()) }
        n as usize
    }
    /// Light groups (`lg_radiance_groups`): `radiance` split by subsets of the scene's lights, `groups.len()` planes from one chain of
    /// walks, group-major: plane g of ray r at `g * rays.len() + r`.  Plane g is what `radiance` returns on an accel rebuilt with the
    /// lights of `groups[g].lights` alone (bit l: light l in add order) and, without `sys::LG_GROUP_AMBIENT` in its flags, no ambient
    /// term -- bit for bit.  The background belongs to every group.  At most `sys::LG_MAX_LIGHT_GROUPS` groups.
    pub fn radiance_groups(&self, rays: &[[f64; 6]], groups: &[sys::lg_light_group]) -> Vec<[f64; 3]> {
        const _: () = assert!(std::mem::size_of::<sys::lg_light_group>() == 8);
        let total = rays.len().checked_mul(groups.len()).expect("radiance_groups: rays.len() * groups.len() overflows usize");
        let mut out = vec![[0f64; 3]; total];
        if rays.is_empty() { return out }
        let rc = unsafe {
            sys::lg_radiance_groups(self.ptr, rays.as_ptr() as *const f64, rays.len(), groups.as_ptr(), groups.len(), out.as_mut_ptr() as *mut f64)
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        out
    }
    /// `radiance_groups` for rays in device memory, enqueued on a HIP stream; `groups` is a host slice and may be dropped on return
    ///
    /// # Safety
    /// `dev_rays` (6 n doubles) and `dev_radiance` (groups.len() * n * 3 doubles) must be device memory of the accel's device (the
    /// library checks what HIP can tell it).
    pub unsafe fn radiance_groups_device(&self, dev_rays: *const f64, n: usize, groups: &[sys::lg_light_group], dev_radiance: *mut f64,
                                         hip_stream: *mut std::ffi::c_void) {
        if sys::lg_radiance_groups_device(self.ptr, dev_rays, n, groups.as_ptr(), groups.len(), dev_radiance, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// Radiance gather (`lg_radiance_gather`): li() along `dirs[k]` from `origins[i]`, what `radiance` returns for that ray, at
    /// `i * dirs.len() + k` of `radiance`, and / or reduced per pose into `sums`: `sums[i * n_weights + c]` = the sum over k, in order from
    /// +0.0, of radiance(i, k) * `weights[k * n_weights + c]` (one product, one sum a step).  `None` = not asked for; not both.  `weights`:
    /// `dirs.len() * n_weights` doubles, k-major, looked at only with `sums`.  `frames`: one row-major 3 x 3 matrix per pose,
    /// `d[c] = (M[3c]*b.x + M[3c+1]*b.y) + M[3c+2]*b.z`; `None`: the directions are used bit for bit.  `lanes`: 0 auto, 1 direction lanes, 2 pose lanes.
    #[allow(clippy::too_many_arguments)]
    pub fn radiance_gather(&self, origins: &[[f64; 3]], frames: Option<&[[f64; 9]]>, dirs: &[[f64; 3]], weights: Option<&[f64]>, n_weights: usize, lanes: i32,
                           radiance: Option<&mut [[f64; 3]]>, sums: Option<&mut [[f64; 3]]>) {
        const _: () = assert!(std::mem::size_of::<sys::lg_gather_out>() == 16);
        let pairs = origins.len().checked_mul(dirs.len()).expect("radiance_gather: origins.len() * dirs.len() overflows usize");
        assert!(frames.map_or(true, |m| m.len() == origins.len()), "radiance_gather: one frame per pose");
        assert!(radiance.as_ref().map_or(true, |p| p.len() == pairs), "radiance_gather: radiance of origins.len() * dirs.len() elements");
        if let Some(s) = sums.as_ref() {
            assert!(s.len() == origins.len() * n_weights && weights.map_or(false, |w| w.len() == dirs.len() * n_weights),
                    "radiance_gather: sums of origins.len() * n_weights elements, weights of dirs.len() * n_weights");
        }
        let out = sys::lg_gather_out {
            radiance: radiance.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
            sums: sums.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f64),
        };
        let rc = unsafe {
            sys::lg_radiance_gather(self.ptr, origins.as_ptr() as *const f64, frames.map_or(std::ptr::null(), |m| m.as_ptr() as *const f64), origins.len(),
                                    dirs.as_ptr() as *const f64, dirs.len(), weights.map_or(std::ptr::null(), |w| w.as_ptr()), n_weights, lanes, &out)
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `radiance_gather` for tables in device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of the sizes `radiance_gather` states (the library checks what HIP can tell it).
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn radiance_gather_device(&self, dev_origins: *const f64, dev_frames: *const f64, n_poses: usize, dev_dirs: *const f64, n_dirs: usize,
                                         dev_weights: *const f64, n_weights: usize, lanes: i32, dev_out: &sys::lg_gather_out, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_radiance_gather_device(self.ptr, dev_origins, dev_frames, n_poses, dev_dirs, n_dirs, dev_weights, n_weights, lanes, dev_out, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// `radiance` for rays in device memory (6 doubles each), enqueued on a HIP stream: 3 n doubles at `dev_radiance`
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device holding n rays / 3 n doubles (the library checks what HIP can tell it).
    pub unsafe fn radiance_device(&self, dev_rays: *const f64, n: usize, dev_radiance: *mut f64, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_radiance_device(self.ptr, dev_rays, n, dev_radiance, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// A film from the caller's rays (`lg_capture_rays`): pixel slot g's rays are `rays[g*samples .. (g+1)*samples]`, summed in that order,
    /// scaled by 1 / samples, quantised like the render's pixels and written at film offset `offsets[g]` (y*width + x), or g without
    /// offsets.  A slot whose offset lies behind the film writes nothing; pixels no slot names keep their bytes.  `rgb`: the same values
    /// before quantisation, width*height of them, addressed like the film.  For the scene's own camera rays this is `capture`'s film.
    pub fn capture_rays(&self, rays: &[[f64; 6]], samples: u32, offsets: Option<&[u64]>, width: u32, height: u32, pixels: &mut [Pixel], rgb: Option<&mut [[f64; 3]]>) {
        let area = (width as usize) * (height as usize);
        assert!(samples > 0 && rays.len() % samples as usize == 0, "capture_rays: pixel slots * samples rays");
        let slots = rays.len() / samples as usize;
        assert!(pixels.len() == area && offsets.map_or(true, |o| o.len() == slots) && rgb.as_ref().map_or(true, |r| r.len() == area));
        if slots == 0 { return }
        let film = unsafe { sys::lg_film_wrap(width, height, pixels.as_mut_ptr() as *mut u8) };
        let rc = unsafe {
            sys::lg_capture_rays(self.ptr, rays.as_ptr() as *const f64, slots, samples, offsets.map_or(std::ptr::null(), |o| o.as_ptr()), film,
                                 rgb.map_or(std::ptr::null_mut(), |r| r.as_mut_ptr() as *mut f64), width, height)
        };
        unsafe { sys::lg_film_free(film) };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `capture_rays` for buffers in device memory, enqueued on a HIP stream: width*height RGBA8 words at `dev_rgba` and / or width*height*3
    /// doubles at `dev_rgb` (either may be null, not both); `dev_offsets` may be null
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device of those sizes (the library checks what HIP can tell it).
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn capture_rays_device(&self, dev_rays: *const f64, pixels: usize, samples: u32, dev_offsets: *const u64, width: u32, height: u32,
                                      dev_rgba: *mut std::ffi::c_void, dev_rgb: *mut f64, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_capture_rays_device(self.ptr, dev_rays, pixels, samples, dev_offsets, width, height, dev_rgba, dev_rgb, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// The camera of the scene this accel was built from, as a view (`lg_accel_view`): `capture_views` of it is `capture`'s film.
    pub fn view(&self) -> View {
        let mut v: View = unsafe { std::mem::zeroed() };
        if unsafe { sys::lg_accel_view(self.ptr, &mut v) } != 0 { panic!("lasgun: {}", last_error()) }
        v
    }
    /// `camera_rays` with `view` in the camera's place (`lg_view_rays`): the pixels [x0,x1) x [y0,y1) of a width x height film, row-major,
    /// samples_root^2 rays a pixel in camera order.
    pub fn view_rays(&self, view: &View, width: u32, height: u32, rect: (u32, u32, u32, u32)) -> Vec<[f64; 6]> {
        let (x0, y0, x1, y1) = rect;
        let n = (x1.saturating_sub(x0) as usize) * (y1.saturating_sub(y0) as usize) * (view.samples_root as usize) * (view.samples_root as usize);
        let mut out = vec![[0f64; 6]; n];
        let rc = unsafe { sys::lg_view_rays(self.ptr, view, width, height, x0, y0, x1, y1, if n == 0 { std::ptr::null_mut() } else { out.as_mut_ptr() as *mut f64 }) };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        out
    }
    /// `view_rays` into device memory, enqueued on a HIP stream
    ///
    /// # Safety
    /// `dev_rays` must be device memory of the accel's device holding the rectangle's rays, 6 doubles each.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn view_rays_device(&self, view: &View, width: u32, height: u32, rect: (u32, u32, u32, u32), dev_rays: *mut f64, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_view_rays_device(self.ptr, view, width, height, rect.0, rect.1, rect.2, rect.3, dev_rays, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// This accel from K cameras into K width x height films in ONE call (`lg_capture_views`): film v is `pixels[v*width*height ..]`, its
    /// f64 RGB before quantisation `rgb[v*width*height ..]`.  The views share samples_root.  Either output may be absent, not both.
    pub fn capture_views(&self, views: &[View], width: u32, height: u32, pixels: Option<&mut [Pixel]>, rgb: Option<&mut [[f64; 3]]>) {
        let n = views.len().checked_mul((width as usize) * (height as usize)).expect("capture_views: views.len() * width * height overflows usize");
        assert!(pixels.as_ref().map_or(true, |p| p.len() == n) && rgb.as_ref().map_or(true, |r| r.len() == n), "capture_views: views.len() * width * height pixels");
        let rc = unsafe {
            sys::lg_capture_views(self.ptr, views.as_ptr(), views.len(), width, height, pixels.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u8),
                                  rgb.map_or(std::ptr::null_mut(), |r| r.as_mut_ptr() as *mut f64))
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `capture_views` for films in device memory, enqueued on a HIP stream; `views` stays a host slice, copied before the call returns
    ///
    /// # Safety
    /// `dev_rgba` / `dev_rgb` must be null or device memory of the accel's device holding views.len() * width * height RGBA8 words / RGB triples.
    pub unsafe fn capture_views_device(&self, views: &[View], width: u32, height: u32, dev_rgba: *mut std::ffi::c_void, dev_rgb: *mut f64, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_capture_views_device(self.ptr, views.as_ptr(), views.len(), width, height, dev_rgba, dev_rgb, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// The number of materials of the accel's tables (`lg_accel_material_count`): the rows of `capture_features`' `material_rgb`.
    pub fn material_count(&self) -> usize { unsafe { sys::lg_accel_material_count(self.ptr) } }
    /// Feature buffers of the scene's own camera view (`lg_capture_features`): first-hit depth, shading normal, albedo, coverage and ids of
    /// the pixels [x0,x1) x [y0,y1) of a width x height film, the rays made on the device in the render's 8 x 8 tiles.  Every plane given is
    /// width*height long and addressed like the film (y*width + x); pixels outside the rectangle keep their values.  Normal and albedo are
    /// means over all the pixel's samples (premultiplied by coverage), depth the mean over the samples that hit (+inf: none), id sample 0's
    /// kind, prim, instance, material.  `material_rgb`: `material_count()` colours, summed per hit material (required with albedo).
    #[allow(clippy::too_many_arguments)]
    pub fn capture_features(&self, width: u32, height: u32, rect: (u32, u32, u32, u32), depth: Option<&mut [f32]>, normal: Option<&mut [[f32; 3]]>,
                            albedo: Option<&mut [[f32; 3]]>, coverage: Option<&mut [f32]>, id: Option<&mut [[u32; 4]]>, material_rgb: Option<&[[f64; 3]]>) {
        let area = (width as usize) * (height as usize);
        assert!(depth.as_ref().map_or(true, |p| p.len() == area) && normal.as_ref().map_or(true, |p| p.len() == area)
                && albedo.as_ref().map_or(true, |p| p.len() == area) && coverage.as_ref().map_or(true, |p| p.len() == area)
                && id.as_ref().map_or(true, |p| p.len() == area), "capture_features: planes of width * height pixels");
        assert!(material_rgb.map_or(true, |m| m.len() == self.material_count()), "capture_features: material_count() colours");
        let out = sys::lg_features {
            depth: depth.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            normal: normal.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f32),
            albedo: albedo.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f32),
            coverage: coverage.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            id: id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
        };
        let rc = unsafe {
            sys::lg_capture_features(self.ptr, width, height, rect.0, rect.1, rect.2, rect.3, &out, material_rgb.map_or(std::ptr::null(), |m| m.as_ptr() as *const f64))
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `capture_features` into device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked for)
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device, width*height pixels a plane and `material_count()` * 3 doubles (the
    /// library checks what HIP can tell it).
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn capture_features_device(&self, width: u32, height: u32, rect: (u32, u32, u32, u32), dev_out: &sys::lg_features, dev_material_rgb: *const f64,
                                          hip_stream: *mut std::ffi::c_void) {
        if sys::lg_capture_features_device(self.ptr, width, height, rect.0, rect.1, rect.2, rect.3, dev_out, dev_material_rgb, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// View features (`lg_capture_view_features`): `capture_features`' planes and the world-space hit point for K views in ONE call, K whole
    /// films.  Every plane given is views.len()*width*height long, the element of (v, x, y) at v*width*height + y*width + x.  depth and
    /// point are means over the samples that hit (+inf and (0, 0, 0): none); point is what reprojects a pixel of one view into another.
    /// The views share `samples_root`.  `material_rgb`: `material_count()` colours, summed per hit material (required with albedo).
    #[allow(clippy::too_many_arguments)]
    pub fn capture_view_features(&self, views: &[View], width: u32, height: u32, depth: Option<&mut [f32]>, normal: Option<&mut [[f32; 3]]>,
                                 albedo: Option<&mut [[f32; 3]]>, coverage: Option<&mut [f32]>, id: Option<&mut [[u32; 4]]>, point: Option<&mut [[f32; 3]]>,
                                 material_rgb: Option<&[[f64; 3]]>) {
        const _: () = assert!(std::mem::size_of::<sys::lg_view_features>() == 48);
        let n = views.len().checked_mul((width as usize) * (height as usize)).expect("capture_view_features: views.len() * width * height overflows usize");
        assert!(depth.as_ref().map_or(true, |p| p.len() == n) && normal.as_ref().map_or(true, |p| p.len() == n)
                && albedo.as_ref().map_or(true, |p| p.len() == n) && coverage.as_ref().map_or(true, |p| p.len() == n)
                && id.as_ref().map_or(true, |p| p.len() == n) && point.as_ref().map_or(true, |p| p.len() == n),
                "capture_view_features: planes of views.len() * width * height pixels");
        assert!(material_rgb.map_or(true, |m| m.len() == self.material_count()), "capture_view_features: material_count() colours");
        let out = sys::lg_view_features {
            depth: depth.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            normal: normal.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f32),
            albedo: albedo.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f32),
            coverage: coverage.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr()),
            id: id.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut u32),
            point: point.map_or(std::ptr::null_mut(), |p| p.as_mut_ptr() as *mut f32),
        };
        let rc = unsafe {
            sys::lg_capture_view_features(self.ptr, views.as_ptr(), views.len(), width, height, &out, material_rgb.map_or(std::ptr::null(), |m| m.as_ptr() as *const f64))
        };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
    }
    /// `capture_view_features` into device memory, enqueued on a HIP stream: `dev_out`'s members are device pointers (null = not asked
    /// for); `views` stays a host slice, copied before the call returns
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device, views.len()*width*height pixels a plane and `material_count()` * 3
    /// doubles (the library checks what HIP can tell it).
    pub unsafe fn capture_view_features_device(&self, views: &[View], width: u32, height: u32, dev_out: &sys::lg_view_features, dev_material_rgb: *const f64,
                                               hip_stream: *mut std::ffi::c_void) {
        if sys::lg_capture_view_features_device(self.ptr, views.as_ptr(), views.len(), width, height, dev_out, dev_material_rgb, hip_stream) != 0 {
            panic!("lasgun: {}", last_error())
        }
    }
    /// The order a query's rays are walked in: false (default) as given, true sorted on the device by a coherence key -- for rays that
    /// arrive in no particular order; the sort is part of every query's time.  The answers are the same bytes either way.
    pub fn set_query_order(&self, sorted: bool) {
        if unsafe { sys::lg_accel_set_query_order(self.ptr, sorted as i32) } != 0 { panic!("lasgun: {}", last_error()) }
    }
    pub fn get_query_order(&self) -> bool {
        unsafe { sys::lg_accel_get_query_order(self.ptr) != 0 }
    }
    /// The order `set_query_order(true)` walks these rays in: (perm, keys) -- perm[s] the ray walked in slot s, keys[i] ray i's key;
    /// perm is the stable ascending sort of keys.
    pub fn query_order(&self, rays: &[[f64; 6]]) -> (Vec<u32>, Vec<u32>) {
        let (mut perm, mut keys) = (vec![0u32; rays.len()], vec![0u32; rays.len()]);
        if rays.is_empty() { return (perm, keys) }
        let rc = unsafe { sys::lg_query_order(self.ptr, rays.as_ptr() as *const f64, rays.len(), perm.as_mut_ptr(), keys.as_mut_ptr()) };
        if rc != 0 { panic!("lasgun: {}", last_error()) }
        (perm, keys)
    }
    /// `query_order` for rays in device memory (6 doubles each), enqueued on a HIP stream: n u32 at `dev_perm` and, unless null, at `dev_keys`
    ///
    /// # Safety
    /// The pointers must be device memory of the accel's device holding n rays / n u32 (the library checks what HIP can tell it).
    pub unsafe fn query_order_device(&self, dev_rays: *const f64, n: usize, dev_perm: *mut u32, dev_keys: *mut u32, hip_stream: *mut std::ffi::c_void) {
        if sys::lg_query_order_device(self.ptr, dev_rays, n, dev_perm, dev_keys, hip_stream) != 0 { panic!("lasgun: {}", last_error()) }
    }
}
impl<'s> Drop for Accel<'s> {
    fn drop(&mut self) { unsafe { sys::lg_accel_free(self.ptr) } }
}
// The reference shares `&Accel` between its capture threads (lib.rs:67-103).  The C side guards every entry point that takes
// an accel with that accel's own mutex (internal.h: lg_accel), so the handle may be used and dropped from any thread.
unsafe impl<'s> Send for Accel<'s> {}
unsafe impl<'s> Sync for Accel<'s> {}

/// GPUs a `capture` / `render` is split over (none given: every visible device); see `Scene::set_threads`
pub fn set_devices(devices: &[i32]) {
    if unsafe { sys::lg_set_devices(devices.as_ptr(), devices.len() as i32) } != 0 { panic!("lasgun: {}", last_error()) }
}

/// Render the given scene (lib.rs:46-50)
pub fn render(scene: &Scene, resolution: (u32, u32)) -> Film {
    let mut film = Film::new(resolution.0, resolution.1);
    capture(scene, &mut film);
    film
}

/// Record an image of the scene on the given film (lib.rs:55-104): the BVH is (re)built inside, the call returns when
/// every pixel is written.
pub fn capture(scene: &Scene, film: &mut Film) {
    let (w, h) = (film.w, film.h);
    let staging = unsafe { sys::lg_film_new(w, h) };
    let rc = unsafe { sys::lg_capture(scene.ptr, staging) };
    if rc != 0 {
        unsafe { sys::lg_film_free(staging) };
        panic!("lasgun: {}", last_error())
    }
    let px = unsafe { std::slice::from_raw_parts(sys::lg_film_pixels(staging), (w as usize) * (h as usize) * 4) };
    for (at, p) in px.chunks_exact(4).enumerate() { film[at] = [p[0], p[1], p[2], p[3]] }
    unsafe { sys::lg_film_free(staging) }
}

/// Capture subset k of n: every pixel {k + i*n} of the row-major pixel buffer and no other (lib.rs:110-162)
pub fn capture_subset(k: usize, n: usize, root: &Accel, img: &mut impl Img) {
    assert!(n > 0);
    let (w, h) = (img.w(), img.h());
    let area = (w as usize) * (h as usize);
    let offsets: Vec<u64> = (k..area).step_by(n).map(|o| o as u64).collect();
    if offsets.is_empty() { return }
    let mut rgba = vec![0u8; offsets.len() * 4];
    let rc = unsafe { sys::lg_capture_pixels(root.ptr, w, h, offsets.as_ptr(), offsets.len(), rgba.as_mut_ptr(), std::ptr::null_mut()) };
    if rc != 0 { panic!("lasgun: {}", last_error()) }
    for (i, offset) in offsets.iter().enumerate() {
        let (x, y) = ((*offset as usize % w as usize) as u32, (*offset as usize / w as usize) as u32);
        img.set(x, y, &[rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]])
    }
}

/// Several subsets of one `n` in ONE render: writes what the calls `capture_subset(k, n, ..)` for `k` in `ks` write, and nothing else.
/// No counterpart in the reference, whose progressive front end calls `capture_subset` a hundred times in a row
/// (www/renderer.ts:103-120); on a GPU a batch costs `ks.len() / n` of a frame instead of a launch chain per subset.
pub fn capture_subsets(ks: &[usize], n: usize, root: &Accel, img: &mut impl Img) {
    assert!(n > 0);
    let (w, h) = (img.w(), img.h());
    let area = (w as usize) * (h as usize);
    let staging = unsafe { sys::lg_film_new(w, h) };
    let rc = unsafe { sys::lg_capture_subsets(ks.as_ptr(), ks.len(), n, root.ptr, staging) };
    if rc != 0 {
        unsafe { sys::lg_film_free(staging) };
        panic!("lasgun: {}", last_error())
    }
    let px = unsafe { std::slice::from_raw_parts(sys::lg_film_pixels(staging), area * 4) };
    for &k in ks {
        for o in (k..area).step_by(n) {
            img.set((o % w as usize) as u32, (o / w as usize) as u32, &[px[4 * o], px[4 * o + 1], px[4 * o + 2], px[4 * o + 3]])
        }
    }
    unsafe { sys::lg_film_free(staging) }
}

// ---------------------------------------------------------------------------------------------------------------
// The table of measured kernel-organisation choices (no counterpart in the reference; include/lasgun_hip.h, lg_tune_*):
// export it once, import it at start-up, and no launch of a known kind is ever measured again.
// ---------------------------------------------------------------------------------------------------------------
pub mod tune {
    use super::*;
    pub use sys::lg_tune_entry as Entry;
    pub fn export() -> Vec<Entry> {
        let n = unsafe { sys::lg_tune_export(std::ptr::null_mut(), 0) };
        let mut v = vec![Entry::default(); n];
        let m = unsafe { sys::lg_tune_export(v.as_mut_ptr(), n) };
        v.truncate(m.min(n));
        v
    }
    pub fn import(entries: &[Entry]) { if unsafe { sys::lg_tune_import(entries.as_ptr(), entries.len()) } != 0 { panic!("lasgun: {}", last_error()) } }
    pub fn clear() { unsafe { sys::lg_tune_clear() } }
}

// ---------------------------------------------------------------------------------------------------------------
// output::render (src/output.rs:5-18): render to a PNG file
// ---------------------------------------------------------------------------------------------------------------
pub mod output {
    use super::*;
    use std::io::Write;

    struct Image { w: u32, h: u32, px: Vec<Pixel> }
    impl Index<usize> for Image {
        type Output = Pixel;
        fn index(&self, at: usize) -> &Pixel { &self.px[at] }
    }
    impl IndexMut<usize> for Image {
        fn index_mut(&mut self, at: usize) -> &mut Pixel { &mut self.px[at] }
    }
    impl PixelBuffer for Image {
        fn save(&self, filename: &str) { write_png(filename, self.w, self.h, &self.px).unwrap() }
    }

    pub fn render(scene: &Scene, resolution: [u32; 2], filename: &str) {
        let mut film = self::film(resolution);
        capture(scene, &mut film);
        film.save(filename)
    }
    /// A film in the given dimensions whose `save` writes a PNG
    pub fn film(resolution: [u32; 2]) -> Film {
        let (w, h) = (resolution[0], resolution[1]);
        Film::new_with_output(w, h, Box::new(Image { w, h, px: vec![[0, 0, 0, 0]; (w as usize) * (h as usize)] }))
    }

    fn crc32(data: &[u8]) -> u32 {
        let mut c = 0xFFFF_FFFFu32;
        for &b in data {
            c ^= b as u32;
            for _ in 0..8 { c = if c & 1 != 0 { 0xEDB8_8320 ^ (c >> 1) } else { c >> 1 } }
        }
        !c
    }
    fn chunk(out: &mut Vec<u8>, kind: &[u8; 4], data: &[u8]) {
        out.extend_from_slice(&(data.len() as u32).to_be_bytes());
        let mut body = kind.to_vec();
        body.extend_from_slice(data);
        out.extend_from_slice(&body);
        out.extend_from_slice(&crc32(&body).to_be_bytes());
    }
    /// 8-bit RGBA PNG, filter 0 rows in stored (uncompressed) deflate blocks
    fn write_png(filename: &str, w: u32, h: u32, px: &[Pixel]) -> std::io::Result<()> {
        let mut raw = Vec::with_capacity((w as usize * 4 + 1) * h as usize);
        for row in px.chunks((w as usize).max(1)) {
            raw.push(0u8);
            for p in row { raw.extend_from_slice(p) }
        }
        let (mut a, mut b) = (1u32, 0u32); // adler32
        for &v in &raw { a = (a + v as u32) % 65521; b = (b + a) % 65521 }
        let mut z = vec![0x78u8, 0x01];
        if raw.is_empty() { z.extend_from_slice(&[1, 0, 0, 0xFF, 0xFF]) } // a film without pixels: one empty final block
        let mut blocks = raw.chunks(65535).peekable();
        while let Some(block) = blocks.next() {
            z.push(if blocks.peek().is_none() { 1 } else { 0 });
            z.extend_from_slice(&(block.len() as u16).to_le_bytes());
            z.extend_from_slice(&(!(block.len() as u16)).to_le_bytes());
            z.extend_from_slice(block);
        }
        z.extend_from_slice(&((b << 16) | a).to_be_bytes());
        let mut out = vec![0x89, b'P', b'N', b'G', 0x0D, 0x0A, 0x1A, 0x0A];
        let mut ihdr = Vec::new();
        ihdr.extend_from_slice(&w.to_be_bytes());
        ihdr.extend_from_slice(&h.to_be_bytes());
        ihdr.extend_from_slice(&[8, 6, 0, 0, 0]);
        chunk(&mut out, b"IHDR", &ihdr);
        chunk(&mut out, b"IDAT", &z);
        chunk(&mut out, b"IEND", &[]);
        std::fs::File::create(filename)?.write_all(&out)
    }
}
