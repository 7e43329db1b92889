// lasgun_amd/csrc/view_ray.h -- what the kernels of k_views.hip (lg_capture_views*) and k_view_features.hip (lg_capture_view_features*)
// share: the global pixel tile -> (view, pixel) mapping, the read of a view's record, and the view's ray.  One text, so that the K films and
// the K feature planes of a call see the same pixels through the same rays.
#pragma once
#include "shade.h"

namespace lg {

struct ViewPixel {
    uint32_t v, x, y;
    unsigned long long pix; // v * w * h + y * w + x: index into rgba (words) / rgb (x 3 doubles)
    bool active;
};
// global pixel tile G, lane -> the view and its pixel (pixel_of, mode 0, per film)
__device__ __forceinline__ ViewPixel view_pixel(const ViewArgs &Q, uint32_t G, uint32_t lane) {
    ViewPixel px;
    px.v = G / Q.tiles_per_view;
    const uint32_t t = G - px.v * Q.tiles_per_view;
    const uint32_t ty = t / Q.tiles_x, tx = t - ty * Q.tiles_x;
    px.x = tx * 8u + (lane & 7u);
    px.y = ty * 8u + (lane >> 3);
    px.active = px.x < Q.w && px.y < Q.h;
    px.pix = (unsigned long long)px.v * Q.w * Q.h + (unsigned long long)px.y * Q.w + px.x;
    return px;
}
// the view's record.  The table is written by a copy that is through before the launch starts and by nothing else: it is read through the
// constant address space, so that a wave-uniform v gives scalar loads and a per-lane v ordinary ones.
__device__ __forceinline__ DView view_load(const ViewArgs &Q, uint32_t v) {
    typedef const __attribute__((address_space(4))) double cdouble;
    typedef const __attribute__((address_space(4))) uint32_t cword;
    cdouble *p = (cdouble *)(uintptr_t)(Q.views + v);
    DView V;
    V.origin = V3{p[0], p[1], p[2]}; V.view = V3{p[3], p[4], p[5]}; V.up = V3{p[6], p[7], p[8]}; V.aux = V3{p[9], p[10], p[11]};
    V.image_plane_height = p[12]; V.pixel_separation = p[13]; V.ss_distance = p[14];
    V.ss_root = *(cword *)(p + 15); V.pad = 0u;
    return V;
}
// Camera::sample for sample `sidx` of pixel (x, y) of view V (camera.rs:113-146): camera_ray() of shade.h, the view's fields in the camera's place
__device__ __forceinline__ Ray view_ray(const DParams &P, const DView &V, uint32_t x, uint32_t y, uint32_t sidx) {
    double img_plane_height = V.image_plane_height;
    double img_plane_width = img_plane_height * P.aspect;
    double pixel_size = img_plane_height * P.hinv;
    double sample_separation = V.ss_distance * pixel_size;
    double sox = ((double)x * P.winv - 0.5) * img_plane_width;
    double soy = (0.5 - (double)(y + 1u) * P.hinv) * img_plane_height;
    V3 cam_o = V.origin + ((soy * V.pixel_separation) * V.up) + ((sox * V.pixel_separation) * V.aux);
    V3 cam_d = V.view + (soy * V.up) + (sox * V.aux);
    V3 updiff = V.up * sample_separation;
    V3 auxdiff = V.aux * sample_separation;
    V3 halfdiff = updiff * 0.5 + auxdiff * 0.5;
    const uint32_t dim = V.ss_root;
    uint32_t si = sidx / dim, sj = sidx % dim;
    V3 dd = cam_d + ((double)sj * updiff) + ((double)si * auxdiff) + halfdiff;
    return ray_new(cam_o, dd);
}

} // namespace lg
