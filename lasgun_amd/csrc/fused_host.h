// lasgun_amd/csrc/fused_host.h -- the gate of the fused form of the camera's level 0 (k_wavefront.hip, wf_trace_kernel<.., FUSED>; DESIGN.md
// 3.2), the part that touches no device.  Kept free of HIP: tools/fused_gate_check.cpp runs exactly this text under AddressSanitizer /
// UBSan on the CPU, launch.cpp calls it in WfChunk::run, lg_fused_shade_gate hands it to the tests.
//
// The fused form shades in the closest pass's epilogue and in the shadow pass's tail and launches no shade pass.  Its kernels hold
// li = (0 + [visible] term) + ambient for ONE light and finish the pixel with the camera's finish_pixel, so it is the form of exactly one
// chain: the scene camera's own level 0, when that is the chain's only level, with exactly one light, where the closest launch takes the
// packet form and the shadow launch the pair form.  Everything else keeps the three kernels.  Wrong means wrong pixels: every condition
// is stated, and each alone refuses.
#pragma once

namespace lg {

enum FusedRefusal : int {
    FUSED_OK = 0,
    FUSED_SWITCH_OFF = 1,   // lg_accel_set_fused_shade(0) / LASGUN_FUSED_SHADE=0
    FUSED_OWN_LEVEL0 = 2,   // level 0 is not the camera's: a radiance query, a gather, a view batch, light groups, lit scatter (their own passes)
    FUSED_LEVELS = 3,       // the chain has a level below (glass or a mirror with recursion): the shade pass makes the children
    FUSED_LIGHTS = 4,       // no light (no shadow pass to finish the pixels) or more than one
    FUSED_NOT_PACKET = 5,   // the closest launch does not take the packet form (packet_host.h: the scene graph, the pair image, its switch)
    FUSED_NOT_PAIRS = 6,    // the shadow launch does not take the pair form (wf_takes_pairs)
};

struct FusedAsk {
    bool switched_on;       // the accel's switch and the environment's
    bool camera_level0;     // the chain's level 0 is the scene camera's own (no Level0 source, no per-level planes)
    unsigned levels;        // levels of the chain (1: no recursion)
    unsigned long nlights;  // the scene's lights
    bool packet_closest;    // DParams::packet of the level-0 closest launch
    bool pair_shadow;       // wf_takes_pairs of the level-0 shadow launch
};

inline FusedRefusal fused_shade_gate(const FusedAsk &q) {
    if (!q.switched_on) return FUSED_SWITCH_OFF;
    if (!q.camera_level0) return FUSED_OWN_LEVEL0;
    if (q.levels != 1u) return FUSED_LEVELS;
    if (q.nlights != 1ul) return FUSED_LIGHTS;
    if (!q.packet_closest) return FUSED_NOT_PACKET;
    if (!q.pair_shadow) return FUSED_NOT_PAIRS;
    return FUSED_OK;
}

} // namespace lg
