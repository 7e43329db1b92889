// lasgun_amd/csrc/k_tri_frames.hip -- the frame table's build kernel (DTriFrame, dscene.h; tri_frames_host.h says which accels get records;
// DESIGN.md 3.2): one lane per record, run once at the accel build.
#include "shade.h"

namespace lg {

// A record is what resolve_hit + shade_frame make of a hit on triangle `tri` of mesh instance `accel` with every expression a ray enters
// left out -- made by the per-hit path's own text (walk.h: triangle_partials, chain_up; shade.h: frame_axes) on the operands the per-hit
// path reads, on the device that renders, under the same compiler flags: the same instructions, so the same bits.  The two variants are
// the chain walked for n = c and for n = -c, the two values face_forward(c, -lr.d) can return; nothing is argued about signs.
__global__ void __launch_bounds__(64) tri_frames_kernel(const DParams P, const DTriFrameJob *jobs, const uint32_t n, DTriFrame *out) {
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= n) return;
    const uint32_t accel = jobs[r].accel, tri = jobs[r].tri;
    const uint32_t *vi = P.tri_v + 3ull * tri;
    const V3 p0 = load_f3(P.vpos, vi[0]), p1 = load_f3(P.vpos, vi[1]), p2 = load_f3(P.vpos, vi[2]);
    V3 dpdu, dpdv;
    triangle_partials(P, tri, P.accels[accel].flags, p0, p1, p2, dpdu, dpdv);
    const V3 c = triangle_c(p0, p1, p2);
    DTriFrame f;
    f.c[0] = c.x; f.c[1] = c.y; f.c[2] = c.z;
    f.pad = 0u;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        Isect is;
        isect_set(is, 0.0, dpdu, dpdv);
        is.has_n = true;
        is.n = v ? -c : c;
        const int32_t mat = chain_up(P, accel, is);
        const FrameAxes ax = frame_axes(is);
        if (v == 0) { // (no n in them: the same for both variants)
            f.ng0[0] = ax.ng0.x; f.ng0[1] = ax.ng0.y; f.ng0[2] = ax.ng0.z;
            f.ss[0] = ax.ss.x; f.ss[1] = ax.ss.y; f.ss[2] = ax.ss.z;
            f.mat = mat;
        }
        f.ns[v][0] = ax.ns.x; f.ns[v][1] = ax.ns.y; f.ns[v][2] = ax.ns.z;
        f.ts[v][0] = ax.ts.x; f.ts[v][1] = ax.ts.y; f.ts[v][2] = ax.ts.z;
    }
    out[r] = f;
}

// P: the scene tables alone (accels, tri_v, tri_t, vpos, vtex, default_material)
hipError_t launch_tri_frames(const DParams &P, const DTriFrameJob *jobs, uint32_t n, DTriFrame *out, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(tri_frames_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, P, jobs, n, out);
    return hipGetLastError();
}

} // namespace lg
