// lasgun_amd/csrc/k_lens.hip -- lens rays (include/lasgun_hip.h, lg_lens_rays*): the rays of two cameras the reference does not have, an
// equirectangular panorama and an equidistant fisheye, generated on the device for lg_capture_rays* / lg_radiance* to walk.
//
// One ray per lane of a grid-stride loop, 48 bytes out as three 16-byte stores -- the shape of camera_rays_kernel (k_query.hip).  All of it
// is the lens's own arithmetic (an EXTRA: nothing of the reference is mirrored here), f64 with contraction off, the trigonometry trig.h's
// correctly rounded p_sincos / p_atan2.  The order of evaluation below is the one include/lasgun_hip.h states: it is the contract.
#include <hip/hip_runtime.h>

#include "dscene.h"
#include "trig.h"

namespace lg {

__global__ void __launch_bounds__(256) lens_rays_kernel(const DLens L, uint32_t w, uint32_t h, uint32_t root, const unsigned long long *offsets, unsigned long long n, double *rays) {
    const unsigned long long S = (unsigned long long)root * root, npix = (unsigned long long)w * h;
    const double PI_ = 3.141592653589793, TWO_PI = 6.283185307179586, RAD = 0.017453292519943295; // pi, 2 pi, pi / 180 as doubles
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long g = i / S;
        const uint32_t s = (uint32_t)(i - g * S), si = s / root, sj = s - si * root;
        const unsigned long long off = offsets ? offsets[g] : g;
        V3 o = vzero(), d = vzero();
        if (off < npix) {
            const uint32_t x = (uint32_t)(off % w), y = (uint32_t)(off / w);
            const double u = ((double)x + ((double)sj + 0.5) / (double)root) / (double)w;
            const double v = ((double)y + ((double)si + 0.5) / (double)root) / (double)h;
            o = L.origin;
            if (L.kind == 0) { // equirectangular
                const double phi = (u - 0.5) * TWO_PI, theta = (0.5 - v) * PI_;
                double sp, cp, st, ct;
                p_sincos(phi, sp, cp);
                p_sincos(theta, st, ct);
                d = ((ct * sp) * L.right + st * L.up) + (ct * cp) * L.forward;
            } else { // equidistant fisheye
                const uint32_t m = w < h ? w : h;
                const double a = (2.0 * u - 1.0) * ((double)w / (double)m), b = (1.0 - 2.0 * v) * ((double)h / (double)m);
                const double r = sqrt(a * a + b * b), psi = p_atan2(b, a), theta = r * ((L.fov_deg * 0.5) * RAD);
                double sp, cp, st, ct;
                p_sincos(psi, sp, cp);
                p_sincos(theta, st, ct);
                d = st * (cp * L.right + sp * L.up) + ct * L.forward;
            }
        }
        double2 *out = reinterpret_cast<double2 *>(rays + 6ull * i);
        out[0] = make_double2(o.x, o.y); out[1] = make_double2(o.z, d.x); out[2] = make_double2(d.y, d.z);
    }
}

hipError_t launch_lens_rays(const DLens &L, uint32_t w, uint32_t h, uint32_t root, const unsigned long long *offsets, unsigned long long n, double *rays,
                            uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(lens_rays_kernel, dim3(blocks), dim3(256), 0, stream, L, w, h, root, offsets, n, rays);
    return hipGetLastError();
}

} // namespace lg
