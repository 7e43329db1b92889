// lasgun_amd/csrc/travform.h -- the host side that the tiled traversal kernels of the query family share (k_query.hip, k_radiance.hip's
// closest pass, k_visibility.hip, k_features.hip): ONE table of the (FAST, LDSS, PRUNE) forms a kernel family is compiled in -- the
// launcher, the occupancy figure and the dynamic-LDS limit all go through it, so a form that can be launched cannot be missing from
// the other two.  (A limit that misses a launched form fails only on a scene whose stacks plus image pass 64 KiB.)  The render's own
// kernels (k_wavefront.hip, k_mega.hip, k_queue.hip) have other form sets and do not use this.
#pragma once
#include <utility>

#include "shade.h"

namespace lg {

// A kernel file describes its family ONCE, as
//     template <bool FAST, bool LDSS, bool PRUNE> struct K { static constexpr int variants; static const void *kernel(int variant); };
// (the variants of a form: closest / any-hit, as given / permuted, ...) and gets the three operations below.
struct TravForm { bool fast, ldss, prune; };
constexpr TravForm TRAV_FORMS[] = {{true, false, false}, {false, true, true}, {false, false, true}, {false, true, false}, {false, false, false}};
constexpr size_t TRAV_NFORMS = sizeof TRAV_FORMS / sizeof TRAV_FORMS[0];

template <template <bool, bool, bool> class K, size_t... I> const void *trav_kernel(size_t form, int variant, std::index_sequence<I...>) {
    const void *(*const of[])(int) = {&K<TRAV_FORMS[I].fast, TRAV_FORMS[I].ldss, TRAV_FORMS[I].prune>::kernel...};
    return of[form](variant);
}
template <template <bool, bool, bool> class K> const void *trav_kernel(size_t form, int variant) {
    return trav_kernel<K>(form, variant, std::make_index_sequence<TRAV_NFORMS>());
}
// the form a launch takes: fast mode has one, the reference walk is pruned or not, with the scene in LDS or not
constexpr size_t trav_form(bool fast, bool ldss, bool prune) {
    size_t f = 0;
    while (f < TRAV_NFORMS && !(TRAV_FORMS[f].fast == fast && TRAV_FORMS[f].ldss == (ldss && !fast) && TRAV_FORMS[f].prune == (prune && !fast))) ++f;
    return f;
}
constexpr bool trav_forms_complete() {
    for (int m = 0; m < 8; ++m)
        if (trav_form(m & 1, m & 2, m & 4) >= TRAV_NFORMS) return false;
    return true;
}
static_assert(trav_forms_complete(), "TRAV_FORMS misses a form that some (fast, ldss, prune) selects: trav_kernel would index past its table");
// Dynamic LDS of a traversal launch: the per-lane stacks (`stack_depth` words in fast mode, P.stack_depth otherwise) and behind them the
// scene image (1024-lane workgroups) or the accel records (256-lane workgroups, reference walk)
inline size_t trav_lds_bytes(const DParams &P, bool fast, uint32_t stack_depth) {
    const bool ldss = P.lds_image && !fast;
    const uint32_t block = ldss ? LG_LDSS_BLOCK : LG_BLOCK, depth = fast ? stack_depth : P.stack_depth;
    return (size_t)depth * block * sizeof(uint32_t) + (ldss ? (size_t)P.lds_image_n16 * 16u : (!fast && P.accel_image ? (size_t)P.accel_image_n16 * 16u : 0u));
}
// launch the form that (fast, P.lds_image, P.prune) selects, in `variant`; args: the kernel's parameters in order
template <template <bool, bool, bool> class K>
hipError_t trav_launch(const DParams &P, bool fast, int variant, uint32_t blocks, uint32_t stack_depth, void **args, hipStream_t stream) {
    const bool ldss = P.lds_image && !fast;
    (void)hipLaunchKernel(trav_kernel<K>(trav_form(fast, ldss, P.prune != 0u), variant), dim3(blocks), dim3(ldss ? LG_LDSS_BLOCK : LG_BLOCK), args,
                          trav_lds_bytes(P, fast, stack_depth), stream);
    return hipGetLastError();
}
// workgroups per CU of the 256-lane form P takes (P without an LDS-resident scene): the least over its variants
template <template <bool, bool, bool> class K> hipError_t trav_occupancy(const DParams &P, bool fast, uint32_t stack_depth, int *blocks_per_cu) {
    const size_t form = trav_form(fast, false, P.prune != 0u), lds = trav_lds_bytes(P, fast, stack_depth);
    for (int v = 0; v < K<false, false, false>::variants; ++v) {
        int n = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trav_kernel<K>(form, v), LG_BLOCK, lds);
        if (e != hipSuccess) return e;
        if (v == 0 || n < *blocks_per_cu) *blocks_per_cu = n;
    }
    return hipSuccess;
}
// raise the dynamic-LDS limit of every variant of every form with this LDSS to `bytes`
template <template <bool, bool, bool> class K> hipError_t trav_set_lds_limit(size_t bytes, bool ldss) {
    for (size_t f = 0; f < TRAV_NFORMS; ++f)
        for (int v = 0; TRAV_FORMS[f].ldss == ldss && v < K<false, false, false>::variants; ++v) {
            const hipError_t e = hipFuncSetAttribute(trav_kernel<K>(f, v), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

} // namespace lg
