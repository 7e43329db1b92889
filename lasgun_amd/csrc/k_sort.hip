// lasgun_amd/csrc/k_sort.hip -- the opt-in ray order of a query (include/lasgun_hip.h, lg_accel_set_query_order / lg_query_order*): every
// ray gets a 32-bit coherence key (raykey.h) and the (key, index) pairs are sorted by a stable least-significant-digit radix sort, 8 bits
// a pass.  What comes out is perm[s] = the ray walked in slot s -- the stable ascending sort of the keys, so a pure function of the rays.
//
// A pass cuts the n elements into `nblocks` contiguous chunks of 256 * items elements, one per 256-lane workgroup, and is four kernels:
//   sort_hist_kernel     per chunk, how many of its elements carry each digit            -> hist[digit * nblocks + chunk]
//   sort_tile_sum_kernel, sort_scan_kernel  exclusive prefix sum over hist in that (digit-major) order: where chunk c's elements of digit d start
//   sort_scatter_kernel  per chunk again, 256 elements a round in element order: an element's place is its digit's running offset, plus the
//                        elements of that digit in the waves before it (one count per wave and digit, in LDS), plus those in the lanes
//                        below it (eight ballots match the digit, mbcnt counts the lanes below: k_wavefront.hip, wave_append)
// Elements of one digit keep their order in every pass: that is what makes LSD passes compose, and perm deterministic.
// The first pass reads no index array (an element's index is its position), the last one writes no keys (nobody reads them).
// Plain vector stores and atomicAdd on LDS words only.
#include <hip/hip_runtime.h>

#include "raykey.h"

namespace lg {

constexpr uint32_t SORT_BLOCK = 256u, SORT_DIGITS = 256u, SORT_WAVES = SORT_BLOCK / 64u;
static_assert(SORT_BLOCK == SORT_DIGITS, "one lane per digit where a workgroup reads or writes a histogram");

__device__ __forceinline__ uint32_t sort_lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// keys[i] = ray i's key.  A ray is 48 bytes, read as three 16-byte loads (as k_query.hip reads it)
__global__ void __launch_bounds__(SORT_BLOCK) sort_key_kernel(const double *rays, unsigned long long n, uint32_t *keys, const KeyBounds B) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * SORT_BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * SORT_BLOCK) {
        const double2 *r = reinterpret_cast<const double2 *>(rays + 6ull * i);
        const double2 a = r[0], b = r[1], c = r[2];
        const double v[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
        keys[i] = ray_key(v, B);
    }
}

__global__ void __launch_bounds__(SORT_BLOCK) sort_hist_kernel(const uint32_t *keys, unsigned long long n, uint32_t shift, uint32_t items,
                                                               uint32_t *hist, uint32_t nblocks) {
    __shared__ uint32_t h[SORT_DIGITS];
    const uint32_t tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const unsigned long long start = (unsigned long long)blockIdx.x * SORT_BLOCK * items;
    for (uint32_t r = 0; r < items; ++r) {
        const unsigned long long i = start + (unsigned long long)r * SORT_BLOCK + tid;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & (SORT_DIGITS - 1u)], 1u);
    }
    __syncthreads();
    hist[(size_t)tid * nblocks + blockIdx.x] = h[tid];
}

// The scan, in tiles of 4,096 counts (a workgroup; 16 consecutive counts a lane, read and written as four 16-byte units): a first kernel
// leaves every tile's sum, the second adds up the sums of the tiles before its own (at most 128 of them: total = 256 * nblocks <= 2^19
// counts) and writes its counts' exclusive prefixes back in place.  The counts add up to n < 2^32.
constexpr uint32_t SCAN_PER = 16u, SCAN_TILE = SORT_BLOCK * SCAN_PER;
// exclusive prefix of v over the workgroup's 256 lanes; *all = the workgroup's sum.  `lds` is free again after the call.
__device__ __forceinline__ uint32_t sort_block_scan(uint32_t v, uint32_t *lds, uint32_t tid, uint32_t *all) {
    lds[tid] = v;
    __syncthreads();
    for (uint32_t d = 1u; d < SORT_BLOCK; d <<= 1) {
        const uint32_t add = tid >= d ? lds[tid - d] : 0u;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[tid];
    *all = lds[SORT_BLOCK - 1u];
    __syncthreads();
    return incl - v;
}
__device__ __forceinline__ void sort_scan_load(const uint32_t *hist, uint32_t total, uint32_t at, uint32_t c[SCAN_PER]) {
    const uint4 *src = reinterpret_cast<const uint4 *>(hist + at);
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER / 4u; ++k) {
        const uint4 q = at < total ? src[k] : make_uint4(0u, 0u, 0u, 0u); // (total is a multiple of 256: a lane's 16 counts are all there or none)
        c[4u * k] = q.x; c[4u * k + 1u] = q.y; c[4u * k + 2u] = q.z; c[4u * k + 3u] = q.w;
    }
}
__global__ void __launch_bounds__(SORT_BLOCK) sort_tile_sum_kernel(const uint32_t *hist, uint32_t total, uint32_t *tile_sum) {
    __shared__ uint32_t lds[SORT_BLOCK];
    const uint32_t tid = threadIdx.x;
    uint32_t c[SCAN_PER], sum = 0u, all = 0u;
    sort_scan_load(hist, total, blockIdx.x * SCAN_TILE + tid * SCAN_PER, c);
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; ++k) sum += c[k];
    (void)sort_block_scan(sum, lds, tid, &all);
    if (tid == 0u) tile_sum[blockIdx.x] = all;
}
__global__ void __launch_bounds__(SORT_BLOCK) sort_scan_kernel(uint32_t *hist, uint32_t total, const uint32_t *tile_sum) {
    __shared__ uint32_t lds[SORT_BLOCK];
    const uint32_t tid = threadIdx.x, at = blockIdx.x * SCAN_TILE + tid * SCAN_PER;
    uint32_t before = 0u, all = 0u;
    (void)sort_block_scan(tid < blockIdx.x ? tile_sum[tid] : 0u, lds, tid, &before); // (gridDim.x <= 128 < 256 lanes)
    uint32_t c[SCAN_PER], sum = 0u;
    sort_scan_load(hist, total, at, c);
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER; ++k) sum += c[k];
    uint32_t run = before + sort_block_scan(sum, lds, tid, &all);
    if (at >= total) return;
    uint4 *dst = reinterpret_cast<uint4 *>(hist + at);
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER / 4u; ++k) {
        uint4 q;
        q.x = run; run += c[4u * k];
        q.y = run; run += c[4u * k + 1u];
        q.z = run; run += c[4u * k + 2u];
        q.w = run; run += c[4u * k + 3u];
        dst[k] = q;
    }
}

// idx_in == nullptr: the first pass, an element's index is its position; keys_out == nullptr: the last pass
__global__ void __launch_bounds__(SORT_BLOCK) sort_scatter_kernel(const uint32_t *keys_in, const uint32_t *idx_in, uint32_t *keys_out, uint32_t *idx_out,
                                                                  unsigned long long n, uint32_t shift, uint32_t items, const uint32_t *offsets,
                                                                  uint32_t nblocks) {
    __shared__ uint32_t base[SORT_DIGITS];             // where this chunk's next element of each digit goes
    __shared__ uint32_t wcnt[SORT_WAVES][SORT_DIGITS]; // this round: elements of each digit in each wave
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    base[tid] = offsets[(size_t)tid * nblocks + blockIdx.x];
    const unsigned long long start = (unsigned long long)blockIdx.x * SORT_BLOCK * items;
    for (uint32_t r = 0; r < items; ++r) {
        const unsigned long long i = start + (unsigned long long)r * SORT_BLOCK + tid;
        if (start + (unsigned long long)r * SORT_BLOCK >= n) break; // (uniform: the whole round is past the end)
        const bool valid = i < n;
        const uint32_t key = valid ? keys_in[i] : 0u;
        const uint32_t id = valid ? (idx_in ? idx_in[i] : (uint32_t)i) : 0u;
        const uint32_t digit = (key >> shift) & (SORT_DIGITS - 1u);
#pragma unroll
        for (uint32_t w = 0; w < SORT_WAVES; ++w) wcnt[w][tid] = 0u;
        __syncthreads(); // (also: base[] of the round before is written)
        unsigned long long same = __builtin_amdgcn_ballot_w64(valid); // the valid lanes of this wave with this lane's digit
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t below = sort_lanes_below(same);
        if (valid && below == 0u) wcnt[wave][digit] = (uint32_t)__builtin_popcountll(same); // one writer per wave and digit
        __syncthreads();
        if (valid) {
            uint32_t at = base[digit] + below;
            for (uint32_t w = 0; w < wave; ++w) at += wcnt[w][digit];
            if (keys_out) keys_out[at] = key;
            idx_out[at] = id;
        }
        __syncthreads();
        uint32_t round = 0u;
#pragma unroll
        for (uint32_t w = 0; w < SORT_WAVES; ++w) round += wcnt[w][tid];
        base[tid] += round;
    }
}

// ---- host-callable launchers (query.cpp)
// Chunks of a pass over n elements: at most SORT_MAX_BLOCKS of them, each a whole number of 256-element rounds
constexpr uint32_t SORT_MAX_BLOCKS = 2048u, SORT_MIN_ITEMS = 4u, SORT_MAX_TILES = SORT_DIGITS * SORT_MAX_BLOCKS / SCAN_TILE;
static_assert(SORT_MAX_TILES <= SORT_BLOCK, "sort_scan_kernel adds the tile sums up with one lane per tile");
static uint32_t sort_items(unsigned long long n) {
    const unsigned long long per = (n + (unsigned long long)SORT_BLOCK * SORT_MAX_BLOCKS - 1ull) / ((unsigned long long)SORT_BLOCK * SORT_MAX_BLOCKS);
    return (uint32_t)(per < SORT_MIN_ITEMS ? SORT_MIN_ITEMS : per);
}
static uint32_t sort_blocks(unsigned long long n, uint32_t items) {
    return (uint32_t)((n + (unsigned long long)SORT_BLOCK * items - 1ull) / ((unsigned long long)SORT_BLOCK * items));
}
// bytes of scratch a sort of n rays needs: two key arrays and two index arrays (16 bytes a ray) and one histogram
size_t sort_scratch_bytes(unsigned long long n) {
    const size_t arr = ((size_t)n * sizeof(uint32_t) + 255u) & ~(size_t)255u;
    return 4u * arr + ((size_t)SORT_DIGITS * SORT_MAX_BLOCKS + SORT_MAX_TILES) * sizeof(uint32_t);
}
// Keys of `rays` into keys_out (or scratch where it is nullptr), then the sort; the permutation ends in perm_out (or scratch where it is
// nullptr) and *perm receives where.  1 <= n < 2^32; scratch holds sort_scratch_bytes(n); everything is enqueued on `stream`.
hipError_t launch_query_order(const double *rays, unsigned long long n, const KeyBounds &B, void *scratch, uint32_t *keys_out, uint32_t *perm_out,
                              const uint32_t **perm, uint32_t grid_cap, hipStream_t stream) {
    const size_t arr = ((size_t)n * sizeof(uint32_t) + 255u) & ~(size_t)255u;
    uint8_t *m = reinterpret_cast<uint8_t *>(scratch);
    uint32_t *ka = reinterpret_cast<uint32_t *>(m), *kb = reinterpret_cast<uint32_t *>(m + arr);
    uint32_t *ia = reinterpret_cast<uint32_t *>(m + 2u * arr), *ib = reinterpret_cast<uint32_t *>(m + 3u * arr);
    uint32_t *hist = reinterpret_cast<uint32_t *>(m + 4u * arr), *tile_sum = hist + (size_t)SORT_DIGITS * SORT_MAX_BLOCKS;
    uint32_t *k0 = keys_out ? keys_out : ka;
    const uint32_t kblocks = (uint32_t)std::min<unsigned long long>((n + SORT_BLOCK - 1ull) / SORT_BLOCK, grid_cap < 1u ? 1u : grid_cap);
    hipLaunchKernelGGL(sort_key_kernel, dim3(kblocks), dim3(SORT_BLOCK), 0, stream, rays, n, k0, B);
    const uint32_t items = sort_items(n), nblocks = sort_blocks(n, items);
    const uint32_t total = SORT_DIGITS * nblocks, tiles = (total + SCAN_TILE - 1u) / SCAN_TILE;
    constexpr uint32_t passes = (KEY_BITS + 7u) / 8u;
    const uint32_t *kin = k0, *iin = nullptr;
    const uint32_t *final_idx = nullptr;
    for (uint32_t p = 0; p < passes; ++p) {
        const bool last = p + 1u == passes;
        // the ping-pong: pass 0 -> B, pass 1 -> A, ...; the last pass's indices go where the caller (or the walk) reads them
        uint32_t *kout = last ? nullptr : (p & 1u) ? ka : kb;
        uint32_t *iout = last && perm_out ? perm_out : (p & 1u) ? ia : ib;
        hipLaunchKernelGGL(sort_hist_kernel, dim3(nblocks), dim3(SORT_BLOCK), 0, stream, kin, n, p * 8u, items, hist, nblocks);
        hipLaunchKernelGGL(sort_tile_sum_kernel, dim3(tiles), dim3(SORT_BLOCK), 0, stream, hist, total, tile_sum);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(tiles), dim3(SORT_BLOCK), 0, stream, hist, total, tile_sum);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3(nblocks), dim3(SORT_BLOCK), 0, stream, kin, iin, kout, iout, n, p * 8u, items, hist, nblocks);
        kin = kout; iin = iout; final_idx = iout;
    }
    *perm = final_idx;
    return hipGetLastError();
}

} // namespace lg
