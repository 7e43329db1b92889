// lasgun_amd/csrc/rq_closest_body.h -- the body of W1 of level 0 of a radiance query (k_radiance.hip), included once into each of its two
// kernels: rq_closest_kernel (Q: RadianceArgs, a finished ray goes to radiance[]) and rf_closest_kernel (Q: FilmArgs, it goes to a film);
// rq_finish is overloaded on Q.  The text level0.h's l0_closest_body was made from; this family keeps it (k_radiance.hip says why),
// and keeps it whole: over tilewalk.h's prologue and cursor three radiance and film rows measured slower (profiles/tilewalk_account.md).
// In scope: template parameters FAST, LDSS, PRUNE, PERM; kernel parameters P (DParams) and Q.
    static_assert(!(FAST && LDSS), "the LDS-resident scene holds the reference tree only");
    static_assert(!(FAST && PRUNE), "the fast mode prunes its own trees by its own rule");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t ntiles = P.ntiles;
    if (ntiles == 0u) return; // (uniform: before the LDS copy and its barrier)
    uint32_t *stack = lds_stack + tid;
    constexpr uint32_t stride = LDSS ? LG_LDSS_BLOCK : LG_BLOCK;
    const uint4 *scn = nullptr;
    if (LDSS) {
        uint4 *dst = reinterpret_cast<uint4 *>(lds_stack + P.stack_depth * stride);
        copy_to_lds(dst, reinterpret_cast<const uint4 *>(P.lds_image), P.lds_image_n16, tid, stride);
        __syncthreads(); // the only workgroup-wide step; every wave reaches it before pulling tiles
        scn = dst;
    }
    const uint4 *const arec = (LDSS || FAST) ? nullptr : load_accel_image(P, P.stack_depth * LG_BLOCK);
    Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0}; (void)cnt;
    if (!wave_has_work(ntiles)) return;
    uint32_t band = LDSS ? xcc_id() : 0u, bands_left = TILE_HEADS;
    for (bool final = false; !final;) {
        uint32_t tile;
        if (LDSS) tile = claim_tile(P.tile_counter, ntiles, band, bands_left, final);
        else tile = claim_tile_single(P.tile_counter, ntiles, final);
        if (tile == NO_TILE) break;
        const unsigned long long i = (unsigned long long)tile * 64ull + lane; // the chunk's work item: index of level 0's arrays
        const bool active = Q.base + i < Q.n;
        unsigned long long r = 0;
        Ray ray = ray_new(V3{0.0, 0.0, 0.0}, V3{0.0, 0.0, 1.0});
        if (active) {
            r = rq_ray_index<PERM>(Q, Q.base + i);
            ray = rq_load_ray(Q, r);
        }
        Best b;
        b.ref = NO_HIT; b.t = INFINITY; b.accel = 0u;
        if (active) walk<LDSS, FAST, PRUNE>(P, ray, false, stack, stride, b, scn, cnt, arec);
        const bool hit = active && b.ref != NO_HIT;
        // ---- this wave's slots in the level's hit queue (wflevel.h: dense where most lanes hit, appended otherwise)
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        const uint32_t nhit = (uint32_t)__builtin_popcountll(mask);
        unsigned long long h = i;
        if (nhit < WF_FULL_MIN) {
            P.wf_hq[i] = WF_NONE; // (every lane stands for slot i of the dense part, a ray or a slot past the last ray: the chunk's arrays hold whole tiles)
            if (nhit != 0u) {
                uint32_t base_v = 0u;
                if (lane == 0u) base_v = atomicAdd(P.wf_counts + P.wf_levels, nhit);
                h = P.wf_hit_cap + (uint32_t)__builtin_amdgcn_readfirstlane((int)base_v) + lanes_below(mask);
            }
        } else if (!hit) P.wf_hq[i] = WF_NONE; // a hole of a dense block
        if (hit) {
            // A bare ray index: bit 31 of this word is WF_SKIP to the shadow pass (wflevel.h, hit_of), which would then neither walk the hit nor write
            // its vis word.  i stays below 2^31 because a query's chunks come from the same ChunkPlan as a render's (launch.cpp: cap_limit,
            // 0x7FFFFFF0 rays for the level-by-level pipeline) -- raise that cap for queries and this store has to mask or flag like k_wavefront.hip's.
            P.wf_hq[h] = (uint32_t)i;
            Shade sh;
            shade_frame(P, ray, b, sh);
            const unsigned long long n = P.wf_hit_stride;
            double *f = P.frame + h;
            f[0 * n] = sh.praw.x; f[1 * n] = sh.praw.y; f[2 * n] = sh.praw.z;
            f[3 * n] = sh.ng.x; f[4 * n] = sh.ng.y; f[5 * n] = sh.ng.z;
            f[6 * n] = sh.ns.x; f[7 * n] = sh.ns.y; f[8 * n] = sh.ns.z;
            f[9 * n] = sh.ss.x; f[10 * n] = sh.ss.y; f[11 * n] = sh.ss.z;
            f[12 * n] = (double)sh.mat;
        } else if (active) { // integrate.rs:26-28
            const V3 value = background(P, normalize(ray.d));
            if (P.wf_levels == 1u) rq_finish(Q, r, value);
            else {
                const unsigned long long n = P.wf_cap;
                P.wf_out[i] = value.x; P.wf_out[n + i] = value.y; P.wf_out[2 * n + i] = value.z;
                P.wf_child[i] = WF_MISS;
            }
        }
    }
