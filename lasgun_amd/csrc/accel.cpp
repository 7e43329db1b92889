// lasgun_amd/csrc/accel.cpp -- Accel::from (src/accelerators/bvh.rs:135-202 on the host, host.cpp) as device tables: flatten, the LDS images,
// grids and budgets from the device's occupancy, one upload; and the tables once more with what was left out of them (fast trees, leaf records).
#include "internal.h"
#include "attributes_host.h"
#include "pairs_host.h"
#include "tri_frames_host.h"

// What a record of lg_hit_attributes_of* may name (attributes_host.h, the counts table): a mesh accel's faces are its OBJ's (lg_hit::prim of
// a triangle is the face number), and the leaves of a group's reference tree hold its spheres and boxes -- each sits in that group and in
// no other.  A mesh's tree is not walked.
static std::vector<uint32_t> attr_counts_of(const FlatScene &f, const Scene &scene) {
    std::vector<uint32_t> faces(f.accels.size(), 0u), tri_base(f.accels.size(), 0u), sphere_accel(f.spheres.size(), NO_HIT), cuboid_accel(f.cuboids.size(), NO_HIT);
    std::vector<uint32_t> todo;
    for (size_t id = 0; id < f.accels.size(); ++id) {
        const DAccel &A = f.accels[id];
        if (A.flags & AF_MESH) {
            const int64_t obj = id < f.accel_obj.size() ? f.accel_obj[id] : -1;
            if (obj >= 0 && (size_t)obj < scene.meshes.size() && scene.meshes[(size_t)obj]) faces[id] = (uint32_t)(scene.meshes[(size_t)obj]->tri.size() / 3);
            tri_base[id] = id < f.accel_tri_base.size() ? f.accel_tri_base[id] : 0u;
            if ((size_t)tri_base[id] + faces[id] > f.tri_v.size() / 3) faces[id] = 0u; // (never past the triangle tables)
            continue;
        }
        if (A.node_base >= f.nodes.size()) continue; // (an empty group has no tree)
        todo.assign(1, 0u);
        while (!todo.empty()) {
            const uint32_t nidx = todo.back();
            todo.pop_back();
            const DNode &nd = f.nodes[A.node_base + nidx];
            if (!(nd.meta & NODE_LEAF)) { todo.push_back(nidx + 1u); todo.push_back(nd.link); continue; }
            for (uint32_t k = 0; k < (nd.meta & 0xFFFFu); ++k) {
                const uint32_t ref = f.primref[(size_t)A.prim_base + nd.link + k], kind = ref >> 30, idx = ref & PRIM_INDEX_MASK;
                if (kind == PK_SPHERE && idx < sphere_accel.size()) sphere_accel[idx] = (uint32_t)id;
                else if (kind == PK_CUBOID && idx < cuboid_accel.size()) cuboid_accel[idx] = (uint32_t)id;
            }
        }
    }
    return attr_counts_build(faces, tri_base, sphere_accel, cuboid_accel);
}

// The frame table's plan for a flattened scene (tri_frames_host.h), without a device: every accel as the plan sees it -- a mesh instance's
// triangles are its OBJ's faces, from its mesh's first triangle on -- and the plan itself: base[a] per accel, the records returned.
static std::vector<TriFramesAccel> tri_frames_accels(const FlatScene &f, const Scene &scene) {
    std::vector<TriFramesAccel> t(f.accels.size());
    for (size_t id = 0; id < f.accels.size(); ++id) {
        t[id] = TriFramesAccel{f.accels[id].flags, id < f.accel_tri_base.size() ? f.accel_tri_base[id] : 0u, 0u};
        const int64_t obj = id < f.accel_obj.size() ? f.accel_obj[id] : -1;
        if ((f.accels[id].flags & AF_MESH) && obj >= 0 && (size_t)obj < scene.meshes.size() && scene.meshes[(size_t)obj])
            t[id].faces = (uint32_t)std::min<size_t>(scene.meshes[(size_t)obj]->tri.size() / 3, 0xFFFFFFFFu);
    }
    return t;
}
uint32_t scene_tri_frames(const FlatScene &f, const Scene &scene, std::vector<uint32_t> &base) {
    const std::vector<TriFramesAccel> t = tri_frames_accels(f, scene);
    base.assign(t.size(), NO_HIT);
    return tri_frames_plan(t.data(), t.size(), f.tri_v.size() / 3, base.data());
}

// raise the dynamic-LDS limit of the traversal kernels of EVERY kernel file (ldss: their LDS-resident-scene forms; otherwise the 256-lane
// forms): a kernel file with such kernels adds itself here
static void set_lds_limits(size_t bytes, bool ldss) {
    for (auto set : {mega_set_lds_limit, wf_set_lds_limit, queue_set_lds_limit, query_set_lds_limit, rq_set_lds_limit, visibility_set_lds_limit, features_set_lds_limit,
                     open_directions_set_lds_limit, range_scan_set_lds_limit, hit_layers_set_lds_limit, trace_paths_set_lds_limit, gather_set_lds_limit, view_set_lds_limit, view_features_set_lds_limit, light_groups_set_lds_limit, scatter_set_lds_limit, lit_set_lds_limit, attributes_set_lds_limit})
        HIP_TRY(set(bytes, ldss));
}

// The LDS-resident scene image of a flattened scene (a->flat; a->stack_depth, a->node_pairs and a->prune say which): the image's words into
// `img`, the compact bases into the accel records of a->flat, the offsets, ranges and form into `a`.  Touches no device (lg_scene_lds_image
// calls it for a scene alone).  false: the tables do not fit beside the stacks.
constexpr size_t LDS_MAX = 160 * 1024;
static bool make_lds_image(lg_accel *a, size_t big_mesh_tris, std::vector<uint32_t> &img) {
    static const bool times = std::getenv("LASGUN_DEBUG_TIMES") != nullptr;
    a->lds_image_n16 = 0; a->lds_pairs = false; a->pair_refusal.clear(); a->pair_rel.clear();
    {
        {
            FlatScene &fm = a->flat;
            std::vector<uint32_t> nb, pb; // start offsets of every tree / primref run, both kinds
            for (const DAccel &A : fm.accels) { nb.push_back(A.node_base); nb.push_back(A.fnode_base); pb.push_back(A.prim_base); pb.push_back(A.fprim_base); }
            std::sort(nb.begin(), nb.end()); nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
            std::sort(pb.begin(), pb.end()); pb.erase(std::unique(pb.begin(), pb.end()), pb.end());
            auto extent = [](const std::vector<uint32_t> &starts, uint32_t b, size_t total) {
                auto it = std::upper_bound(starts.begin(), starts.end(), b);
                return (uint32_t)((it == starts.end() ? total : (size_t)*it) - b);
            };
            std::vector<std::pair<uint32_t, uint32_t>> nruns, pruns; // (global base, compact base) of each reference tree, once
            uint32_t nn = 0, np = 0;
            // compact numbering: the non-mesh accels first (their slots get a leaf record in the image), then the meshes
            uint32_t np_soup = 0; // slots of the non-mesh accels
            const size_t stack_bytes = (size_t)a->stack_depth * 1024 * 4; // per-lane stacks of the private walks
            const size_t accel16 = fm.accels.size() * LDS_ACCEL_UNITS;
            // image: [nodes, LDS_NODE_STRIDE units each][primrefs][leaf records, 3 units per slot][accel records]
            // `own_trees`: every accel gets node records of its own -- instances of one mesh (the five walls of the Cornell shell are one
            // two-triangle plane) otherwise share a tree, and the level-0 closest pass's origin-relative form (k_wavefront.hip, l0_rewrite)
            // rewrites a tree relative to ITS accel's local origin, which differs from instance to instance.  Same records, same walk words
            // up to each copy's own base; the primrefs stay shared (a mesh's slots are triangles: never rewritten).
            auto number = [&](bool own_trees) {
                nruns.clear(); pruns.clear(); nn = np = np_soup = 0;
                for (int pass = 0; pass < 2; ++pass) {
                  if (pass == 1) np_soup = np;
                  for (DAccel &A : fm.accels) {
                    if (((A.flags & AF_MESH) != 0u) != (pass == 1)) continue;
                    auto fn = own_trees ? nruns.end() : std::find_if(nruns.begin(), nruns.end(), [&](auto &r) { return r.first == A.node_base; });
                    if (fn == nruns.end()) { nruns.emplace_back(A.node_base, nn); A.lnode_base = nn; nn += extent(nb, A.node_base, fm.nodes.size()); }
                    else A.lnode_base = fn->second;
                    auto fp = std::find_if(pruns.begin(), pruns.end(), [&](auto &r) { return r.first == A.prim_base; });
                    if (fp == pruns.end()) { pruns.emplace_back(A.prim_base, np); A.lprim_base = np; np += extent(pb, A.prim_base, fm.primref.size()); }
                    else A.lprim_base = fp->second;
                  }
                }
                return (size_t)nn * LDS_NODE_STRIDE + ((size_t)np + 3) / 4 + (size_t)np_soup * 3 + accel16;
            };
            size_t n16 = number(false);
            // The copies are paid by every launch of every LDS-resident kernel (each workgroup copies the image once per launch), so they are
            // made only where they are small change: at most 1/16 on top of the shared image, and only for a scene the form can serve at all.
            if (fm.accels.size() <= L0_REL_MAX_ACCELS && nruns.size() < fm.accels.size()) {
                const size_t shared16 = n16, own16 = number(true);
                if (stack_bytes + own16 * 16 > LDS_MAX || (own16 - shared16) * 16 > shared16) n16 = number(false);
                else n16 = own16;
            }
            const size_t prim16 = ((size_t)np + 3) / 4;
            a->l0_rel.clear();
            if (stack_bytes + n16 * 16 <= LDS_MAX) {
                img.assign(n16 * 4, 0u);
                a->lds_node_off = 0;
                for (auto &r : nruns)
                    for (uint32_t i = 0, e = extent(nb, r.first, fm.nodes.size()); i < e; ++i) {
                        uint32_t *rec = &img[((size_t)(r.second + i) * LDS_NODE_STRIDE) * 4];
                        std::memcpy(rec, &fm.nodes[r.first + i], 56);
                    }
                a->lds_prim_off = nn * LDS_NODE_STRIDE;
                a->lds_soup_off = a->lds_prim_off + (uint32_t)prim16;
                for (auto &r : pruns)
                    for (uint32_t i = 0, e = extent(pb, r.first, fm.primref.size()); i < e; ++i) {
                        img[(size_t)a->lds_prim_off * 4 + r.second + i] = fm.primref[r.first + i];
                        if (r.second + i < np_soup)
                            std::memcpy(&img[((size_t)a->lds_soup_off + (size_t)(r.second + i) * 3) * 4], &fm.leaf_soup[r.first + i], 48);
                    }
                // walk words of every record (words 16..19; walk.h, traverse_ref): the second formulation of the reference walk
                // addresses nodes by their byte offset in the image and takes a leaf's slot range ready-made
                for (const DAccel &A : fm.accels) {
                    const uint32_t tree0 = a->lds_node_off * 16u + A.lnode_base * LDS_NODE_STRIDE * 16u;
                    for (uint32_t i = 0, e = extent(nb, A.node_base, fm.nodes.size()); i < e; ++i) {
                        uint32_t *rec = &img[((size_t)(A.lnode_base + i) * LDS_NODE_STRIDE) * 4];
                        const DNode &nd = fm.nodes[A.node_base + i];
                        if (nd.meta & NODE_LEAF) { rec[16] = A.lprim_base + nd.link; rec[17] = NODE_LEAF; rec[18] = rec[16] + (nd.meta & 0xFFFFu); rec[19] = nd.pad; }
                        else { rec[16] = tree0 + nd.link * LDS_NODE_STRIDE * 16u; rec[17] = 1u << (nd.meta & 3u); rec[18] = 0u; }
                        rec[17] |= nd.meta & NODE_NOPRUNE;
                    }
                }
                a->lds_accel_off = a->lds_soup_off + np_soup * 3u;
                for (size_t i = 0; i < fm.accels.size(); ++i) {
                    const DAccel &A = fm.accels[i];
                    uint32_t *rec = &img[((size_t)a->lds_accel_off + i * LDS_ACCEL_UNITS) * 4];
                    std::memcpy(rec, &A.minv, 96);
                    rec[24] = a->lds_node_off * 16u + A.lnode_base * LDS_NODE_STRIDE * 16u;
                    rec[25] = A.lprim_base; rec[26] = A.prim_base - A.lprim_base; rec[27] = A.flags;
                    rec[28] = (uint32_t)A.parent; rec[29] = A.nchain; rec[30] = A.lone;
                    for (int k = 0; k < MAX_CHAIN; ++k) rec[32 + k] = A.chain[k];
                    std::memcpy(rec + 40, A.prune, sizeof A.prune);
                    std::memcpy(rec + LDS_ACCEL_DOOR * 4, A.door, sizeof A.door);
                }
                // the origin-relative form's ranges (DRelAccel): offered only when no record would be rewritten for two accels
                if (fm.accels.size() <= L0_REL_MAX_ACCELS) {
                    bool own = true;
                    for (size_t i = 0; i < fm.accels.size(); ++i)
                        for (size_t j = 0; j < i; ++j) {
                            const DAccel &A = fm.accels[i], &B = fm.accels[j];
                            own = own && A.lnode_base != B.lnode_base && (((A.flags | B.flags) & AF_MESH) != 0u || A.lprim_base != B.lprim_base);
                        }
                    for (const DAccel &A : fm.accels) {
                        DRelAccel r{};
                        r.node_off = a->lds_node_off * 16u + A.lnode_base * LDS_NODE_STRIDE * 16u;
                        r.node_n = extent(nb, A.node_base, fm.nodes.size());
                        r.slot0 = A.lprim_base;
                        r.slot_n = (A.flags & AF_MESH) ? 0u : extent(pb, A.prim_base, fm.primref.size());
                        own = own && (size_t)r.node_off + (size_t)r.node_n * LDS_NODE_STRIDE * 16u <= (size_t)a->lds_prim_off * 16u && r.slot0 + r.slot_n <= np_soup;
                        a->l0_rel.push_back(r);
                    }
                    if (!own) a->l0_rel.clear();
                }
                // The pair form of the image (pairs_host.h; walk.h, traverse_ref<.., PAIR>), made IN PLACE of the node form where the switch asks for it
                // (lg_accel_set_node_pairs, LASGUN_NODE_PAIRS; not beside the REFILL experiment, which reads node records): [pair records of
                // every tree][root records][primrefs][leaf records][accel records] -- everything behind the node records copied as it is, the
                // accel records' unit [6].x pointing at the tree's root record.  2 * pairs + roots == node records (pair_size_ok): the pair
                // records hold the 56 payload bytes of every node record but the roots', so the image grows by nothing but the root records
                // (and shrinks against the 80-byte LDS node records).  A tree whose slot ranges do not fit a child word, or instances of one
                // tree with different slot bases: the node form stays, and pair_refusal says why (LASGUN_DEBUG_TIMES prints it).
                static const bool pairs_env = env_on("LASGUN_NODE_PAIRS");
                static const bool refill_env = [] { const char *e = std::getenv("LASGUN_REFILL"); return e && e[0] == '1'; }();
                // (an accel whose renders take the pruned walk keeps the node form, which that walk reads from LDS; lg_accel_set_prune(1) on an accel
                // that holds pair records sends its pruned launches to the L2 tables instead: internal.h, lds_resident)
                const int prune_set = a->image_prune != -2 ? a->image_prune : a->prune;
                const bool pruned_now = prune_set < 0 ? (prune_env() < 0 ? big_mesh_tris >= PRUNE_MIN_TRIS : prune_env() != 0) : prune_set != 0;
                if (a->node_pairs && pairs_env && !refill_env && !pruned_now) {
                    std::vector<uint32_t> run_pair(nruns.size(), 0u), run_n(nruns.size(), 0u), run_lprim(nruns.size(), 0u); // first pair record of each tree, its pair records, its slot base
                    size_t pairs = 0;
                    for (size_t r = 0; r < nruns.size(); ++r) {
                        run_pair[r] = (uint32_t)pairs;
                        run_n[r] = (uint32_t)pair_interior_count(&fm.nodes[nruns[r].first], extent(nb, nruns[r].first, fm.nodes.size()));
                        pairs += run_n[r];
                    }
                    const size_t pair16 = pairs * (PAIR_REC_BYTES / 16u), root16 = nruns.size() * (PAIR_ROOT_BYTES / 16u), tail16 = n16 - a->lds_prim_off;
                    const size_t p16 = pair16 + root16 + tail16;
                    std::vector<uint32_t> pimg(p16 * 4, 0u);
                    std::string why;
                    bool ok = pair_size_ok(pairs, nruns.size(), nn) && stack_bytes + p16 * 16 <= LDS_MAX;
                    if (!ok) why = "the trees are not binary, or the pair form does not fit beside the stacks";
                    std::memcpy(&pimg[(pair16 + root16) * 4], &img[(size_t)a->lds_prim_off * 4], tail16 * 16);
                    const uint32_t shift = (uint32_t)(pair16 + root16) - a->lds_prim_off; // what every offset behind the node records moves by (mod 2^32)
                    std::vector<bool> built(nruns.size(), false);
                    for (size_t i = 0; ok && i < fm.accels.size(); ++i) {
                        const DAccel &A = fm.accels[i];
                        const size_t r = (size_t)(std::find_if(nruns.begin(), nruns.end(), [&](auto &q) { return q.second == A.lnode_base; }) - nruns.begin());
                        if (r >= nruns.size()) { ok = false; why = "an accel without a tree in the image"; break; }
                        const size_t pair_off = (size_t)run_pair[r] * PAIR_REC_BYTES, root_off = pair16 * 16u + r * PAIR_ROOT_BYTES;
                        if (!built[r]) {
                            ok = pair_build_tree(&fm.nodes[nruns[r].first], extent(nb, nruns[r].first, fm.nodes.size()), A.lprim_base, pair_off, root_off,
                                                 reinterpret_cast<unsigned char *>(pimg.data()), (pair16 + root16) * 16u, &why);
                            built[r] = true; run_lprim[r] = A.lprim_base;
                        } else if (run_lprim[r] != A.lprim_base) { ok = false; why = "instances of one tree with different slot bases"; } // (a leaf word carries absolute slots)
                        pimg[((size_t)(a->lds_accel_off + shift) + i * LDS_ACCEL_UNITS) * 4 + 24] = (uint32_t)root_off;
                        a->pair_rel.push_back({(uint32_t)root_off, (uint32_t)pair_off, run_n[r]});
                    }
                    if (ok) {
                        a->lds_prim_off += shift; a->lds_soup_off += shift; a->lds_accel_off += shift;
                        img.swap(pimg); n16 = p16;
                        a->lds_pairs = true;
                    } else {
                        a->pair_rel.clear(); a->pair_refusal = why;
                        if (times) std::fprintf(stderr, "[lasgun] accel build: no pair form of the LDS image (%s): the node form serves every kernel\n", why.c_str());
                    }
                }
                a->lds_image_n16 = (uint32_t)n16;
                return true;
            }
        }
    }
    return false;
}
// the image builder for a scene alone (lg_scene_lds_image): what lg_accel_from would copy into LDS, without a device
bool scene_lds_image(const Scene &scene, bool pairs, std::vector<uint32_t> &img, uint32_t info[8]) {
    lg_accel a;
    a.scene = &scene;
    a.node_pairs = pairs;
    a.prune = 0;
    flatten_scene(scene, a.flat, false, false);
    a.stack_depth = a.flat.max_stack + 2;
    if (!make_lds_image(&a, 0, img)) return false;
    info[0] = a.lds_image_n16; info[1] = a.lds_node_off; info[2] = a.lds_prim_off; info[3] = a.lds_soup_off; info[4] = a.lds_accel_off;
    info[5] = a.lds_pairs ? 1u : 0u; info[6] = (uint32_t)a.flat.accels.size(); info[7] = (uint32_t)a.flat.nodes.size();
    return true;
}

static void build_and_upload(lg_accel *a, bool with_fast) {
    a->ldss_blocks = 0; a->lds_image_n16 = 0; a->lds_pairs = false; a->pair_refusal.clear(); a->pair_rel.clear(); a->fast_available = true;
        static const bool times = std::getenv("LASGUN_DEBUG_TIMES") != nullptr; // (where lg_accel_from's time goes: flatten / upload / derived)
        const auto t_begin = std::chrono::steady_clock::now();
        // The culling records and strips of the pruned walk's mesh leaves are built when that walk will run: by default from PRUNE_MIN_TRIS
        // triangles in a mesh (below: on), when LASGUN_PRUNE=1 or lg_accel_set_prune(1) ask for it (rebuild_tables).
        size_t big_mesh_tris = 0;
        for (const auto &m : a->scene->meshes) if (m && m->tri.size() / 3 > big_mesh_tris) big_mesh_tris = m->tri.size() / 3;
        const bool with_records = a->prune == 1 || (a->prune < 0 && (prune_env() == 1 || (prune_env() < 0 && big_mesh_tris >= PRUNE_MIN_TRIS)));
        flatten_scene(*a->scene, a->flat, with_fast, with_records); // host HLBVH build + flatten (throws on what the reference would panic on)
        const auto t_flat = std::chrono::steady_clock::now();
        use_device(a->device);
        const FlatScene &f = a->flat;
        TableStage stage; // (committed at the end: one allocation, one copy)
        stage.add(a->nodes, f.nodes); stage.add(a->nodes4, f.nodes4); stage.add(a->primref, f.primref); stage.add(a->spheres, f.spheres); stage.add(a->sphere_mat, f.sphere_mat);
        stage.add(a->cuboids, f.cuboids); stage.add(a->cuboid_mat, f.cuboid_mat); stage.add(a->tri_v, f.tri_v); stage.add(a->tri_n, f.tri_n);
        stage.add(a->tri_t, f.tri_t); stage.add(a->leaf_soup, f.leaf_soup); stage.add(a->chunks, f.chunks); stage.add(a->strips, f.strips); stage.add(a->sphere_ref_leaf, f.sphere_ref_leaf); stage.add(a->cuboid_ref_leaf, f.cuboid_ref_leaf);
        stage.add(a->tri_ref_leaf, f.tri_ref_leaf); stage.add(a->accel_ref_leaf, f.accel_ref_leaf); stage.add(a->vpos, f.vpos); stage.add(a->vnorm, f.vnorm); stage.add(a->vtex, f.vtex);
        stage.add(a->materials, f.materials); stage.add(a->lights, f.lights); // (the accel records: below, once their compact bases are known)
        {   // the counters' two records, zeroed (the second: iteration counters of the diagnostic build)
            static const std::vector<DStats> zero(2);
            stage.add(a->stats, zero);
        }
        const auto t_up = std::chrono::steady_clock::now();
        a->device_bytes = f.nodes.size() * sizeof(DNode) + f.nodes4.size() * sizeof(DNode4) + f.primref.size() * 4 + f.spheres.size() * sizeof(DSphere) +
                          f.cuboids.size() * sizeof(DCuboid) + f.tri_v.size() * 12 + f.vpos.size() * 4 + f.vnorm.size() * 4 + f.leaf_soup.size() * sizeof(DLeafRec) +
                          f.strips.size() * sizeof(DStrip) + f.chunks.size() * sizeof(DChunk) +
                          f.accels.size() * sizeof(DAccel) + f.materials.size() * sizeof(DMaterial);
        if (!a->stream) a->stream = g_streams.take(a->device);
        // per-lane LDS stack: worst case of this scene graph, +2 guard entries
        a->stack_depth = f.max_stack + 2;
        // (the pair form of the walk -- walk.h, traverse_ref<.., PAIR> -- keeps this depth: per level its stack holds the far children that are HIT of the
        // interior nodes on the lane's path, the node form's every far child of those nodes -- a subset, entry for entry; frames and guard entries are the same)
        // the fast kernel falls back to the reference traversal on exact ties, so its stack must hold either
        a->stack_depth_fast1 = (f.max_stack > f.max_stack_fast1 ? f.max_stack : f.max_stack_fast1) + 2;
        if ((size_t)a->stack_depth * 256 * 4 > LDS_MAX)
            throw Error("BVH too deep for the LDS traversal stack (" + std::to_string(a->stack_depth) + " entries per lane; the reference panics beyond 64 per level, bvh.rs:497)");
        a->fast_available = (size_t)a->stack_depth_fast1 * 256 * 4 <= LDS_MAX;
        // The fast tree's tight boxes are only meaningful if every accel's `minv` (which moves the rays) really is the
        // inverse of its `m` (which moved the boxes).  Transform3::rotate(theta, axis) takes the transpose for the inverse
        // without normalising the axis (transform.rs:144-148), so a non-unit axis gives a pair that is not: the reference
        // still renders *something* through its fat, overlapping leaves, and the reference traversal reproduces that
        // bit for bit, but the fast mode is refused for such a scene.
        for (const DAccel &A : f.accels) {
            double worst = 0.0;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) {
                    double v = (c == 3 ? A.m.c[3][r] : 0.0);
                    for (int k = 0; k < 3; ++k) v += A.m.c[k][r] * (c == 3 ? A.minv.c[3][k] : A.minv.c[c][k]);
                    const double want = (c < 3 && r == c) ? 1.0 : 0.0;
                    if (!(std::fabs(v - want) <= worst)) worst = std::fabs(v - want);
                }
            if (!(worst <= 1e-11)) { // two orders below the 1e-9 the fast tree's boxes are pushed out by
                a->fast_available = false;
                a->fast_refusal = "fast mode unavailable: an aggregate's transform and inverse do not match (rotate() about a non-unit axis?)";
            }
        }
        // The fast mode cannot be made exact for meshes in principle: a ray that lies within rounding of a FAR triangle's
        // plane is accepted by the reference wherever it passes (its fat leaves test every triangle), and a tight tree never visits that
        // triangle.  The band in which that happens is ~ 64 u R^2 / edge wide: negligible for a tessellated surface seen from nearby,
        // not for a mesh whose coordinates dwarf its small triangles (round 4's progression_soup_scene: triangles at 1e9 beside
        // triangles of 0.05 -- 5 wrong pixels in 4,100 scenes).  Such a mesh is refused, like a transform that does not invert.
        for (const auto &m : a->scene->meshes) { // (a question about the fast mode: asked when its trees are built -- every lg_accel_set_mode(1) goes through such a build first)
            if (!m || !with_fast) continue;
            double max_abs = 0.0, min_edge = INFINITY;
            for (float v : m->position) if (std::isfinite(v)) max_abs = std::fmax(max_abs, std::fabs((double)v));
            for (size_t t = 0; t + 2 < m->tri.size(); t += 3) {
                double longest = 0.0;
                for (int e = 0; e < 3; ++e) {
                    const size_t i = (size_t)m->tri[t + e].v, j = (size_t)m->tri[t + (e + 1) % 3].v;
                    double d2 = 0.0;
                    for (int c = 0; c < 3; ++c) { const double d = (double)m->position[3 * i + c] - (double)m->position[3 * j + c]; d2 += d * d; }
                    longest = std::fmax(longest, std::sqrt(d2));
                }
                if (longest > 0.0 && std::isfinite(longest)) min_edge = std::fmin(min_edge, longest);
            }
            if (std::isfinite(min_edge) && max_abs > min_edge * 0x1p20) {
                a->fast_available = false;
                a->fast_refusal = "fast mode unavailable: a mesh whose coordinates exceed 2^20 times its smallest triangle (a ray in a far triangle's plane is accepted by the reference wherever it passes)";
            }
        }
        if (!a->fast_available) a->stack_depth_fast1 = a->stack_depth;
        // Scenes whose tables stay in L2: the accel records (LDS_ACCEL_UNITS x 16 bytes each) go into LDS behind the stacks of the 256-lane
        // kernels when that keeps four workgroups on a CU -- entering and leaving nested accels is a chain of dependent fetches of
        // these records (37 % of the walk's cycles on config 4m when they come from L2)
        a->accel_image_n16 = 0;
        {
            const size_t img = f.accels.size() * LDS_ACCEL_UNITS * 16;
            if (f.accels.size() <= 64 && ((size_t)a->stack_depth * 256 * 4 + img) * 4 <= LDS_MAX) a->accel_image_n16 = (uint32_t)(f.accels.size() * LDS_ACCEL_UNITS);
        }
        const size_t extra_lds = (size_t)a->accel_image_n16 * 16;
        size_t lds = (size_t)std::max(a->stack_depth, a->stack_depth_fast1) * 256 * 4 + extra_lds;
        if (lds > 64 * 1024) set_lds_limits(lds, false);
        int per_cu = 0, cus = 0;
        HIP_TRY(trace_occupancy(a->stack_depth, false, extra_lds, &per_cu));
        int per_cu_fast = 0;
        HIP_TRY(trace_occupancy(a->stack_depth_fast1, true, 0, &per_cu_fast));
        if (per_cu_fast < 1) per_cu_fast = 1;
        a->max_blocks_fast = (uint32_t)per_cu_fast;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, a->device));
        if (per_cu < 1) per_cu = 1;
        a->max_blocks = (uint32_t)(per_cu * cus);
        a->max_blocks_fast *= (uint32_t)cus;
        int wb = 0, wbf = 0;
        HIP_TRY(wf_trace_occupancy(a->stack_depth, false, extra_lds, &wb));
        HIP_TRY(wf_trace_occupancy(a->stack_depth_fast1, true, 0, &wbf));
        a->wf_blocks = (uint32_t)((wb < 1 ? 1 : wb) * cus);
        a->wf_blocks_fast = (uint32_t)((wbf < 1 ? 1 : wbf) * cus);
        int qb = 0;
        HIP_TRY(queue_occupancy(a->stack_depth, extra_lds, &qb));
        a->queue_blocks = (uint32_t)((qb < 1 ? 1 : qb) * cus);
        a->cus = (uint32_t)cus;
        // LDS-resident scene: the REFERENCE tree's nodes (56 of 64 bytes, padded to 80 when that fits),
        // its primrefs, the spheres (padded to 48 when that fits) and cuboids, behind 1024 per-lane
        // stacks, all within one CU's LDS.  The flat tables interleave reference and fast trees per
        // accel, so the image renumbers the reference trees compactly (DAccel::lnode_base / lprim_base).
        {
            std::vector<uint32_t> img;
            if (make_lds_image(a, big_mesh_tris, img)) {
                stage.add(a->lds_image, img);
                set_lds_limits(LDS_MAX, true);
                a->ldss_blocks = (uint32_t)cus;
            }
            FlatScene &fm = a->flat;
            stage.add(a->accels, fm.accels); // with the compact bases
            if (a->accel_image_n16) { // the accel records alone, global bases in unit [6] (the LDS-resident image carries compact ones)
                std::vector<uint32_t> img((size_t)a->accel_image_n16 * 4, 0u);
                for (size_t i = 0; i < fm.accels.size(); ++i) {
                    const DAccel &A = fm.accels[i];
                    uint32_t *rec = &img[i * LDS_ACCEL_UNITS * 4];
                    std::memcpy(rec, &A.minv, 96);
                    rec[24] = A.node_base; rec[25] = A.prim_base; rec[26] = 0u; rec[27] = A.flags;
                    rec[28] = (uint32_t)A.parent; rec[29] = A.nchain; rec[30] = A.lone;
                    for (int k = 0; k < MAX_CHAIN; ++k) rec[32 + k] = A.chain[k];
                    std::memcpy(rec + 40, A.prune, sizeof A.prune);
                    std::memcpy(rec + LDS_ACCEL_DOOR * 4, A.door, sizeof A.door);
                }
                stage.add(a->accel_image, img);
            }
        }
        stage.add(a->accel_tri_base, f.accel_tri_base); // (ray queries: k_query.hip)
        stage.add(a->attr_counts, attr_counts_of(a->flat, *a->scene)); // (lg_hit_attributes_of*: k_attributes.hip)
        // The frame table of flat triangles (tri_frames_host.h: the plan): its records are staged as zeros and filled on the
        // device, by the per-hit path's own text (k_tri_frames.hip), before lg_accel_from returns.
        std::vector<uint32_t> tf_base;
        a->tri_frame_records = scene_tri_frames(a->flat, *a->scene, tf_base);
        {
            std::vector<DTriFrameJob> jobs(a->tri_frame_records);
            const std::vector<TriFramesAccel> ta = tri_frames_accels(a->flat, *a->scene);
            if (a->tri_frame_records && !tri_frames_jobs(ta.data(), ta.size(), a->flat.tri_v.size() / 3, tf_base.data(), a->tri_frame_records, jobs.data()))
                throw Error("frame table: the plan does not add up");
            stage.add(a->tri_frame_base, tf_base); stage.add(a->tri_frame_jobs, jobs);
            stage.add(a->tri_frames, std::vector<DTriFrame>(a->tri_frame_records));
        }
        stage.commit(a->arena);
        if (a->tri_frame_records) {
            DParams T{};
            T.accels = a->accels.p; T.tri_v = a->tri_v.p; T.tri_t = a->tri_t.p; T.vpos = a->vpos.p; T.vtex = a->vtex.p;
            T.default_material = a->flat.default_material;
            HIP_TRY(launch_tri_frames(T, a->tri_frame_jobs.p, a->tri_frame_records, a->tri_frames.p, a->stream));
            HIP_TRY(hipStreamSynchronize(a->stream)); // (a caller's stream may carry the first launch that reads it)
        }
        // Which organisation is the default (measured, tools/threshold_sweep.py): the megakernel unless the scene has
        // so many spheres / boxes that BVH-node and sphere tests dominate a ray (>= 512: with the scene tables in LDS
        // the megakernel keeps up to ~50 node + primitive tests per ray; beyond that the traversal kernels' lower
        // register pressure outweighs the per-pixel state traffic); scenes that also carry a big mesh have long,
        // uneven tiles and need more of them per wave to balance.
        {
            size_t big_mesh = 0;
            for (const auto &m : a->scene->meshes) if (m && m->tri.size() / 3 > big_mesh) big_mesh = m->tri.size() / 3;
            // Scenes with glass / mirror run level by level in the wavefront pipeline under the same criterion (tools/bench_configs.py
            // --org=...): where node and sphere tests dominate.  Small specular scenes are a wash (Cornell glass
            // 512^2: 0.81 ms level by level, 0.80 ms in the megakernel since both walk with traverse_ref), and with a big mesh the deeper
            // levels are few, long, incoherent walks through 254-triangle leaves whose slowest wave sets each launch's length
            // (100k-triangle glass torus: 226 against 136 ms): those stay in the megakernel, where other tiles fill the gaps.
            // the reference's mesh leaves hold up to 254 triangles (bvh.rs:187,289): skipping one pays for many node steps -- from PRUNE_MIN_TRIS
            // triangles (tools/prune_threshold_probe.py, profiles/r05_prune_threshold.jsonl: below that the pruned walk is 5-30 % SLOWER on
            // 1024^2 frames and its records are a third to a half of the accel build; rounds 3-5 had 256)
            a->prune_default = big_mesh >= PRUNE_MIN_TRIS;
            a->streaming_pays = f.spheres.size() + f.cuboids.size() >= 512 && !(f.has_specular && big_mesh >= 4096);
            a->mega_narrow = f.spheres.size() + f.cuboids.size() < 512;
            // a big mesh of glass / mirror: the queue organisation (round 4; config 4: 38.7 against the megakernel's 40.8 ms and the
            // level-by-level pipeline's 80; a metal mesh beside a small mirror -- config 4m -- stays in the megakernel: 14.7 / 16.4)
            bool specular_mesh = false; // a mesh of >= 4096 triangles that is itself glass / mirror: every hit on it spawns secondary rays
            for (const DAccel &A : f.accels)
                if ((A.flags & AF_MESH) && A.material >= 0) {
                    const int kind = f.materials[(size_t)A.material].kind;
                    size_t tris = 0;
                    for (const auto &m : a->scene->meshes) if (m && m->tri.size() / 3 > tris) tris = m->tri.size() / 3; // (an upper bound: the largest mesh)
                    specular_mesh = specular_mesh || ((kind == MAT_GLASS || kind == MAT_MIRROR) && tris >= 4096);
                }
            a->queue_default = f.has_specular && big_mesh >= 4096 && specular_mesh;
            a->streaming_min_items = big_mesh >= 4096 ? (1ull << 23) : (1ull << 21); // (config 3's scene at 1024^2: 0.84 ms in the megakernel, 0.99 level by level; at 2048^2: 2.20 / 2.11)
        }
        if (times) {
            const auto t_end = std::chrono::steady_clock::now();
            auto ms = [](auto a0, auto a1) { return std::chrono::duration<double, std::milli>(a1 - a0).count(); };
            std::fprintf(stderr, "[lasgun] accel build: flatten %.3f ms, table uploads %.3f ms, streams / occupancy / LDS images %.3f ms\n", ms(t_begin, t_flat), ms(t_flat, t_up), ms(t_up, t_end));
        }
}

// First request for the fast mode: its trees are built and every table is uploaded into a SECOND accel; only when all of
// that has succeeded are the tables swapped in (a failure -- a HIP error, out of memory -- leaves the accel as it was).
// The reference trees must come out as they did at lg_accel_from: a scene modified since is an error, not a silent
// change of the parity tables.  Caller holds a->mtx.
static void swap_tables(lg_accel &x, lg_accel &y) {
    using std::swap;
    swap(x.flat, y.flat);
    swap(x.arena, y.arena); swap(x.stats, y.stats); // (the counters' record is a view into the arena like the small tables)
    swap(x.nodes, y.nodes); swap(x.nodes4, y.nodes4); swap(x.primref, y.primref); swap(x.spheres, y.spheres); swap(x.sphere_mat, y.sphere_mat);
    swap(x.cuboids, y.cuboids); swap(x.cuboid_mat, y.cuboid_mat); swap(x.tri_v, y.tri_v); swap(x.tri_n, y.tri_n); swap(x.tri_t, y.tri_t);
    swap(x.vpos, y.vpos); swap(x.vnorm, y.vnorm); swap(x.vtex, y.vtex); swap(x.leaf_soup, y.leaf_soup); swap(x.chunks, y.chunks); swap(x.strips, y.strips);
    swap(x.sphere_ref_leaf, y.sphere_ref_leaf); swap(x.cuboid_ref_leaf, y.cuboid_ref_leaf); swap(x.tri_ref_leaf, y.tri_ref_leaf); swap(x.accel_ref_leaf, y.accel_ref_leaf);
    swap(x.accels, y.accels); swap(x.materials, y.materials); swap(x.lights, y.lights); swap(x.accel_tri_base, y.accel_tri_base); swap(x.attr_counts, y.attr_counts);
    swap(x.tri_frames, y.tri_frames); swap(x.tri_frame_jobs, y.tri_frame_jobs); swap(x.tri_frame_base, y.tri_frame_base); swap(x.tri_frame_records, y.tri_frame_records);
    swap(x.lds_image, y.lds_image); swap(x.accel_image, y.accel_image); swap(x.accel_image_n16, y.accel_image_n16);
    swap(x.lds_image_n16, y.lds_image_n16); swap(x.lds_node_off, y.lds_node_off); swap(x.lds_prim_off, y.lds_prim_off);
    swap(x.lds_soup_off, y.lds_soup_off); swap(x.lds_accel_off, y.lds_accel_off);
    swap(x.ldss_blocks, y.ldss_blocks); swap(x.cus, y.cus); swap(x.l0_rel, y.l0_rel);
    swap(x.lds_pairs, y.lds_pairs); swap(x.pair_refusal, y.pair_refusal); swap(x.pair_rel, y.pair_rel);
    swap(x.stack_depth, y.stack_depth); swap(x.stack_depth_fast1, y.stack_depth_fast1); swap(x.max_blocks, y.max_blocks); swap(x.max_blocks_fast, y.max_blocks_fast);
    swap(x.wf_blocks, y.wf_blocks); swap(x.wf_blocks_fast, y.wf_blocks_fast); swap(x.queue_blocks, y.queue_blocks);
    swap(x.queue_default, y.queue_default); swap(x.prune_default, y.prune_default); swap(x.queue_min_items, y.queue_min_items); swap(x.specular_small_items, y.specular_small_items);
    swap(x.device_bytes, y.device_bytes); swap(x.fast_available, y.fast_available); swap(x.fast_refusal, y.fast_refusal);
    swap(x.streaming_pays, y.streaming_pays); swap(x.streaming_min_items, y.streaming_min_items); swap(x.mega_narrow, y.mega_narrow);
    x.packet_scene = y.packet_scene = -1; // (the packet walk's gate reads the tables: asked again at the next launch)
}
// the tables once more, with what was left out of them: the fast mode's trees (lg_accel_set_mode(1)), the pruned walk's leaf records (lg_accel_set_prune(1), lg_audit_prune)
void rebuild_tables(const lg_accel *ca, bool fast) {
    if (fast && ca->flat.has_fast) return;
    lg_accel *a = const_cast<lg_accel *>(ca);
    use_device(a->device);
    std::unique_ptr<lg_accel> next(new lg_accel());
    next->scene = a->scene;
    next->device = a->device;
    next->prune = a->prune == 1 || a->flat.has_records ? 1 : a->prune; // (what the tables hold stays in them)
    next->node_pairs = a->node_pairs; // (the LDS image in the form the switch asks for now)
    next->image_prune = a->prune;     // (... by the caller's own setting of the pruned walk, not by what the tables must hold)
    build_and_upload(next.get(), fast || a->flat.has_fast); // throws: `a` is untouched
    next->prune = a->prune;
    // (bit patterns, not values: a NaN bound of a degenerate scene equals itself here)
    if (next->flat.dump_f.size() != a->flat.dump_f.size() ||
        (!a->flat.dump_f.empty() && std::memcmp(next->flat.dump_f.data(), a->flat.dump_f.data(), a->flat.dump_f.size() * sizeof(a->flat.dump_f[0])) != 0) ||
        next->flat.dump_i != a->flat.dump_i)
        throw Error("the scene was modified after lg_accel_from: the accel's reference trees no longer match it (build a new accel)");
    HIP_TRY(hipDeviceSynchronize()); // nothing may still be reading the tables that are about to be replaced
    swap_tables(*a, *next);
    std::swap(a->flat.dump_f, next->flat.dump_f); // same contents; keeps the storage lg_accel_dump's callers point into
    std::swap(a->flat.dump_i, next->flat.dump_i);
    // `next` (the old tables) is released here; its stream was never created for launches
}

lg_accel *accel_from_on(const lg_scene *s, int device) {
    lg_accel *a = nullptr;
    int rc = guarded([&] {
        a = new lg_accel();
        a->scene = &s->s;
        a->device = device;
        build_and_upload(a, false);
    });
    if (rc) { delete a; return nullptr; }
    return a;
}
