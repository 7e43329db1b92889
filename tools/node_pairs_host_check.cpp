// tools/node_pairs_host_check.cpp -- the device-free part of the pair form of the LDS image (lasgun_amd/csrc/pairs_host.h: record sizes,
// the packing of a child word with its range checks, the size bound, the builder) in a stand-alone program, meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_node_pairs_predicate.py does).  It builds random reference trees in the
// flattener's layout (first child = the next record, second child = link), turns each into pair records inside a heap block of EXACTLY the
// stated size (so a write past either end is ASan's to find), reads the records back against the node records, and walks random rays
// through both forms: the same leaves in the same order, every box tested at most once by the pair form and exactly the boxes the node
// form tests when the walk runs to its end.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/node_pairs_host_check.cpp -o check && ./check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../lasgun_amd/csrc/pairs_host.h"

using namespace lg;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Tree {
    std::vector<DNode> nodes;
    uint32_t slots = 0;
};
// a random tree of `leaves` leaves in pre-order; every leaf takes 1 .. max_count slots
static void grow(Tree &t, std::mt19937 &rng, uint32_t leaves, uint32_t max_count, double lo[3], double hi[3]) {
    const size_t me = t.nodes.size();
    t.nodes.emplace_back();
    std::memset(&t.nodes[me], 0, sizeof(DNode));
    for (int k = 0; k < 3; ++k) { t.nodes[me].bmin[k] = lo[k]; t.nodes[me].bmax[k] = hi[k]; }
    t.nodes[me].parent = NO_HIT;
    if (leaves == 1) {
        const uint32_t count = 1u + rng() % max_count;
        t.nodes[me].link = t.slots; t.nodes[me].meta = NODE_LEAF | count;
        t.slots += count;
        return;
    }
    const uint32_t axis = rng() % 3u, left = 1u + rng() % (leaves - 1u);
    std::uniform_real_distribution<double> u(0.3, 0.7);
    const double cut = lo[axis] + (hi[axis] - lo[axis]) * u(rng), overlap = (hi[axis] - lo[axis]) * 0.05;
    double lhi[3] = {hi[0], hi[1], hi[2]}, rlo[3] = {lo[0], lo[1], lo[2]};
    lhi[axis] = cut + overlap; rlo[axis] = cut - overlap;
    grow(t, rng, left, max_count, lo, lhi);
    const uint32_t second = (uint32_t)t.nodes.size();
    grow(t, rng, leaves - left, max_count, rlo, hi);
    t.nodes[me].link = second; t.nodes[me].meta = axis;
}

struct RayH { double o[3], dinv[3]; bool neg[3]; };
static bool slab(const double bmin[3], const double bmax[3], const RayH &r) { // Bounds::intersects as the walk writes it (slab_intersects_nc)
    double tnear = 0, tfar = 0;
    for (int k = 0; k < 3; ++k) {
        const double t1 = (bmin[k] - r.o[k]) * r.dinv[k], t2 = (bmax[k] - r.o[k]) * r.dinv[k];
        const double mn = std::fmin(t1, t2), mx = std::fmax(t1, t2);
        tnear = k ? std::fmax(tnear, mn) : mn; tfar = k ? std::fmin(tfar, mx) : mx;
    }
    return !(tnear > tfar) && !(tfar <= 0.0);
}
struct Trace { std::vector<std::pair<uint32_t, uint32_t>> leaves; std::vector<uint32_t> tested; size_t max_stack = 0; };
// the reference's walk (bvh.rs:471-505) over the node records; stop_after: the any-hit walk's early exit after that many leaves (0: never)
static Trace walk_nodes(const Tree &t, const RayH &r, uint32_t lprim, size_t stop_after) {
    Trace tr;
    std::vector<uint32_t> st;
    uint32_t cur = 0;
    for (;;) {
        const DNode &n = t.nodes[cur];
        tr.tested.push_back(cur);
        if (slab(n.bmin, n.bmax, r)) {
            if (n.meta & NODE_LEAF) {
                tr.leaves.emplace_back(lprim + n.link, lprim + n.link + (n.meta & 0xFFFFu));
                if (stop_after && tr.leaves.size() == stop_after) return tr;
                if (st.empty()) return tr;
                cur = st.back(); st.pop_back();
            } else {
                const bool neg = r.neg[n.meta & 3u];
                st.push_back(neg ? cur + 1u : n.link);
                cur = neg ? n.link : cur + 1u;
                if (st.size() > tr.max_stack) tr.max_stack = st.size();
            }
        } else {
            if (st.empty()) return tr;
            cur = st.back(); st.pop_back();
        }
    }
}
// the pair form over the image; `box_node`: which node record each tested box came from, found by its bytes' place in the image
static Trace walk_pairs(const std::vector<unsigned char> &img, size_t pair_off, size_t root_off, const std::vector<uint32_t> &pair_node,
                        const Tree &t, const RayH &r, size_t stop_after) {
    Trace tr;
    std::vector<uint32_t> st;
    double b[12];
    uint32_t w[4];
    std::memcpy(b, &img[root_off], 48); std::memcpy(w, &img[root_off + PAIR_ROOT_WORD_OFF], 4);
    tr.tested.push_back(0u);
    if (!slab(b, b + 3, r)) return tr;
    uint32_t word = w[0];
    for (;;) {
        if (word & PAIR_LEAF) {
            tr.leaves.emplace_back(pair_word_first(word), pair_word_end(word));
            if (stop_after && tr.leaves.size() == stop_after) return tr;
            if (st.empty()) return tr;
            word = st.back(); st.pop_back();
            continue;
        }
        EXPECT(word >= pair_off && (word - pair_off) % PAIR_REC_BYTES == 0 && (word - pair_off) / PAIR_REC_BYTES < pair_node.size());
        const uint32_t parent = pair_node[(word - pair_off) / PAIR_REC_BYTES];
        std::memcpy(b, &img[word], 96); std::memcpy(w, &img[word + PAIR_WORDS_OFF], 16);
        tr.tested.push_back(parent + 1u); tr.tested.push_back(t.nodes[parent].link);
        const bool hit_a = slab(b, b + 3, r), hit_b = slab(b + 6, b + 9, r);
        int axis = w[2] == 1u ? 0 : w[2] == 2u ? 1 : 2;
        const bool neg = r.neg[axis];
        const uint32_t near_w = neg ? w[1] : w[0], far_w = neg ? w[0] : w[1];
        const bool near_hit = neg ? hit_b : hit_a, far_hit = neg ? hit_a : hit_b;
        if (near_hit && far_hit) { st.push_back(far_w); if (st.size() > tr.max_stack) tr.max_stack = st.size(); word = near_w; }
        else if (near_hit) word = near_w;
        else if (far_hit) word = far_w;
        else { if (st.empty()) return tr; word = st.back(); st.pop_back(); }
    }
}

int main() {
    std::mt19937 rng(0x9A175u);
    // ---- the packing and its range checks
    {
        uint32_t w = 0;
        EXPECT(pair_leaf_word(0, 1, &w) && w == (PAIR_LEAF | (1u << 16)) && pair_word_first(w) == 0 && pair_word_end(w) == 1);
        EXPECT(pair_leaf_word(65535, 1, &w) && pair_word_first(w) == 65535 && pair_word_end(w) == 65536);
        EXPECT(pair_leaf_word(1000, 32767, &w) && pair_word_first(w) == 1000 && pair_word_end(w) == 33767);
        EXPECT(!pair_leaf_word(65536, 1, &w));          // a slot beyond 16 bits
        EXPECT(!pair_leaf_word(65535, 2, &w));          // a range that ends beyond them
        EXPECT(!pair_leaf_word(0, 32768, &w));          // a count beyond 15 bits
        EXPECT(!pair_leaf_word(0, 0, &w));              // the builder emits no empty leaf
        EXPECT(!pair_leaf_word(0xFFFFFFFFFFull, 1, &w));
        EXPECT(pair_interior_word(0, &w) && w == 0u);
        EXPECT(pair_interior_word(0x7FFFFFF0ull, &w) && w == 0x7FFFFFF0u);
        EXPECT(!pair_interior_word(0x80000000ull, &w)); // would read as a leaf
        EXPECT(!pair_interior_word(24, &w));            // not a 16-byte unit
        EXPECT(pair_size_ok(1018, 1, 2037) && !pair_size_ok(2037, 1, 2037) && !pair_size_ok(0, 2, 1) && !pair_size_ok(1400, 1, 2037) && !pair_size_ok(1017, 1, 2037));
        EXPECT(pair_size_ok(0, 1, 1) && pair_size_ok(1018 + 5, 6, 2037 + 5 * 3) && !pair_size_ok(1018, 0, 2036)); // one leaf; six trees; no tree
    }
    // ---- random trees: the image against the node records, the walks against each other
    for (int round = 0; round < 60; ++round) {
        Tree t;
        double lo[3] = {-1.0, -2.0, -0.5}, hi[3] = {2.0, 1.0, 3.5};
        const uint32_t leaves = round == 0 ? 1u : round == 1 ? 2u : 2u + rng() % 300u;
        grow(t, rng, leaves, round % 7 == 0 ? 254u : 4u, lo, hi);
        const size_t n = t.nodes.size(), interior = pair_interior_count(t.nodes.data(), n);
        EXPECT(interior == leaves - 1u && n == 2u * leaves - 1u);
        EXPECT(pair_size_ok(interior, 1, n));
        const uint32_t lprim = rng() % 1000u;
        const size_t lead = (rng() % 4u) * 16u, pair_off = lead, root_off = lead + interior * PAIR_REC_BYTES, bytes = root_off + PAIR_ROOT_BYTES;
        std::vector<unsigned char> img(bytes, 0xA5);
        std::string why;
        const bool fits = (uint64_t)lprim + t.slots <= 65536u;
        const bool ok = pair_build_tree(t.nodes.data(), n, lprim, pair_off, root_off, img.data(), bytes, &why);
        EXPECT(ok == fits);
        if (!ok) continue;
        for (size_t i = 0; i < lead; ++i) EXPECT(img[i] == 0xA5); // nothing outside the stated ranges
        // record by record, in all bytes: a restatement from the node records
        std::vector<uint32_t> pair_node;
        for (uint32_t i = 0; i < n; ++i) if (!(t.nodes[i].meta & NODE_LEAF)) pair_node.push_back(i);
        std::vector<uint32_t> rank(n, 0u);
        for (size_t k = 0; k < pair_node.size(); ++k) rank[pair_node[k]] = (uint32_t)k;
        auto word = [&](uint32_t i) {
            const DNode &c = t.nodes[i];
            return (c.meta & NODE_LEAF) ? (PAIR_LEAF | (lprim + c.link) | ((c.meta & 0xFFFFu) << 16)) : (uint32_t)(pair_off + rank[i] * PAIR_REC_BYTES);
        };
        std::vector<unsigned char> want(bytes, 0xA5);
        for (size_t k = 0; k < pair_node.size(); ++k) {
            const uint32_t i = pair_node[k], c0 = i + 1u, c1 = t.nodes[i].link;
            unsigned char *rec = &want[pair_off + k * PAIR_REC_BYTES];
            std::memcpy(rec, &t.nodes[c0], 48); std::memcpy(rec + 48, &t.nodes[c1], 48);
            const uint32_t w[4] = {word(c0), word(c1), 1u << (t.nodes[i].meta & 3u), 0u};
            std::memcpy(rec + 96, w, 16);
        }
        std::memset(&want[root_off], 0, PAIR_ROOT_BYTES);
        std::memcpy(&want[root_off], &t.nodes[0], 48);
        const uint32_t w0 = word(0);
        std::memcpy(&want[root_off + 48], &w0, 4);
        EXPECT(img == want);
        // every leaf reachable with its slot range, every interior node through exactly one record
        {
            std::vector<uint32_t> todo{w0};
            size_t seen_leaves = 0, seen_pairs = 0;
            uint32_t slots = 0;
            while (!todo.empty()) {
                const uint32_t w = todo.back(); todo.pop_back();
                if (w & PAIR_LEAF) { ++seen_leaves; slots += pair_word_end(w) - pair_word_first(w); continue; }
                ++seen_pairs;
                uint32_t cw[2];
                std::memcpy(cw, &img[w + PAIR_WORDS_OFF], 8);
                todo.push_back(cw[0]); todo.push_back(cw[1]);
            }
            EXPECT(seen_leaves == leaves && seen_pairs == interior && slots == t.slots);
        }
        // the walks
        std::uniform_real_distribution<double> uo(-4.0, 5.0), ud(-1.0, 1.0);
        for (int q = 0; q < 400; ++q) {
            RayH r;
            for (int k = 0; k < 3; ++k) {
                r.o[k] = uo(rng);
                double d = ud(rng);
                if (q % 50 == 7 && k == q % 3) d = 0.0;
                if (q % 50 == 9 && k == q % 3) d = -0.0;
                if (q % 50 == 11) r.o[k] = lo[k]; // on the faces of the root box
                r.dinv[k] = 1.0 / d; r.neg[k] = r.dinv[k] < 0.0;
            }
            const Trace a = walk_nodes(t, r, lprim, 0), b = walk_pairs(img, pair_off, root_off, pair_node, t, r, 0);
            EXPECT(a.leaves == b.leaves);
            std::vector<uint32_t> ta = a.tested, tb = b.tested;
            std::sort(ta.begin(), ta.end()); std::sort(tb.begin(), tb.end());
            EXPECT(ta == tb); // the closest form: the same multiset of box tests
            EXPECT(std::adjacent_find(tb.begin(), tb.end()) == tb.end()); // ... each at most once
            EXPECT(b.max_stack <= a.max_stack); // the stack never holds more than the node form's
            if (a.leaves.size() > 1) { // the any-hit form with the early exit: the same leaves, a superset of the box tests
                const size_t stop = 1u + (size_t)q % a.leaves.size();
                const Trace c = walk_nodes(t, r, lprim, stop), d = walk_pairs(img, pair_off, root_off, pair_node, t, r, stop);
                EXPECT(c.leaves == d.leaves);
                std::vector<uint32_t> tc = c.tested, td = d.tested;
                std::sort(tc.begin(), tc.end()); std::sort(td.begin(), td.end());
                EXPECT(std::includes(td.begin(), td.end(), tc.begin(), tc.end()));
            }
        }
    }
    // ---- what the builder refuses
    {
        Tree t;
        double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
        grow(t, rng, 5, 3, lo, hi);
        const size_t n = t.nodes.size(), interior = pair_interior_count(t.nodes.data(), n), bytes = interior * PAIR_REC_BYTES + PAIR_ROOT_BYTES;
        std::vector<unsigned char> img(bytes, 0);
        std::string why;
        EXPECT(pair_build_tree(t.nodes.data(), n, 0, 0, interior * PAIR_REC_BYTES, img.data(), bytes, &why));
        EXPECT(!pair_build_tree(t.nodes.data(), n, 0, 0, interior * PAIR_REC_BYTES, img.data(), bytes - 16, &why) && !why.empty()); // the root record would leave the image
        EXPECT(!pair_build_tree(t.nodes.data(), n, 0, 16, interior * PAIR_REC_BYTES, img.data(), interior * PAIR_REC_BYTES, &why));  // the pair records would
        EXPECT(!pair_build_tree(t.nodes.data(), n, 0, 8, interior * PAIR_REC_BYTES, img.data(), bytes, &why));                       // not a unit
        EXPECT(!pair_build_tree(t.nodes.data(), 0, 0, 0, 0, img.data(), bytes, &why));                                               // an empty tree
        EXPECT(!pair_build_tree(t.nodes.data(), n, 65536u - 2u, 0, interior * PAIR_REC_BYTES, img.data(), bytes, &why));             // slots beyond 16 bits
        Tree bad = t;
        for (DNode &nd : bad.nodes) if (!(nd.meta & NODE_LEAF)) { nd.link = (uint32_t)n + 3u; break; }
        EXPECT(!pair_build_tree(bad.nodes.data(), n, 0, 0, interior * PAIR_REC_BYTES, img.data(), bytes, &why)); // a child outside the tree
        Tree fat = t;
        for (DNode &nd : fat.nodes) if (nd.meta & NODE_LEAF) { nd.meta = NODE_LEAF | 0xFFFFu; break; }
        EXPECT(!pair_build_tree(fat.nodes.data(), n, 0, 0, interior * PAIR_REC_BYTES, img.data(), bytes, &why)); // a count beyond 15 bits
    }
    if (failures) { std::fprintf(stderr, "node_pairs_host_check: %d failures\n", failures); return 1; }
    std::printf("node_pairs_host_check: ok\n");
    return 0;
}
