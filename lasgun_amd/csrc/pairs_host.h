// lasgun_amd/csrc/pairs_host.h -- the pair form of the reference trees in the LDS image (walk.h, traverse_ref<.., PAIR>), the
// part that touches no device: record sizes, the packing of a child word with its range checks, the size of a tree's records and the
// builder that turns one reference tree's DNode records into pair records and a root record.  Index arithmetic over caller-supplied
// tables, so kept free of HIP: tools/node_pairs_host_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, and
// accel.cpp calls it.
//
// A pair record (PAIR_REC_BYTES = 112, seven 16-byte units) stands for one INTERIOR node: the boxes of its two children (first child
// = the node after it, second child = DNode::link; 48 bytes each: bmin, bmax), then four words: the first child's word, the second
// child's word, 1 << split axis of the interior node, 0.  A child word says in 32 bits what a stack entry must later say:
//   interior child   the byte offset of ITS pair record in the image (bit 31 clear)
//   leaf child       PAIR_LEAF | first slot (compact numbering, bits 0..15) | slot count << 16 (bits 16..30)
// A root record (56 bytes in a PAIR_ROOT_BYTES = 64 slot) stands for node 0, which has no parent: its box and its own word.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "dscene.h"

namespace lg {

// (the record sizes and the fields of a child word -- PAIR_* -- are dscene.h's: the kernels read them too)

// false: the range does not fit the word (the form is then refused for the accel)
inline bool pair_leaf_word(uint64_t first, uint64_t count, uint32_t *w) {
    if (count == 0 || count > PAIR_COUNT_MAX || first > PAIR_SLOT_MAX || first + count > (uint64_t)PAIR_SLOT_MAX + 1u) return false;
    *w = PAIR_LEAF | (uint32_t)first | ((uint32_t)count << PAIR_SLOT_BITS);
    return true;
}
inline bool pair_interior_word(uint64_t cursor, uint32_t *w) {
    if (cursor >= PAIR_LEAF || (cursor & 15u) != 0u) return false;
    *w = (uint32_t)cursor;
    return true;
}
inline uint32_t pair_word_first(uint32_t w) { return w & PAIR_SLOT_MAX; }
inline uint32_t pair_word_end(uint32_t w) { return (w & PAIR_SLOT_MAX) + ((w >> PAIR_SLOT_BITS) & PAIR_COUNT_MAX); }

// interior nodes of a tree of n records (== its pair records)
inline size_t pair_interior_count(const DNode *nodes, size_t n) {
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) k += (nodes[i].meta & NODE_LEAF) ? 0u : 1u;
    return k;
}
// The bound on the image.  An interior node has exactly two children, so a tree of n records has (n - 1) / 2 interior nodes: over all trees
// 2 * pairs + roots == node records, exactly.  The pair records then hold the 56 payload bytes of every node record but the roots' (112 *
// pairs = 56 * (nodes - roots)), and the image grows by nothing but the root records (against the 80-byte LDS node records it shrinks).
inline bool pair_size_ok(size_t pair_recs, size_t roots, size_t node_recs) { return roots != 0 && pair_recs * 2u + roots == node_recs; }

// One reference tree -- nodes[0 .. n), first child of interior node i = i + 1, second = nodes[i].link, a leaf's slots = lprim_base +
// link .. + (meta & 0xFFFF) -- as pair records at byte offset pair_off of the image (in node order of the interior nodes) and a root
// record at root_off.  `img` holds img_bytes bytes; nothing outside [pair_off, pair_off + 112 * interior) and [root_off, root_off +
// 64) is written.  false (with *why): a malformed tree, a range that does not fit a child word, or records that would leave the image.
inline bool pair_build_tree(const DNode *nodes, size_t n, uint32_t lprim_base, size_t pair_off, size_t root_off, unsigned char *img,
                            size_t img_bytes, std::string *why) {
    auto fail = [&](const char *m) { if (why) *why = m; return false; };
    if (n == 0) return fail("an empty tree");
    if ((pair_off & 15u) || (root_off & 15u)) return fail("record offsets must be multiples of 16");
    std::vector<uint32_t> rank(n, 0u); // pair index of every interior node
    size_t interior = 0;
    for (size_t i = 0; i < n; ++i) if (!(nodes[i].meta & NODE_LEAF)) rank[i] = (uint32_t)interior++;
    if (interior > (img_bytes / PAIR_REC_BYTES) || pair_off > img_bytes || img_bytes - pair_off < interior * PAIR_REC_BYTES)
        return fail("the pair records do not fit the image");
    if (root_off > img_bytes || img_bytes - root_off < PAIR_ROOT_BYTES) return fail("the root record does not fit the image");
    auto word_of = [&](size_t i, uint32_t *w) {
        if (nodes[i].meta & NODE_LEAF) return pair_leaf_word((uint64_t)lprim_base + nodes[i].link, nodes[i].meta & 0xFFFFu, w);
        return pair_interior_word((uint64_t)pair_off + (uint64_t)rank[i] * PAIR_REC_BYTES, w);
    };
    for (size_t i = 0; i < n; ++i) {
        if (nodes[i].meta & NODE_LEAF) continue;
        const size_t c0 = i + 1, c1 = nodes[i].link;
        if (c0 >= n || c1 >= n || c1 <= c0) return fail("an interior node whose children lie outside its tree");
        unsigned char *rec = img + pair_off + (size_t)rank[i] * PAIR_REC_BYTES;
        std::memcpy(rec, nodes[c0].bmin, 24); std::memcpy(rec + 24, nodes[c0].bmax, 24);
        std::memcpy(rec + 48, nodes[c1].bmin, 24); std::memcpy(rec + 72, nodes[c1].bmax, 24);
        uint32_t w[4] = {0u, 0u, 1u << (nodes[i].meta & 3u), 0u};
        if (!word_of(c0, &w[0]) || !word_of(c1, &w[1])) return fail("a child's range does not fit its word");
        if ((nodes[i].meta & 3u) == 3u) return fail("a split axis of 3");
        std::memcpy(rec + PAIR_WORDS_OFF, w, 16);
    }
    unsigned char *root = img + root_off;
    std::memset(root, 0, PAIR_ROOT_BYTES);
    std::memcpy(root, nodes[0].bmin, 24); std::memcpy(root + 24, nodes[0].bmax, 24);
    uint32_t w0 = 0u;
    if (!word_of(0, &w0)) return fail("the root's range does not fit its word");
    std::memcpy(root + PAIR_ROOT_WORD_OFF, &w0, 4);
    return true;
}

} // namespace lg
