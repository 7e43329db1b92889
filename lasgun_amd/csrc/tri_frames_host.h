// lasgun_amd/csrc/tri_frames_host.h -- the frame table of flat triangles (DTriFrame, dscene.h; k_tri_frames.hip builds it, shade.h's
// shade_frame_tri reads it in the fused packet closest pass), the part that touches no device: which accels get records,
// where each accel's records start, how large the table is, and the list the build kernel works through.  Kept free of HIP:
// tools/tri_frames_check.cpp runs exactly this text under AddressSanitizer / UBSan on the CPU, accel.cpp calls it at the accel build,
// launch.cpp asks tri_frames_launch_gate, lg_scene_tri_frames_gate hands the plan to the tests.
//
// A record is made for every (mesh instance accel a, triangle k) where a's mesh has no vertex normals (the normal of such a hit is the
// triangle's own, up to a sign), the instance has at most TRI_FRAMES_MAX_INSTANCE triangles and the accel's records together are at
// most TRI_FRAMES_MAX_RECORDS -- the table is for a handful of walls, not for a tessellated surface whose records no cache would hold,
// and not for an accel that is rebuilt for every frame around a big mesh.  Wrong means wrong pixels or a read outside a table: every
// condition is stated, each alone refuses, and what does not add up is refused whole.
#pragma once
#include <cstddef>
#include <cstdint>

#include "dscene.h"

namespace lg {

constexpr uint32_t TRI_FRAMES_MAX_INSTANCE = 1024u; // triangles of one mesh instance
constexpr uint32_t TRI_FRAMES_MAX_RECORDS = 4096u;  // records of one accel
constexpr size_t TRI_FRAME_BYTES = 176u;            // == sizeof(DTriFrame): 21 doubles and a word, padded to 8
static_assert(sizeof(DTriFrame) == TRI_FRAME_BYTES, "one record");

enum TriFramesRefusal : int {
    TRI_FRAMES_OK = 0,
    TRI_FRAMES_NOT_MESH = 1,     // a group: its primitives are spheres, cuboids and other accels
    TRI_FRAMES_HAS_NORMALS = 2,  // AF_HAS_N: the normal is interpolated per hit
    TRI_FRAMES_EMPTY = 3,        // no triangles
    TRI_FRAMES_INSTANCE_CAP = 4, // more than TRI_FRAMES_MAX_INSTANCE triangles
    TRI_FRAMES_MALFORMED = 5,    // its triangles are not all inside the triangle tables
};

// a mesh instance accel as the plan sees it: its DAccel::flags, its mesh's first triangle in the triangle tables and how many it has
struct TriFramesAccel {
    uint32_t flags, tri_base, faces;
};

// one accel's answer; n_tris: triangles in the scene's triangle tables
inline TriFramesRefusal tri_frames_accel_gate(const TriFramesAccel &A, size_t n_tris) {
    if (!(A.flags & AF_MESH)) return TRI_FRAMES_NOT_MESH;
    if (A.flags & AF_HAS_N) return TRI_FRAMES_HAS_NORMALS;
    if (A.faces == 0u) return TRI_FRAMES_EMPTY;
    if (A.faces > TRI_FRAMES_MAX_INSTANCE) return TRI_FRAMES_INSTANCE_CAP;
    if ((size_t)A.tri_base >= n_tris || (size_t)A.faces > n_tris - (size_t)A.tri_base) return TRI_FRAMES_MALFORMED;
    return TRI_FRAMES_OK;
}

// The plan: base[a] (n_accels words, written whole) = accel a's first record, NO_HIT where it has none; returns the records of the table.
// An accel whose admitted instances together exceed TRI_FRAMES_MAX_RECORDS gets no table at all: every base is NO_HIT and 0 is returned.
inline uint32_t tri_frames_plan(const TriFramesAccel *accels, size_t n_accels, size_t n_tris, uint32_t *base) {
    size_t total = 0;
    for (size_t a = 0; a < n_accels; ++a) {
        base[a] = NO_HIT;
        if (tri_frames_accel_gate(accels[a], n_tris) != TRI_FRAMES_OK) continue;
        if (total <= TRI_FRAMES_MAX_RECORDS) base[a] = (uint32_t)total; // (beyond the cap nothing is kept: see below)
        total += accels[a].faces;
    }
    if (total > TRI_FRAMES_MAX_RECORDS) {
        for (size_t a = 0; a < n_accels; ++a) base[a] = NO_HIT;
        return 0u;
    }
    return (uint32_t)total;
}

// Is (base, records) a plan of these accels -- what tri_frames_plan would have made?  Every accel with a base passes its own gate, the
// blocks follow one another without a gap from record 0 and end at `records`, which is within the cap.  The table's readers and its
// builder index it by base[a] + k, k < faces: with this true no such index is at or beyond `records`.
inline bool tri_frames_plan_ok(const TriFramesAccel *accels, size_t n_accels, size_t n_tris, const uint32_t *base, uint32_t records) {
    if (records > TRI_FRAMES_MAX_RECORDS) return false;
    size_t next = 0;
    for (size_t a = 0; a < n_accels; ++a) {
        if (base[a] == NO_HIT) continue;
        if (tri_frames_accel_gate(accels[a], n_tris) != TRI_FRAMES_OK) return false;
        if ((size_t)base[a] != next) return false;
        next += accels[a].faces;
        if (next > (size_t)records) return false;
    }
    return next == (size_t)records;
}

// The build kernel's list: jobs[r] = (accel, global triangle index) of record r, `records` entries and not one more.  false (nothing
// written beyond what was already) where the plan does not add up.
inline bool tri_frames_jobs(const TriFramesAccel *accels, size_t n_accels, size_t n_tris, const uint32_t *base, uint32_t records, DTriFrameJob *jobs) {
    if (!tri_frames_plan_ok(accels, n_accels, n_tris, base, records)) return false;
    for (size_t a = 0; a < n_accels; ++a) {
        if (base[a] == NO_HIT) continue;
        for (uint32_t k = 0; k < accels[a].faces; ++k) jobs[(size_t)base[a] + k] = DTriFrameJob{(uint32_t)a, accels[a].tri_base + k};
    }
    return true;
}

// bytes of a table of `records` records
inline size_t tri_frames_bytes(uint32_t records) { return (size_t)records * TRI_FRAME_BYTES; }

// The launch's part: the table is read by the fused packet closest launch alone, when the switch is on and the accel holds a table.
inline bool tri_frames_launch_gate(bool switched_on, bool fused_packet_closest, uint32_t records) {
    return switched_on && fused_packet_closest && records != 0u && records <= TRI_FRAMES_MAX_RECORDS;
}

} // namespace lg
