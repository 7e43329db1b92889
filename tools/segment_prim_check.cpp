// tools/segment_prim_check.cpp -- lasgun_amd/csrc/segment_prim.h (the per-primitive arithmetic of lg_closest_segments*, k_segments.hip)
// compiled alone for the CPU, with its own main: nothing of HIP, nothing loaded into python.  tests/test_segment_prim_host.py builds it with
// -ffp-contract=off under AddressSanitizer and UBSan and compares what it writes word for word with the numpy restatement
// (tests/segment_ref.py); built with -DLG_SEGMENT_FAULT=1, 2 or 3 it carries one seeded fault.
//
// usage: segment_prim_check IN OUT
// IN:  records of 36 doubles: kind (1 sphere, 2 box, 3 triangle), p0[3], p1[3], 24 doubles of geometry -- a triangle's a, b, c; a sphere's
//      cw, pw; a box's eight world corners --, group, instance, prim, r2, one unused.  Consecutive records of one group are offered to one
//      winner in order.
// OUT: records of 12 doubles: the candidate's x[3], s, d2 and (a triangle's) winning sub-candidate; then the group's winner after this
//      record: its d2, its key (-1: none), its s, its x[3]
#include <cstdio>
#include <vector>

#include "../lasgun_amd/csrc/segment_prim.h"

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: segment_prim_check IN OUT\n"); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "segment_prim_check: cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[36];
    while (std::fread(buf, sizeof buf, 1, in) == 1) rec.insert(rec.end(), buf, buf + 36);
    std::fclose(in);
    const size_t m = rec.size() / 36;
    std::vector<double> out(m * 12);
    lg::SegBest best = lg::seg_none();
    double group = -1.0;
    for (size_t i = 0; i < m; ++i) {
        const double *r = &rec[i * 36];
        const lg::V3 p0{r[1], r[2], r[3]}, p1{r[4], r[5], r[6]};
        const double *g = r + 7;
        lg::SegPt c;
        int which = 0;
        const uint32_t kind = (uint32_t)r[0];
        if (kind == 3u) c = lg::seg_triangle(p0, p1, lg::V3{g[0], g[1], g[2]}, lg::V3{g[3], g[4], g[5]}, lg::V3{g[6], g[7], g[8]}, &which);
        else if (kind == 1u) c = lg::seg_sphere(p0, p1, lg::V3{g[0], g[1], g[2]}, lg::V3{g[3], g[4], g[5]});
        else {
            lg::V3 w[8];
            for (int k = 0; k < 8; ++k) w[k] = lg::V3{g[3 * k], g[3 * k + 1], g[3 * k + 2]};
            c = lg::seg_box(p0, p1, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
        }
        if (r[31] != group) { best = lg::seg_none(); group = r[31]; }
        lg::seg_offer(best, c, r[34], lg::closest_key((uint32_t)r[32], kind, (uint32_t)r[33]));
        double *o = &out[i * 12];
        o[0] = c.x.x; o[1] = c.x.y; o[2] = c.x.z; o[3] = c.s; o[4] = c.d2; o[5] = (double)which;
        o[6] = best.d2; o[7] = best.key == ~0ull ? -1.0 : (double)best.key; o[8] = best.s;
        o[9] = best.x.x; o[10] = best.x.y; o[11] = best.x.z;
    }
    std::FILE *f = std::fopen(argv[2], "wb");
    if (!f || (m && std::fwrite(out.data(), 12 * sizeof(double), m, f) != m) || std::fclose(f) != 0) {
        std::fprintf(stderr, "segment_prim_check: cannot write %s\n", argv[2]);
        return 2;
    }
    std::printf("segment_prim_check: ok, %zu cases\n", m);
    return 0;
}
