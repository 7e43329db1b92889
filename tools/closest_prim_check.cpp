// tools/closest_prim_check.cpp -- lasgun_amd/csrc/closest_prim.h (the per-primitive arithmetic of lg_closest_points*, k_closest.hip) compiled
// alone for the CPU, with its own main: nothing of HIP, nothing loaded into python.  tests/test_closest_prim_host.py builds it with
// -ffp-contract=off under AddressSanitizer and UBSan and compares what it writes word for word with the numpy restatement
// (tests/closest_ref.py); built with -DLG_CLOSEST_FAULT=1, 2 or 3 it carries one seeded fault.
//
// usage: closest_prim_check IN OUT
// IN:  records of 32 doubles: kind (1 sphere, 2 box, 3 triangle), q[3], 24 doubles of geometry -- a triangle's a, b, c; a sphere's cw, pw; a
//      box's eight world corners --, group, instance, prim, r2.  Consecutive records of one group are offered to one winner in order.
// OUT: records of 9 doubles: the candidate's x[3] and d2; then the group's winner after this record: its d2, its key (-1: none), its x[3]
#include <cstdio>
#include <vector>

#include "../lasgun_amd/csrc/closest_prim.h"

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: closest_prim_check IN OUT\n"); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "closest_prim_check: cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[32];
    while (std::fread(buf, sizeof buf, 1, in) == 1) rec.insert(rec.end(), buf, buf + 32);
    std::fclose(in);
    const size_t m = rec.size() / 32;
    std::vector<double> out(m * 9);
    lg::ClosestBest best = lg::closest_none();
    double group = -1.0;
    for (size_t i = 0; i < m; ++i) {
        const double *r = &rec[i * 32];
        const lg::V3 q{r[1], r[2], r[3]};
        const double *g = r + 4;
        lg::ClosestPt c;
        const uint32_t kind = (uint32_t)r[0];
        if (kind == 3u) c = lg::closest_triangle(q, lg::V3{g[0], g[1], g[2]}, lg::V3{g[3], g[4], g[5]}, lg::V3{g[6], g[7], g[8]});
        else if (kind == 1u) c = lg::closest_sphere(q, lg::V3{g[0], g[1], g[2]}, lg::V3{g[3], g[4], g[5]});
        else {
            lg::V3 w[8];
            for (int k = 0; k < 8; ++k) w[k] = lg::V3{g[3 * k], g[3 * k + 1], g[3 * k + 2]};
            c = lg::closest_box(q, w);
        }
        if (r[28] != group) { best = lg::closest_none(); group = r[28]; }
        lg::closest_offer(best, c, r[31], lg::closest_key((uint32_t)r[29], kind, (uint32_t)r[30]));
        double *o = &out[i * 9];
        o[0] = c.x.x; o[1] = c.x.y; o[2] = c.x.z; o[3] = c.d2;
        o[4] = best.d2; o[5] = best.key == ~0ull ? -1.0 : (double)best.key;
        o[6] = best.x.x; o[7] = best.x.y; o[8] = best.x.z;
    }
    std::FILE *f = std::fopen(argv[2], "wb");
    if (!f || (m && std::fwrite(out.data(), 9 * sizeof(double), m, f) != m) || std::fclose(f) != 0) {
        std::fprintf(stderr, "closest_prim_check: cannot write %s\n", argv[2]);
        return 2;
    }
    std::printf("closest_prim_check: ok, %zu cases\n", m);
    return 0;
}
