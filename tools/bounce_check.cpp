// tools/bounce_check.cpp -- lasgun_amd/csrc/bounce.h (the next ray of a ray path at a vertex: lg_trace_paths*, k_paths.hip) compiled alone
// for the CPU, with its own main: nothing of HIP, nothing loaded into python.  tests/test_bounce_host.py builds it with -ffp-contract=off
// under AddressSanitizer and UBSan and compares what it writes word for word with the numpy restatement (tests/bounce_ref.py).
//
// usage: bounce_check IN OUT
// IN:  records of 16 doubles: action, normal (0: N = ng, 1: N = ns), medium, ior, d[3], p[3], ng[3], ns[3]
// OUT: records of 8 doubles:  o'[3], d'[3], medium', finite (1.0 or 0.0: bounce_finite)
#include <cstdio>
#include <vector>

#include "../lasgun_amd/csrc/bounce.h"

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: bounce_check IN OUT\n"); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "bounce_check: cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[16];
    while (std::fread(buf, sizeof buf, 1, in) == 1) rec.insert(rec.end(), buf, buf + 16);
    std::fclose(in);
    const size_t m = rec.size() / 16;
    std::vector<double> out(m * 8);
    for (size_t i = 0; i < m; ++i) {
        const double *r = &rec[i * 16];
        const lg::V3 d{r[4], r[5], r[6]}, p{r[7], r[8], r[9]}, ng{r[10], r[11], r[12]}, ns{r[13], r[14], r[15]};
        const lg::Bounce b = lg::bounce_next((uint32_t)r[0], r[3], d, p, ng, r[1] != 0.0 ? ns : ng, (uint32_t)r[2]);
        double *o = &out[i * 8];
        o[0] = b.o.x; o[1] = b.o.y; o[2] = b.o.z; o[3] = b.d.x; o[4] = b.d.y; o[5] = b.d.z;
        o[6] = (double)b.medium;
        o[7] = lg::bounce_finite(b) ? 1.0 : 0.0;
    }
    std::FILE *f = std::fopen(argv[2], "wb");
    if (!f || (m && std::fwrite(out.data(), 8 * sizeof(double), m, f) != m) || std::fclose(f) != 0) {
        std::fprintf(stderr, "bounce_check: cannot write %s\n", argv[2]);
        return 2;
    }
    std::printf("bounce_check: ok, %zu vertices\n", m);
    return 0;
}
