// tools/nearest_list_check.cpp -- lasgun_amd/csrc/nearest_list.h (the per-point list of lg_nearest*, k_nearest.hip: admissibility, the order,
// the rule between a candidate and a full list, the insertion) compiled alone for the CPU, with its own main: nothing of HIP, nothing loaded
// into python.  tests/test_nearest_list_host.py builds it under AddressSanitizer and UBSan and compares what it writes word for word with
// numpy's lexsort of (d2, key); built with -DLG_NEAREST_FAULT=1, 2 or 3 it carries one seeded fault.
//
// usage: nearest_list_check IN OUT
// IN:  records of 6 64-bit words: group, k (1 .. 8), the candidate's d2 (an f64's bits), its key, its slot, the point's r2 (an f64's bits).
//      Consecutive records of one group are one point's stream of candidates, offered in order to one list of k.
// OUT: per group 1 + 3 * 8 words: m, then 8 entries of d2 bits, key, slot -- all ones from entry m on.
// The list lives in a heap block of EXACTLY k entries: an entry touched beyond it is an ASan report.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../lasgun_amd/csrc/nearest_list.h"

namespace {
struct HeapList {
    std::unique_ptr<lg::NearestEntry[]> e;
    uint32_t k;
    explicit HeapList(uint32_t n) : e(new lg::NearestEntry[n]), k(n) {}
    lg::NearestEntry get(uint32_t i) const { return e[i]; }
    void set(uint32_t i, const lg::NearestEntry &v) { e[i] = v; }
};
double as_double(uint64_t w) { double d; std::memcpy(&d, &w, sizeof d); return d; }
uint64_t as_word(double d) { uint64_t w; std::memcpy(&w, &d, sizeof w); return w; }
} // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: nearest_list_check IN OUT\n"); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "nearest_list_check: cannot read %s\n", argv[1]); return 2; }
    std::vector<uint64_t> rec;
    uint64_t buf[6];
    while (std::fread(buf, sizeof buf, 1, in) == 1) rec.insert(rec.end(), buf, buf + 6);
    std::fclose(in);
    const size_t n = rec.size() / 6;
    std::vector<uint64_t> out;
    size_t groups = 0;
    for (size_t i = 0; i < n;) {
        const uint64_t group = rec[i * 6];
        const uint32_t k = (uint32_t)rec[i * 6 + 1];
        if (k < 1u || k > 8u) { std::fprintf(stderr, "nearest_list_check: k out of range\n"); return 2; }
        HeapList list(k);
        uint32_t m = 0;
        for (; i < n && rec[i * 6] == group; ++i) {
            const uint64_t *r = &rec[i * 6];
            const lg::NearestEntry c{as_double(r[2]), (unsigned long long)r[3], (uint32_t)r[4]};
            if (!lg::nearest_admissible(c.d2, as_double(r[5]))) continue;
            lg::nearest_insert(list, m, k, c);
            if (lg::nearest_worst(list, m, k) != (m == k ? list.get(k - 1u).d2 : INFINITY)) { std::fprintf(stderr, "nearest_list_check: nearest_worst\n"); return 1; }
        }
        out.push_back(m);
        for (uint32_t j = 0; j < 8u; ++j) {
            if (j < m) { const lg::NearestEntry e = list.get(j); out.push_back(as_word(e.d2)); out.push_back(e.key); out.push_back(e.slot); }
            else out.insert(out.end(), 3, ~0ull);
        }
        ++groups;
    }
    std::FILE *f = std::fopen(argv[2], "wb");
    if (!f || (!out.empty() && std::fwrite(out.data(), sizeof(uint64_t), out.size(), f) != out.size()) || std::fclose(f) != 0) {
        std::fprintf(stderr, "nearest_list_check: cannot write %s\n", argv[2]);
        return 2;
    }
    std::printf("nearest_list_check: ok, %zu groups of %zu candidates\n", groups, n);
    return 0;
}
