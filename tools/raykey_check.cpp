// tools/raykey_check.cpp -- the coherence key of a query ray (lasgun_amd/csrc/raykey.h: key_bounds, ray_key) in a stand-alone program,
// meant to be built with -fsanitize=address,undefined,float-cast-overflow and run on the CPU (tests/test_raykey_host.py does, and compares
// the keys with tests/raykey_ref.py word for word).  The (uint32_t) cast of a double in key_cell is undefined for a NaN and for a value
// out of range: a clamp that let one through is a sanitizer report here.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all tools/raykey_check.cpp -o check
//   ./check in.bin out.bin
// in.bin: records of { uint64 n; double lo[3], hi[3]; double rays[n][6] } until the file ends; out.bin: the n uint32 keys of every record.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../lasgun_amd/csrc/raykey.h"

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "raykey_check: cannot open %s\n", in ? argv[2] : argv[1]);
        return 2;
    }
    uint64_t n = 0, records = 0, total = 0;
    while (std::fread(&n, sizeof n, 1, in) == 1) {
        double box[6];
        if (n > (1ull << 28) || std::fread(box, sizeof(double), 6, in) != 6) {
            std::fprintf(stderr, "raykey_check: record %llu is cut short\n", (unsigned long long)records);
            return 2;
        }
        // exactly sized heap blocks: a read past a ray or a write past the keys is a sanitizer report
        std::unique_ptr<double[]> rays(new double[6 * n]);
        std::unique_ptr<uint32_t[]> keys(new uint32_t[n]);
        if (std::fread(rays.get(), 6 * sizeof(double), n, in) != n) {
            std::fprintf(stderr, "raykey_check: record %llu is cut short\n", (unsigned long long)records);
            return 2;
        }
        const lg::KeyBounds b = lg::key_bounds(box, box + 3);
        for (uint64_t i = 0; i < n; ++i) keys[i] = lg::ray_key(rays.get() + 6 * i, b);
        if (std::fwrite(keys.get(), sizeof(uint32_t), n, out) != n) return 2;
        ++records;
        total += n;
    }
    if (std::fclose(out) != 0) return 2;
    std::fclose(in);
    std::printf("raykey_check: ok, %llu records, %llu keys\n", (unsigned long long)records, (unsigned long long)total);
    return 0;
}
