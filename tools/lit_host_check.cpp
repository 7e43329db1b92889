// tools/lit_host_check.cpp -- the device-free host code of lg_scatter_lit* (lasgun_amd/csrc/lit_host.h: the light set's rules, W, n * K * 72,
// n * K * 24 and n * W * 4 with their overflow checks, the NULL and alignment rules of lg_lit_out's nine planes, the host form's staging)
// in a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_lit_host_sanitized.py does).
// The counts go up to 2^64 - 1: an overflow in forming a size is a UBSan report or a wrong value here, not a short buffer on a card.  The
// launch is stubbed out: a "kernel" that fills the staged planes with bytes that name their place (host_check.h, staged_round); every caller's array is a heap block
// of exactly its size, so a copy past an end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/lit_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/lit_host.h"
#include "host_check.h"

using namespace lg;

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
static const lg_light ONE_LIGHT = {{0.0, 1.0, 0.0}, {1.0, 1.0, 1.0}, {1.0, 0.0, 0.0}};

static lg_light_set set_of(const lg_light *table, uint32_t count, uint32_t per_ray) { return lg_light_set{table, count, per_ray, {0.1, 0.2, 0.3}}; }
static bool refused(const void *accel, const double *rays, size_t n, const lg_light_set *lights, const lg_lit_out *out) {
    return throws([&] { (void)check_lit(accel, rays, n, lights, out); });
}
static bool misaligned(const void *rays, const lg_light_set &lights, const lg_lit_out &out, size_t n) {
    return throws([&] { LitSizes z; z.n = n; z.K = lights.count; z.W = lit_words(lights.count); check_lit_alignment((const double *)rays, lights, out, z); });
}

// one host-form call without a device: check, then stage, "launch" and place (staged_round); every byte of every output is looked at.
// planes: a 9-bit mask
static void run(size_t n, uint32_t K, uint32_t per_ray, unsigned planes) {
    const size_t W = (K + 31) / 32;
    const auto asked = [&](unsigned bit, auto *type) { return planes & bit ? reinterpret_cast<decltype(type)>(ASKED) : nullptr; };
    lg_lit_out out{{asked(1u, (lg_hit *)nullptr), asked(2u, (double *)nullptr), asked(4u, (uint32_t *)nullptr), asked(8u, (double *)nullptr), asked(16u, (double *)nullptr),
                    asked(32u, (double *)nullptr), asked(64u, (double *)nullptr)}, asked(128u, (double *)nullptr), asked(256u, (uint32_t *)nullptr)};
    std::unique_ptr<lg_light[]> table(new lg_light[(per_ray ? n : 1) * K + 1]);
    const lg_light_set ls = set_of(table.get(), K, per_ray);
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    const bool any = (planes & 127u) || (K && (planes & 384u));
    EXPECT(refused(&accel, D, n, &ls, &out) == !any);
    if (!any) return;
    const LitSizes z = check_lit(&accel, D, n, &ls, &out);
    EXPECT(z.n == n && z.K == K && z.W == W && z.terms == n * K * 3 && z.visible == n * W && z.lights == (per_ray ? n * K : K));
    // the plane table: nine planes with lights, seven without, in the struct's order, with their alignments
    size_t seen = 0;
    const size_t want_align[9] = {16, 8, 4, 8, 8, 8, 8, 8, 4};
    bool table_ok = true;
    lit_planes(out, z, [&](auto *p, size_t, size_t align, const char *what) { (void)p; table_ok = table_ok && what[0] != 0 && align == want_align[seen]; ++seen; });
    EXPECT(table_ok && seen == (K ? 9u : 7u));
    // the staging: each plane's bytes; terms and visible are n * K * 3 doubles and n * W words exactly (their blocks end there)
    const StagedRound r = staged_round([&](auto &&f) { lit_planes(out, z, f); });
    std::vector<size_t> want{planes & 1u ? 96 * n : 0, planes & 2u ? 8 * 3 * n : 0, planes & 4u ? 4 * n : 0, planes & 8u ? 8 * 6 * n : 0, planes & 16u ? 8 * 3 * n : 0, planes & 32u ? 8 * 6 * n : 0,
                             planes & 64u ? 8 * 5 * n : 0};
    if (K) { want.push_back(planes & 128u ? 8 * n * K * 3 : 0); want.push_back(planes & 256u ? 4 * n * W : 0); }
    EXPECT(r.plane_bytes == want);
}

int main() {
    int accel = 0;
    double buf[64];
    uint32_t words[16];
    lg_hit hit;
    const lg_lit_out all{{&hit, buf, words, buf, buf, buf, buf}, buf, words};
    const lg_lit_out none{{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr};
    const lg_lit_out lights_only{{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, buf, words};
    const lg_light_set one = set_of(&ONE_LIGHT, 1, 0);

    // W
    EXPECT(lit_words(0) == 0 && lit_words(1) == 1 && lit_words(32) == 1 && lit_words(33) == 2 && lit_words(64) == 2 && lit_words(65) == 3 && lit_words(1024) == 32);
    EXPECT(lit_words(0xFFFFFFFFu) == 0x8000000u); // (no wrap in count + 31)

    // the light set's rules
    EXPECT(!refused(&accel, D, 3, &one, &all));
    EXPECT(refused(nullptr, D, 3, &one, &all) && refused(&accel, nullptr, 3, &one, &all) && refused(&accel, D, 3, nullptr, &all) && refused(&accel, D, 3, &one, nullptr));
    EXPECT(refused(&accel, D, 3, &one, &none));
    { const lg_light_set s = set_of(&ONE_LIGHT, LG_MAX_CALL_LIGHTS, 0); EXPECT(!refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(&ONE_LIGHT, LG_MAX_CALL_LIGHTS + 1, 0); EXPECT(refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(&ONE_LIGHT, 0xFFFFFFFFu, 1); EXPECT(refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(&ONE_LIGHT, 1, 2); EXPECT(refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(&ONE_LIGHT, 1, 0xFFFFFFFFu); EXPECT(refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(nullptr, 1, 0); EXPECT(refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(nullptr, 1, 1); EXPECT(refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(nullptr, 0, 0); EXPECT(!refused(&accel, D, 3, &s, &all)); }          // K == 0: no table is looked at
    { const lg_light_set s = set_of(nullptr, 0, 1); EXPECT(!refused(&accel, D, 3, &s, &all)); }
    { const lg_light_set s = set_of(nullptr, 0, 0); EXPECT(refused(&accel, D, 3, &s, &lights_only)); }   // ... and terms / visible are no planes
    EXPECT(!refused(&accel, D, 3, &one, &lights_only));

    // the sizes at the edge of the address space: n * K * 72, n * K * 24, n * W * 4, and the ray limit
    const size_t TOP = SIZE_MAX;
    EXPECT(!refused(&accel, D, QUERY_MAX_RAYS, &one, &all));
    EXPECT(refused(&accel, D, QUERY_MAX_RAYS + 1, &one, &all));
    { const lg_light_set s = set_of(&ONE_LIGHT, LG_MAX_CALL_LIGHTS, 1); EXPECT(!refused(&accel, D, QUERY_MAX_RAYS, &s, &all)); } // 2^38 * 2^10 * 72 < 2^64
    { const lg_light_set s = set_of(&ONE_LIGHT, 1024, 0);
      EXPECT(refused(&accel, D, TOP / 72 / 1024 + 1, &s, &all));  // n * K * 72 wraps
      EXPECT(refused(&accel, D, TOP / 24 / 1024 + 1, &s, &all));  // n * K * 24 wraps
      EXPECT(refused(&accel, D, TOP / 1024 + 1, &s, &all));       // n * K wraps
      EXPECT(refused(&accel, D, TOP / 4 / 32 + 1, &s, &all)); }   // n * W * 4 wraps
    EXPECT(refused(&accel, D, TOP, &one, &all) && refused(&accel, D, TOP / 96 + 1, &one, &all));
    { // the messages name what does not fit
      std::string what;
      const lg_light_set s = set_of(&ONE_LIGHT, 1, 0);
      try { (void)check_lit(&accel, D, TOP / 72 + 1, &s, &lights_only); } catch (const std::exception &e) { what = e.what(); }
      EXPECT(what.find("does not fit the address space") != std::string::npos); }

    // alignment: rays 8; hits 16; the double planes, terms and a per-ray table 8; flags and visible 4; NULL is not misaligned
    alignas(16) static unsigned char raw[256];
    const lg_light_set per_ray = set_of((const lg_light *)raw, 2, 1), shared = set_of((const lg_light *)(raw + 4), 2, 0), per_ray_off = set_of((const lg_light *)(raw + 4), 2, 1);
    const lg_lit_out fine{{(lg_hit *)raw, (double *)raw, (uint32_t *)raw, (double *)raw, (double *)raw, (double *)raw, (double *)raw}, (double *)raw, (uint32_t *)(raw + 4)};
    EXPECT(!misaligned(raw, per_ray, fine, 1) && !misaligned(raw, shared, fine, 1) && !misaligned(raw, per_ray, none, 1)); // (a shared table is host memory: any address)
    EXPECT(misaligned(raw + 4, per_ray, fine, 1) && misaligned(raw, per_ray_off, fine, 1));
    for (unsigned plane = 0; plane < 9; ++plane) {
        const size_t want_align[9] = {16, 8, 4, 8, 8, 8, 8, 8, 4};
        lg_lit_out o = fine;
        void **slot = plane < 7 ? reinterpret_cast<void **>(&o.scatter) + plane : plane == 7 ? reinterpret_cast<void **>(&o.terms) : reinterpret_cast<void **>(&o.visible);
        *slot = raw + want_align[plane] / 2;
        EXPECT(misaligned(raw, per_ray, o, 1));
        *slot = raw + want_align[plane];
        EXPECT(!misaligned(raw, per_ray, o, 1));
    }
    { // K == 0: terms and visible are not looked at
      lg_lit_out o = fine;
      o.terms = (double *)(raw + 1); o.visible = (uint32_t *)(raw + 1);
      EXPECT(!misaligned(raw, set_of(nullptr, 0, 0), o, 1) && misaligned(raw, per_ray, o, 1)); }

    // the staging for every subset of the nine planes, shared and per ray, K at the word edges
    for (unsigned planes = 0; planes < 512; ++planes) run(5, 33, planes & 1u, planes);
    const uint32_t Ks[] = {0, 1, 31, 32, 33, 64, 65, 70};
    for (uint32_t K : Ks)
        for (size_t n : {(size_t)1, (size_t)64, (size_t)65}) { run(n, K, 0, 511); run(n, K, 1, 2u | 128u | 256u); run(n, K, 1, 128u); run(n, K, 0, 256u); }

    if (failures) { std::fprintf(stderr, "lit_host_check: %d failure(s)\n", failures); return 1; }
    std::printf("lit_host_check: ok\n");
    return 0;
}
