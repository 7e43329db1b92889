// tools/lit_host_check.cpp -- the device-free host code of lg_scatter_lit* (lasgun_amd/csrc/lit_host.h: the light set's rules, W, n * K * 72,
// n * K * 24 and n * W * 4 with their overflow checks, the NULL and alignment rules of lg_lit_out's nine planes, the host form's staging)
// in a stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_lit_host_sanitized.py does).
// The counts go up to 2^64 - 1: an overflow in forming a size is a UBSan report or a wrong value here, not a short buffer on a card.  The
// launch is stubbed out: a "kernel" that fills the staged planes with values that name their element; every caller's array is a heap block
// of exactly its size, so a copy past an end is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/lit_host_check.cpp -o check && ./check
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../lasgun_amd/csrc/lit_host.h"

using namespace lg;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const double D[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
static const lg_light ONE_LIGHT = {{0.0, 1.0, 0.0}, {1.0, 1.0, 1.0}, {1.0, 0.0, 0.0}};

static lg_light_set set_of(const lg_light *table, uint32_t count, uint32_t per_ray) { return lg_light_set{table, count, per_ray, {0.1, 0.2, 0.3}}; }
static bool refused(const void *accel, const double *rays, size_t n, const lg_light_set *lights, const lg_lit_out *out) {
    try {
        (void)check_lit(accel, rays, n, lights, out);
    } catch (const std::exception &e) {
        return e.what()[0] != 0;
    }
    return false;
}
static bool misaligned(const void *rays, const lg_light_set &lights, const lg_lit_out &out, size_t n) {
    try {
        LitSizes z;
        z.n = n; z.K = lights.count; z.W = lit_words(lights.count);
        check_lit_alignment((const double *)rays, lights, out, z);
    } catch (const std::exception &e) {
        return e.what()[0] != 0;
    }
    return false;
}

// one host-form call without a device: check, stage, "launch", place; then every element of every output is looked at.  planes: a 9-bit mask
static void run(size_t n, uint32_t K, uint32_t per_ray, unsigned planes) {
    const size_t W = (K + 31) / 32;
    std::unique_ptr<lg_hit[]> hits(planes & 1u ? new lg_hit[n] : nullptr);
    std::unique_ptr<double[]> direct(planes & 2u ? new double[3 * n] : nullptr), reflect(planes & 8u ? new double[6 * n] : nullptr),
        reflect_weight(planes & 16u ? new double[3 * n] : nullptr), refract(planes & 32u ? new double[6 * n] : nullptr),
        refract_weight(planes & 64u ? new double[5 * n] : nullptr), terms(planes & 128u ? new double[n * K * 3 + 1] : nullptr);
    std::unique_ptr<uint32_t[]> flags(planes & 4u ? new uint32_t[n] : nullptr), visible(planes & 256u ? new uint32_t[n * W + 1] : nullptr);
    const lg_lit_out out{{hits.get(), direct.get(), flags.get(), reflect.get(), reflect_weight.get(), refract.get(), refract_weight.get()}, terms.get(), visible.get()};
    std::unique_ptr<lg_light[]> table(new lg_light[(per_ray ? n : 1) * K + 1]);
    const lg_light_set ls = set_of(table.get(), K, per_ray);
    int accel = 0; // (any non-NULL handle: the checks do not look behind it)
    const bool any = (planes & 127u) || (K && (planes & 384u));
    EXPECT(refused(&accel, D, n, &ls, &out) == !any);
    if (!any) return;
    const LitSizes z = check_lit(&accel, D, n, &ls, &out);
    EXPECT(z.n == n && z.K == K && z.W == W && z.terms == n * K * 3 && z.visible == n * W && z.lights == (per_ray ? n * K : K));
    LitStaging st(out, z);
    EXPECT(st.scatter.hits.size() == (out.scatter.hits ? n : 0) && st.scatter.direct.size() == (out.scatter.direct ? 3 * n : 0) &&
           st.scatter.flags.size() == (out.scatter.flags ? n : 0) && st.scatter.refract_weight.size() == (out.scatter.refract_weight ? 5 * n : 0));
    EXPECT(st.terms.size() == (out.terms && K ? n * K * 3 : 0) && st.visible.size() == (out.visible && K ? n * W : 0));
    // the "kernel": every staged element gets a value that names it
    for (size_t i = 0; i < st.terms.size(); ++i) st.terms[i] = 0.5 + (double)i;
    for (size_t i = 0; i < st.visible.size(); ++i) st.visible[i] = 0xA0000000u + (uint32_t)i;
    for (size_t i = 0; i < st.scatter.direct.size(); ++i) st.scatter.direct[i] = 0.25 + (double)i;
    for (size_t i = 0; i < st.scatter.flags.size(); ++i) st.scatter.flags[i] = (uint32_t)(i & 7u);
    if (terms) terms[n * K * 3] = -7.0; // (the element behind the plane: placement must not reach it)
    if (visible) visible[n * W] = 0x77777777u;
    place_lit(out, z, st);
    bool ok = true;
    for (size_t i = 0; terms && K && i < n * K * 3; ++i) ok = ok && terms[i] == 0.5 + (double)i;
    for (size_t i = 0; visible && K && i < n * W; ++i) ok = ok && visible[i] == 0xA0000000u + (uint32_t)i;
    for (size_t i = 0; direct && i < 3 * n; ++i) ok = ok && direct[i] == 0.25 + (double)i;
    for (size_t i = 0; flags && i < n; ++i) ok = ok && flags[i] == (uint32_t)(i & 7u);
    EXPECT(ok);
    EXPECT(!terms || terms[n * K * 3] == -7.0);
    EXPECT(!visible || visible[n * W] == 0x77777777u);
    // the plane table: nine planes with lights, seven without, in the struct's order, with their alignments
    lg_lit_out copy = out;
    size_t seen = 0;
    const size_t want_align[9] = {16, 8, 4, 8, 8, 8, 8, 8, 4};
    bool table_ok = true;
    lit_planes(copy, z, [&](auto *p, auto, size_t, size_t align, const char *what) { (void)p; table_ok = table_ok && what[0] != 0 && align == want_align[seen]; ++seen; });
    EXPECT(table_ok && seen == (K ? 9u : 7u));
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
    EXPECT(!refused(&accel, D, SCATTER_MAX_RAYS, &one, &all));
    EXPECT(refused(&accel, D, SCATTER_MAX_RAYS + 1, &one, &all));
    { const lg_light_set s = set_of(&ONE_LIGHT, LG_MAX_CALL_LIGHTS, 1); EXPECT(!refused(&accel, D, SCATTER_MAX_RAYS, &s, &all)); } // 2^38 * 2^10 * 72 < 2^64
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
