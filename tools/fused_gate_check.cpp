// tools/fused_gate_check.cpp -- the device-free gate of the fused form of the camera's level 0 (lasgun_amd/csrc/fused_host.h: which chains
// of the level-by-level pipeline shade in their closest and shadow passes and launch no shade pass) in a stand-alone program with its own
// main, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_fused_shade_gate.py does).  One asking passes;
// every refusing condition alone flips it, with its own reason; every combination of conditions is refused unless it is that one asking.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/fused_gate_check.cpp -o check && ./check
#include <cstdio>

#include "../lasgun_amd/csrc/fused_host.h"

using namespace lg;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// the headline frame's asking: the camera's own level 0, one level, one light, packet closest, pair shadow, switch on
static FusedAsk good() {
    FusedAsk q;
    q.switched_on = true; q.camera_level0 = true; q.levels = 1u; q.nlights = 1ul; q.packet_closest = true; q.pair_shadow = true;
    return q;
}

int main() {
    CHECK(fused_shade_gate(good()) == FUSED_OK);
    { FusedAsk q = good(); q.switched_on = false; CHECK(fused_shade_gate(q) == FUSED_SWITCH_OFF); }
    { FusedAsk q = good(); q.camera_level0 = false; CHECK(fused_shade_gate(q) == FUSED_OWN_LEVEL0); } // a radiance query, a gather, a view batch, light groups, lit scatter
    { FusedAsk q = good(); q.levels = 2u; CHECK(fused_shade_gate(q) == FUSED_LEVELS); }               // glass or a mirror, recursion 1
    { FusedAsk q = good(); q.levels = 9u; CHECK(fused_shade_gate(q) == FUSED_LEVELS); }
    { FusedAsk q = good(); q.levels = 0u; CHECK(fused_shade_gate(q) == FUSED_LEVELS); }               // (never asked; refused all the same)
    { FusedAsk q = good(); q.nlights = 0ul; CHECK(fused_shade_gate(q) == FUSED_LIGHTS); }             // no shadow pass would finish the pixels
    { FusedAsk q = good(); q.nlights = 2ul; CHECK(fused_shade_gate(q) == FUSED_LIGHTS); }
    { FusedAsk q = good(); q.nlights = 33ul; CHECK(fused_shade_gate(q) == FUSED_LIGHTS); }
    { FusedAsk q = good(); q.nlights = ~0ul; CHECK(fused_shade_gate(q) == FUSED_LIGHTS); }
    { FusedAsk q = good(); q.packet_closest = false; CHECK(fused_shade_gate(q) == FUSED_NOT_PACKET); } // a scene the packet gate refuses, its switch off
    { FusedAsk q = good(); q.pair_shadow = false; CHECK(fused_shade_gate(q) == FUSED_NOT_PAIRS); }     // fast mode, a pruned launch, tables in L2

    // every combination: only the one asking passes
    int passed = 0;
    for (unsigned bits = 0; bits < 16u; ++bits)
        for (unsigned levels = 0; levels < 4u; ++levels)
            for (unsigned long lights = 0; lights < 4ul; ++lights) {
                FusedAsk q;
                q.switched_on = (bits & 1u) != 0; q.camera_level0 = (bits & 2u) != 0; q.packet_closest = (bits & 4u) != 0; q.pair_shadow = (bits & 8u) != 0;
                q.levels = levels; q.nlights = lights;
                const bool want = bits == 15u && levels == 1u && lights == 1ul;
                CHECK((fused_shade_gate(q) == FUSED_OK) == want);
                passed += fused_shade_gate(q) == FUSED_OK ? 1 : 0;
            }
    CHECK(passed == 1);

    if (failures) { std::fprintf(stderr, "fused_gate_check: %d failures\n", failures); return 1; }
    std::printf("fused_gate_check: ok\n");
    return 0;
}
