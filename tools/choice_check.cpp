// tools/choice_check.cpp -- lasgun_amd/csrc/choice.h held to the literals of the ABI: the bits of a launch's organisation as
// lg_accel_last_organisation, lg_tune_entry.choice and a LASGUN_TUNE_FILE line carry them, which integers are well formed, and the twenty
// candidates of the measured choice in their order.  Stand-alone and device-free, for -fsanitize=address,undefined on the CPU;
// tests/test_choice_codec.py builds and runs it.
#include "../lasgun_amd/csrc/choice.h"

#include <cstdio>
#include <cstdlib>

using namespace lg;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::fprintf(stderr, "choice_check: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

static_assert(ORG_MEGA == 0 && ORG_WAVEFRONT == 1 && ORG_QUEUE == 2, "the organisations' numbers are ABI");
static_assert(encode(Choice{ORG_QUEUE, 2, false, true}) == 194 && decode(80).dir == 1 && choice_well_formed(255 - 13) && !choice_well_formed(3), "the codec is constexpr");

int main() {
    for (int v = -1; v <= 256; ++v) {
        CHECK(choice_well_formed(v) == (0 <= v && v < 256 && (v & 15) <= 2));
        if (!choice_well_formed(v)) continue;
        const Choice c = decode(v);
        CHECK((int)c.org == (v & 15));
        CHECK(c.dir == ((v & 16) ? 1 : (v & 64) ? 2 : 0));
        CHECK(c.serial == ((v & 32) != 0));
        CHECK(c.split == ((v & 128) != 0));
        if (!((v & 16) && (v & 64))) CHECK(encode(c) == v);
        else CHECK(encode(c) == (v & ~64)); // both direction bits: bottom-up
    }
    static const int first18[18] = {0, 16, 64, 32, 48, 96, 1, 17, 65, 33, 49, 97, 2, 18, 66, 34, 50, 98};
    for (int rule_serial = 0; rule_serial < 2; ++rule_serial) {
        Choice slot[RACE_SLOTS];
        race_slots(rule_serial != 0, slot);
        CHECK(RACE_SLOTS == 20 && SLOT_MEGA_PARTS == 18 && SLOT_QUEUE_PARTS == 19);
        for (int k = 0; k < 18; ++k) CHECK(encode(slot[k]) == first18[k]);
        CHECK(encode(slot[18]) == (rule_serial ? 224 : 192));
        CHECK(encode(slot[19]) == 194);
        // the rule's slot, found by look-up, is where the index arithmetic of the race put it: only the megakernel's rule has samples in a row
        for (int org = 0; org < 3; ++org)
            for (int serial = 0; serial < 2; ++serial)
                for (int dir = 0; dir < 3; ++dir) {
                    const bool in_a_row = org == ORG_MEGA && serial != 0;
                    CHECK(slot_of(slot, Choice{(Org)org, dir, in_a_row, false}) == org * 6 + (in_a_row ? 3 : 0) + dir);
                }
        CHECK(slot_of(slot, decode(130)) == -1); // (the queue organisation in parts, top-down: no candidate)
    }
    std::printf("choice_check: ok\n");
    return 0;
}
