// lasgun_amd/csrc/choice.h -- how a launch is organised, as a value and as the integer that leaves the library for it (ABI: what
// lg_accel_last_organisation returns, lg_tune_entry.choice, the last word of a LASGUN_TUNE_FILE line); the bits are spelled here alone.
// Device-free: launch.cpp, capi.cpp (lg_tune_import) and tune.cpp (the file) include it; tools/choice_check.cpp holds it to the literals.
#pragma once

namespace lg {

enum Org : int { ORG_MEGA = 0, ORG_WAVEFRONT = 1, ORG_QUEUE = 2 }; // the megakernel, level by level, the queue organisation
// The direction a launch's tiles are claimed in when nothing is forced or measured: from the middle row outwards.  What a frame shows
// tends to sit in its middle, and a launch should END on cheap tiles: config 4 in the megakernel 36.2 -> 32.8 ms, 4m 13.1 -> 12.7,
// simple.rs 0.55 -> 0.53, nothing slower among the configs (profiles/r05_ab_tile_middle.jsonl).
constexpr int DIR_DEFAULT = 2;
struct Choice {
    Org org;
    int dir;     // the launch's tiles are claimed 0 top-down, 1 bottom-up, 2 from the middle row outwards
    bool serial; // the megakernel takes a pixel's samples one after the other ("in a row"), not side by side
    bool split;  // the megakernel / the queue organisation hand a small launch's tiles out in parts
};
// organisation in the low four bits, + 16 bottom-up, + 64 middle-out, + 32 samples in a row, + 128 tiles in parts
constexpr int encode(Choice c) { return (int)c.org | (c.dir == 1 ? 16 : c.dir == 2 ? 64 : 0) | (c.serial ? 32 : 0) | (c.split ? 128 : 0); }
constexpr Choice decode(int v) { return Choice{(Org)(v & 15), (v & 16) ? 1 : (v & 64) ? 2 : 0, (v & 32) != 0, (v & 128) != 0}; } // (16 and 64: bottom-up)
// what an integer from outside (lg_tune_import, a tune file) must be to be remembered
constexpr bool choice_well_formed(int v) { return v >= 0 && v < 256 && (v & 15) <= 2; }

// The candidates of the measured choice, in the order they are raced and reported in: [organisation][samples side by side, in a row]
// [top-down, bottom-up, middle-out], then the megakernel and the queue organisation with their tiles in parts -- middle-out, the megakernel's
// samples as the rule has them (`rule_serial`).  Which of them can take a launch is launch.cpp's business.
constexpr int RACE_SLOTS = 20, SLOT_MEGA_PARTS = 18, SLOT_QUEUE_PARTS = 19;
inline void race_slots(bool rule_serial, Choice (&slot)[RACE_SLOTS]) {
    for (int org = 0; org < 3; ++org)
        for (int serial = 0; serial < 2; ++serial)
            for (int dir = 0; dir < 3; ++dir) slot[org * 6 + serial * 3 + dir] = Choice{(Org)org, dir, serial != 0, false};
    slot[SLOT_MEGA_PARTS] = Choice{ORG_MEGA, DIR_DEFAULT, rule_serial, true};
    slot[SLOT_QUEUE_PARTS] = Choice{ORG_QUEUE, DIR_DEFAULT, false, true};
}
// the first slot that is `c` (-1: none)
inline int slot_of(const Choice (&slot)[RACE_SLOTS], Choice c) {
    for (int k = 0; k < RACE_SLOTS; ++k) if (encode(slot[k]) == encode(c)) return k;
    return -1;
}

} // namespace lg
