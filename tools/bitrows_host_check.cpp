// tools/bitrows_host_check.cpp -- the bit-row host code of lg_visibility* and lg_open_directions* (lasgun_amd/csrc/bitrows_host.h: the used
// bytes of a row, the refusals both families share, the extent of the device form's bits buffer, the compact-to-stride placement) in a
// stand-alone program, meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_bitrows_host_sanitized.py does).
// The counts go up to 2^64 - 1: an overflow in forming a tile count or an extent is a UBSan report or a wrong answer here, not a short
// buffer on a card.  Nothing is allocated for the limits (the counts and a stand-in pointer are enough); for the placement the caller's
// bits are a heap block of exactly the extent, (rows - 1) * row_bytes + used bytes, so an overrun of the last row is an ASan report.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/bitrows_host_check.cpp -o check && ./check
#include "../lasgun_amd/csrc/bitrows_host.h"
#include "host_check.h"

using namespace lg;

static const char *const TOO_MANY = "too many tiles", *const ROWS = "n_rows";

// refused with the family's wording where that is the refusal
static bool refused(size_t rows, size_t cols, unsigned tile_rows, const void *bits, size_t row_bytes) {
    return throws([&] { check_bit_rows(rows, cols, tile_rows, bits, row_bytes, TOO_MANY, ROWS); });
}
static std::string refusal(size_t rows, size_t cols, unsigned tile_rows, const void *bits, size_t row_bytes) {
    return thrown([&] { check_bit_rows(rows, cols, tile_rows, bits, row_bytes, TOO_MANY, ROWS); });
}

// one placement: compact rows that name their byte into a block of exactly the extent, filled with 0xA5
static void place(size_t rows, size_t cols, size_t slack) {
    const size_t used = bit_row_used_bytes(cols), row_bytes = used + slack, extent = bit_rows_extent(rows, row_bytes, used);
    EXPECT(!refused(rows, cols, 8, &failures, row_bytes) && !refused(rows, cols, 64, &failures, row_bytes));
    EXPECT(extent == (rows - 1) * row_bytes + used);
    std::unique_ptr<uint8_t[]> bits(new uint8_t[extent]), compact(new uint8_t[rows * used]); // exactly sized: no slack for the sanitizer to forgive
    std::memset(bits.get(), 0xA5, extent);
    for (size_t i = 0; i < rows * used; ++i) compact[i] = (uint8_t)(i * 7 + 1);
    place_bit_rows(bits.get(), row_bytes, compact.get(), rows, used);
    for (size_t i = 0; i < rows; ++i) {
        for (size_t b = 0; b < used; ++b) EXPECT(bits[i * row_bytes + b] == (uint8_t)((i * used + b) * 7 + 1));
        for (size_t b = used; b < row_bytes && i + 1 < rows; ++b) EXPECT(bits[i * row_bytes + b] == 0xA5);
    }
}

int main() {
    static_assert(sizeof(size_t) == 8, "the limits below are written for a 64-bit size_t");
    const size_t M = 0xFFFFFFFFull, TOP = SIZE_MAX;
    const void *p = &failures; // a stand-in for the caller's bits: the checks do not look behind it
    // ---- the used bytes of a row
    EXPECT(bit_row_used_bytes(1) == 1 && bit_row_used_bytes(7) == 1 && bit_row_used_bytes(8) == 1 && bit_row_used_bytes(9) == 2);
    EXPECT(bit_row_used_bytes(TOP) == (TOP >> 3) + 1 && bit_row_used_bytes(TOP - 7) == TOP >> 3);
    // ---- row_bytes against the used bytes: one below is refused, equal is accepted; without bits row_bytes does not count
    for (size_t n : {(size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)65, (size_t)4096})
        for (unsigned t : {8u, 64u}) {
            const size_t used = bit_row_used_bytes(n);
            EXPECT(refused(3, n, t, p, used - 1) && !refused(3, n, t, p, used) && !refused(3, n, t, nullptr, used - 1) && !refused(3, n, t, nullptr, 0));
        }
    EXPECT(refusal(3, 9, 8, p, 1) == "row_bytes is 1, a row of 9 bits takes 2");
    // ---- the tile count, ceil(rows / tile_rows) * used, exactly at 2^32 - 1 and one above, for both tile heights and with and without bits
    for (const void *b : {p, (const void *)nullptr}) {
        EXPECT(!refused(8 * M, 8, 8, b, 1) && refused(8 * M + 1, 8, 8, b, 1) && refused(8 * M, 9, 8, b, 2));
        EXPECT(!refused(64 * M, 8, 64, b, 1) && refused(64 * M + 1, 8, 64, b, 1) && refused(64 * M, 9, 64, b, 2));
        EXPECT(!refused(8, 8 * M, 8, b, M) && refused(9, 8 * M, 8, b, M) && refused(8, 8 * M + 1, 8, b, M + 1));
        EXPECT(!refused(64, 8 * M, 64, b, M) && refused(65, 8 * M, 64, b, M) && refused(64, 8 * M + 1, 64, b, M + 1));
        EXPECT(!refused(8 * 65535, 8 * 65537, 8, b, 65537) && refused(8 * 65536, 8 * 65536, 8, b, 65536));          // (2^16 - 1)(2^16 + 1) = 2^32 - 1
        EXPECT(!refused(64 * 65535, 8 * 65537, 64, b, 65537) && refused(64 * 65536, 8 * 65536, 64, b, 65536));
        EXPECT(refused(TOP, 1, 8, b, 1) && refused(TOP, 1, 64, b, 1) && refused(1, TOP, 8, b, TOP) && refused(TOP, TOP, 64, b, TOP)); // nothing wraps on the way
    }
    EXPECT(refusal(8 * M + 1, 8, 8, p, 1) == TOO_MANY && refusal(64 * M + 1, 8, 64, nullptr, 1) == TOO_MANY);
    // ---- rows that do not fit the address space: (rows - 1) * row_bytes + used at SIZE_MAX and one stride above
    for (size_t rows : {(size_t)2, (size_t)3, (size_t)9, (size_t)4096, (size_t)1 << 20})
        for (size_t cols : {(size_t)1, (size_t)9, (size_t)4096}) { // (2^26 tiles at the most: it is the stride that is refused)
            const size_t used = bit_row_used_bytes(cols), limit = (TOP - used) / (rows - 1);
            EXPECT(refused(rows, cols, 8, p, limit + 1) && !refused(rows, cols, 8, p, limit));
            EXPECT(refused(rows, cols, 64, p, limit + 1) && !refused(rows, cols, 64, p, limit));
            EXPECT(!refused(rows, cols, 8, nullptr, limit + 1)); // no bits: no rows to place
            EXPECT(bit_rows_extent(rows, limit, used) <= TOP && bit_rows_extent(rows, limit, used) >= limit);
        }
    EXPECT(refusal(2, 9, 8, p, TOP - 1) == "bits: n_rows rows of row_bytes bytes do not fit the address space");
    // one row: its extent is its used part whatever the stride
    EXPECT(!refused(1, 9, 8, p, TOP) && !refused(1, 9, 64, p, TOP) && bit_rows_extent(1, TOP, 2) == 2);
    // ---- placement: compact and a stride of used + 3, over 0xA5
    for (size_t rows : {(size_t)1, (size_t)2, (size_t)9})
        for (size_t cols : {(size_t)1, (size_t)8, (size_t)9, (size_t)65})
            for (size_t slack : {(size_t)0, (size_t)3}) place(rows, cols, slack);
    if (failures) { std::fprintf(stderr, "bitrows_host_check: %d failures\n", failures); return 1; }
    std::printf("bitrows_host_check: ok\n");
    return 0;
}
