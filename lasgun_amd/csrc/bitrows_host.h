// lasgun_amd/csrc/bitrows_host.h -- what a bit row is, for the two queries that answer in bit-packed rows (lg_visibility*, lg_open_directions*;
// query.cpp): its used bytes, the refusals both share, the extent of the device form's bits buffer and the host form's compact-to-stride
// placement.  size_t arithmetic that can overflow, so kept free of HIP: tools/bitrows_host_check.cpp runs this text under ASan / UBSan on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

namespace lg {

// The bytes of a row that hold its n bits: ceil(n / 8)
inline size_t bit_row_used_bytes(size_t n) { return n / 8 + (n % 8 ? 1 : 0); }

// What both families refuse of `rows` rows of `cols` bits (neither is 0) whose tiles are `tile_rows` rows x 8 columns; row_bytes counts
// only where there are bits.  The wording is the family's: `too_many` for more than 2^32 - 1 tiles, `rows_name` its name for the row count.
inline void check_bit_rows(size_t rows, size_t cols, unsigned tile_rows, const void *bits, size_t row_bytes, const char *too_many, const char *rows_name) {
    const size_t used = bit_row_used_bytes(cols);
    if (bits && row_bytes < used)
        throw std::runtime_error("row_bytes is " + std::to_string(row_bytes) + ", a row of " + std::to_string(cols) + " bits takes " + std::to_string(used));
    const unsigned long long tile_row_count = (unsigned long long)(rows / tile_rows + (rows % tile_rows ? 1 : 0));
    if (tile_row_count > 0xFFFFFFFFull / used) throw std::runtime_error(too_many);
    if (bits && rows > 1 && row_bytes > (SIZE_MAX - used) / (rows - 1))
        throw std::runtime_error(std::string("bits: ") + rows_name + " rows of row_bytes bytes do not fit the address space");
}

// The bytes of a checked bits buffer from its first to its last written one: the last row ends with its used part
inline size_t bit_rows_extent(size_t rows, size_t row_bytes, size_t used) { return (rows - 1) * row_bytes + used; }

// compact rows (`used` bytes each) -> the caller's stride: the bytes of a row behind its used part are never written
inline void place_bit_rows(uint8_t *bits, size_t row_bytes, const uint8_t *compact, size_t rows, size_t used) {
    for (size_t i = 0; i < rows; ++i) std::memcpy(bits + i * row_bytes, compact + i * used, used);
}

} // namespace lg
