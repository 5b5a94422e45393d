// mrt_shard.h — the row-shard layout of a context: which supersampled rows a shard owns and how many rows its planes are
// allocated for.  Plain C++ with no HIP dependency and no packer: the one statement of this geometry in the library
// (create_single and create_group call it, nothing else computes these), and it can be built stand-alone under a sanitizer
// where no device exists (tests/native/shard_layout_main.cpp).
//
// Contract (include/mrt.h):
//   shard_rows == 0 means 8, shard_count == 0 means 1;
//   the effective shard_rows is min(shard_rows, nh): a block taller than the frame owns the same rows as a block of nh rows,
//   every row goes to shard 0 and nobody allocates for rows that do not exist;
//   row block b (rows [b * rows, (b + 1) * rows) of the frame) belongs to shard b % shard_count;
//   padded_rows = ceil(ceil(nh / rows) / count) * rows with the effective rows, or nh when count == 1;
//   all of it in 64 bits, so local_rows <= padded_rows < 2 * nh for every u32 input.
#pragma once
#include <stdint.h>

#include <vector>

namespace mrt {

constexpr uint32_t kShardRowsDefault = 8;

struct ShardLayout {
    uint32_t shard_rows = kShardRowsDefault;      // the effective value: what the kernels divide by
    uint32_t shard_count = 1;                     // 0 taken as 1
    uint32_t local_rows = 0;                      // rows this shard owns = row_of.size()
    uint64_t padded_rows = 0;                     // rows every shard of this geometry allocates for (the largest shard, whole blocks)
    std::vector<uint32_t> row_of;                 // local row -> frame row, ascending
};

// shard_index >= shard_count (after 0 -> 1) owns nothing: the callers refuse it before they get here.
inline ShardLayout shard_layout(uint32_t nh, uint32_t shard_index, uint32_t shard_count, uint32_t shard_rows)
{
    ShardLayout L;
    const uint64_t count = shard_count ? shard_count : 1u;
    uint64_t rows = shard_rows ? shard_rows : kShardRowsDefault;
    if (rows > nh) rows = nh;
    if (rows == 0) rows = 1;                      // nh == 0: no rows at all, keep the divisions defined
    L.shard_rows = (uint32_t)rows;
    L.shard_count = (uint32_t)count;
    const uint64_t n_blocks = ((uint64_t)nh + rows - 1) / rows;
    // this shard's blocks are index, index + count, ...: walk those, not every row (count may be 2^32 - 1)
    for (uint64_t b = shard_index; b < n_blocks; b += count) {
        const uint64_t y0 = b * rows, y1 = y0 + rows < nh ? y0 + rows : nh;
        for (uint64_t y = y0; y < y1; ++y) L.row_of.push_back((uint32_t)y);
    }
    L.local_rows = (uint32_t)L.row_of.size();
    L.padded_rows = count == 1 ? (uint64_t)nh : ((n_blocks + count - 1) / count) * rows;      // < 2 * nh, so it may pass 2^32: 64 bits
    return L;
}

}  // namespace mrt
