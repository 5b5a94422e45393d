"""Row-shard geometries shared by tests/test_shard_layout_host.py and tests/test_gpu_shards.py, and the brute-force statement
of the layout both compare with.  The statement is written here from the contract (include/mrt.h), not taken
from micro_raytracer_amd/dist.py or csrc/mrt_shard.h, which are what it checks."""

DEFAULT_ROWS = 8


def eff_rows(nh, shard_rows):
    return min(shard_rows or DEFAULT_ROWS, nh)


def brute_rows(nh, count, shard_rows, r):
    """Frame rows of shard r: every row whose block index is r modulo the shard count."""
    R, count = eff_rows(nh, shard_rows), count or 1
    return [y for y in range(nh) if (y // R) % count == r]


def owners(nh, count, shard_rows):
    """The shards that can own a row: block b belongs to shard b % count, so with count >= the number of blocks shards
    0 .. blocks-1 own one block each and every other shard owns nothing.  Enumerating these covers every non-empty shard,
    also where count is 2^32 - 1."""
    R = eff_rows(nh, shard_rows)
    n_blocks = -(-nh // R)
    return range(min(count or 1, n_blocks))


def brute_padded(nh, count, shard_rows):
    """The largest shard, rounded up to whole blocks; nh for one shard."""
    R, count = eff_rows(nh, shard_rows), count or 1
    if count == 1:
        return nh
    return max(-(-len(brute_rows(nh, count, shard_rows, r)) // R) * R for r in owners(nh, count, shard_rows))


# ---- the host grid (tests/test_shard_layout_host.py) ---------------------------------------------------------------------------
GRID_NH = (1, 2, 7, 8, 9, 23, 64, 1080)
GRID_COUNT = (0, 1, 2, 3, 5, 8, 64)


def grid_rows(nh):
    return sorted({0, 1, 3, 7, 8, 9, 13, nh - 1, nh, nh + 1, 1000})        # nh - 1 == 0 on a one-row frame: the default


def grid():
    """(nh, count, shard_rows) of the issue's grid; every shard_index of each is checked."""
    return [(nh, count, sr) for nh in GRID_NH for sr in grid_rows(nh) for count in GRID_COUNT]


def extremes():
    """(nh, count, shard_rows, indices): sums that wrap in 32 bits.  shard_rows near 2^32 with small counts (every index), and
    counts near 2^32 with the default rows and with 3-row blocks (indices 0, 1, count - 1 and every shard that owns a row)."""
    out = []
    for nh in GRID_NH:
        for sr in sorted({2**31, 2**32 - nh, 2**32 - nh + 1, 2**32 - 1} - {2**32}):       # (2^32 on a one-row frame is no u32)
            for count in (1, 2, 3, 64):
                out.append((nh, count, sr, tuple(range(count))))
        for count in (2**31, 2**32 - 1):
            for sr in (0, 3, 2**32 - 1):
                idx = sorted({0, 1, count - 1} | set(owners(nh, count, sr)))
                out.append((nh, count, sr, tuple(idx)))
    return out


# ---- the GPU geometries (tests/test_gpu_shards.py): (nh, shard_count, shard_rows) on a 20-pixel-wide frame ------------------------
# An 8x8 wavefront tile of shard-local rows covers 8 / shard_rows blocks that lie shard_count blocks apart in the frame.
GEOMETRIES = [
    # tiles straddling two to eight blocks, a partial last block in the middle of a tile
    (23, 2, 1), (23, 3, 3), (23, 5, 5), (23, 2, 13), (23, 3, 16), (23, 5, 3),
    (52, 3, 1), (52, 2, 3), (52, 5, 5), (52, 3, 13), (52, 2, 16), (52, 5, 13),
    # blocks as tall as the frame and taller: every row on shard 0, planes of nh rows
    (23, 2, 23), (23, 3, 24), (9, 2, 1000), (7, 3, 8),
    # more shards than blocks: shards without rows that still answer mrt_accum with the count
    (9, 5, 3), (7, 5, 7), (23, 5, 13), (9, 4, 0),
    # one row
    (1, 1, 1), (1, 3, 0), (1, 2, 1000),
    # a ragged last block that is its shard's only block, and the default rows on a non-multiple height
    (9, 2, 8), (52, 3, 0),
]
# The two inputs whose 32-bit sums wrapped before the layout moved to 64 bits (shard_rows = 2^32 - 1 with 2 shards;
# shard_count = 2^32 - 1), as (nh, count, shard_rows, shard indices to run, the small geometry they must render like): like
# shard_rows = 9; like 5 shards -- of 8-row blocks, where nine rows are two blocks and three shards are empty, and of 9-row
# blocks, where four are.  The last index of the huge count runs in place of the small geometry's last shard.
OVERFLOW = [
    (9, 2, 2**32 - 1, (0, 1), (9, 2, 9)),
    (9, 2**32 - 1, 0, (0, 1, 2, 3, 2**32 - 2), (9, 5, 0)),
    (9, 2**32 - 1, 9, (0, 1, 2, 3, 2**32 - 2), (9, 5, 9)),
]
# straddling geometries of nh = 23 for the launch shapes (40 samples)
SHAPE_GEOMETRIES = [(23, 2, 3), (23, 3, 5), (23, 5, 13)]
