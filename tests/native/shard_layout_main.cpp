// TEST INFRASTRUCTURE: prints the row-shard layout of csrc/mrt_shard.h -- the header alone, no HIP, no library -- for every
// "nh shard_index shard_count shard_rows" line on stdin (or one tuple on the command line).  Built with
// -fsanitize=address,undefined and run as a program by tests/test_shard_layout_host.py.
// One output line per tuple: shard_rows shard_count local_rows padded_rows, then the frame row of every local row.
#include <stdio.h>
#include <stdlib.h>

#include "../../micro_raytracer_amd/csrc/mrt_shard.h"

static void emit(unsigned long long nh, unsigned long long index, unsigned long long count, unsigned long long rows)
{
    const mrt::ShardLayout L = mrt::shard_layout((uint32_t)nh, (uint32_t)index, (uint32_t)count, (uint32_t)rows);
    printf("%u %u %u %llu", L.shard_rows, L.shard_count, L.local_rows, (unsigned long long)L.padded_rows);
    for (uint32_t y : L.row_of) printf(" %u", y);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc == 5) {
        emit(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10));
        return 0;
    }
    if (argc != 1) { fprintf(stderr, "usage: shard_layout [nh shard_index shard_count shard_rows]   (or tuples on stdin)\n"); return 2; }
    unsigned long long nh, index, count, rows;
    int n;
    while ((n = scanf("%llu %llu %llu %llu", &nh, &index, &count, &rows)) == 4) {
        if (nh > 0xffffffffull || index > 0xffffffffull || count > 0xffffffffull || rows > 0xffffffffull) { fprintf(stderr, "shard_layout: a value does not fit 32 bits\n"); return 2; }
        emit(nh, index, count, rows);
    }
    if (n != EOF) { fprintf(stderr, "shard_layout: malformed input\n"); return 2; }
    return 0;
}
