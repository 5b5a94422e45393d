// TEST INFRASTRUCTURE: x86 build of the bodies of mrt_gather (csrc/mrt_gather.h) for tests/test_gather_host.py and
// tests/test_gpu_gather.py: the rays of a call, the frame about a normal, and the reduction of one point per 64 emulated lanes.
// Built by the test itself through tests/emu/build.py (without the host packer): the flags of tests/emu/Makefile.
#include <stddef.h>

#include "../../micro_raytracer_amd/csrc/mrt_gather.h"

using namespace mrt;

namespace {

template <u32 OUT>
void reduce_point(const float *sums, const float *dirs, u32 n_dirs, u32 n_samples, float *res)
{
    constexpr u32 W = gather_words(OUT);
    float p[64][W];
    for (u32 l = 0; l < 64u; ++l) gather_lane_partial<OUT>(sums, dirs, n_dirs, l, n_samples, p[l]);
    for (u32 off = 32u; off > 0u; off >>= 1)
        for (u32 l = 0; l < off; ++l)
            for (u32 w = 0; w < W; ++w) p[l][w] = p[l][w] + p[l + off][w];
    const float scale = gather_scale<OUT>(n_dirs);
    for (u32 w = 0; w < W; ++w) res[w] = p[0][w] * scale;
}

}  // namespace

extern "C" {

// The rays of points [first, first + count) of a call on seed (seed_lo, seed_hi): orig, dir [count][n_dirs][3], key [count][n_dirs];
// pos and normal are the call's whole arrays (normal: HEMI_COS only)
void gp_rays(uint32_t seed_lo, uint32_t seed_hi, uint32_t key_base, uint32_t n_dirs, uint32_t dist, float offset, const float *pos,
             const float *normal, uint32_t first, uint32_t count, float *orig, float *dir, uint32_t *key)
{
    const GatherSet g = {seed_lo, seed_hi, key_base, n_dirs, dist, offset};
    for (u32 il = 0; il < count; ++il)
        for (u32 j = 0; j < n_dirs; ++j) {
            const size_t i = (size_t)first + il, r = (size_t)il * n_dirs + j;
            G3 o, d;
            u32 k;
            gather_ray(g, (u32)i, j, pos + i * 3u, normal ? normal + i * 3u : nullptr, o, d, k);
            orig[r * 3u] = o.x; orig[r * 3u + 1u] = o.y; orig[r * 3u + 2u] = o.z;
            dir[r * 3u] = d.x; dir[r * 3u + 1u] = d.y; dir[r * 3u + 2u] = d.z;
            key[r] = k;
        }
}

// unit[3] = gather_unit(normal), and the frame about it
void gp_frame(const float *normal, float *unit, float *t, float *bt)
{
    const G3 n = gather_unit({normal[0], normal[1], normal[2]});
    G3 a, b;
    gather_frame(n, a, b);
    unit[0] = n.x; unit[1] = n.y; unit[2] = n.z;
    t[0] = a.x; t[1] = a.y; t[2] = a.z;
    bt[0] = b.x; bt[1] = b.y; bt[2] = b.z;
}

// sums, dirs [n_points][n_dirs][3] -> res [n_points][3] (out 0) or [n_points][9][3] (out 1).  Returns 0, or 1 for another out.
int gp_reduce(uint32_t out, const float *sums, const float *dirs, uint32_t n_points, uint32_t n_dirs, uint32_t n_samples, float *res)
{
    if (out > 1u) return 1;
    for (u32 pt = 0; pt < n_points; ++pt) {
        const size_t base = (size_t)pt * n_dirs * 3u;
        if (out == MRT_GATHER_SH9) reduce_point<MRT_GATHER_SH9>(sums + base, dirs + base, n_dirs, n_samples, res + (size_t)pt * 27u);
        else reduce_point<MRT_GATHER_MEAN>(sums + base, dirs + base, n_dirs, n_samples, res + (size_t)pt * 3u);
    }
    return 0;
}

// sizeof and the offsets of the last members of the two structs, as this compiler lays them out
void gp_layout(uint32_t *words)
{
    words[0] = (uint32_t)sizeof(mrt_gather_desc);
    words[1] = (uint32_t)offsetof(mrt_gather_desc, n_dirs);
    words[2] = (uint32_t)offsetof(mrt_gather_desc, reserved);
    words[3] = (uint32_t)sizeof(mrt_gather_info);
    words[4] = (uint32_t)offsetof(mrt_gather_info, rays);
    words[5] = (uint32_t)offsetof(mrt_gather_info, lds_bytes);
}

}
