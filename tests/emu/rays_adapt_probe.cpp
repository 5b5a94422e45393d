// TEST INFRASTRUCTURE: x86 build of the per-lane body of csrc/mrt_rays_adapt.h -- the text of mrt_radiance_adaptive's kernel
// pt_rays_tiles -- on a scene packed by pack_scene, for tests/test_radiance_adaptive_host.py: one round over a tile list, laid
// out as the kernel lays it out (one "wavefront" of 64 lanes per listed tile and chunk phase), with the listed reduction of
// mrt_adapt.hip restated in C for the launches that go through the chunk planes.
// Built by the test itself through tests/emu/build.py: the flags of tests/emu/Makefile, with mrt_pack.cpp.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_rays_adapt.h"

// what this probe runs: the feature sets of pt_rays_tiles (MRT_RAYS_LIST of csrc/mrt_rays.h itself)
#define MRT_RAYS(F) LANE_F(F)
#define LANE_FEAT_LIST MRT_RAYS_LIST
#include "lane_host.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *ra_error(void) { return g_err.c_str(); }

// One round: samples [sample_base, + n_samples) of the n_listed tiles of `list` on the rays orig, dir [nh][nw][3], k_split
// wavefronts per tile.  accum [nh][nw][3] is read and written in place (k_split == 1) or receives the fold of the chunk planes
// (k_split >= 2), as does half when it is not NULL; the planes start out as NaN, the stale data of unlisted tiles.
int ra_round(const mrt_render_desc *d, const mrt_desc_ext *ext, uint32_t feat, uint64_t seed, uint32_t sample_base, uint32_t n_samples, uint32_t k_split,
             uint32_t n_listed, const uint32_t *list, const float *orig, const float *dir, float *accum, float *half, uint64_t *segments)
{
    lane::Packing k;
    const int rc = lane::pack(d, ext, PackOpts(), lane::Level(), k, g_err);
    if (rc) return rc;
    if (!lane::with_feat(feat, [](auto) {})) return lane::no_inst(feat, g_err);
    if ((k.pk.features & F_ALL & ~feat) != 0u) { g_err = "FEAT does not cover the scene"; return -104; }
    if (k_split == 0u || (half && k_split < 2u)) { g_err = "k_split: >= 1, and >= 2 with a half buffer"; return -105; }
    const u32 nw = k.pk.nw, nh = k.pk.nh;
    const size_t plane = (size_t)nw * nh * 3u;
    const u32 nc = (sample_base + n_samples - 1u) / kChunk - sample_base / kChunk + 1u;
    std::vector<float> partial;
    lane::set_sampling(k, seed, sample_base, n_samples, accum);
    k.P.k_split = k_split; k.P.to_planes = 0u;
    if (k_split > 1u) {
        uint32_t nan_bits = 0x7fc00000u;
        float nan;
        memcpy(&nan, &nan_bits, sizeof nan);
        partial.assign(plane * nc, nan);
        k.P.partial = partial.data(); k.P.partial_stride = plane;
    }
    uint64_t segs = 0;
    // pt_rays_tiles: wavefront W serves list entry W / k_split with chunk phase W % k_split; a launch of 4-wavefront workgroups
    // also has wavefronts past the list, which stay out of the body
    const u32 n_waves = ((n_listed * k_split + 3u) / 4u) * 4u;
    for (u32 w = 0; w < n_waves; ++w) {
        if (w >= n_listed * k_split) continue;
        const u32 entry = w / k_split, phase = w - entry * k_split;
        for (u32 l = 0; l < 64u; ++l) {
            u32 p;
            if (!rays_tile_pixel(list[entry], l, nw, nh, p)) continue;
            lane::with_feat(feat, [&](auto f) {
                u32 sg = 0;
                rays_tile_body<decltype(f)::value>(k.S, p, phase, lane::ray_at(orig, p), lane::ray_at(dir, p), sg);
                segs += sg;
            });
        }
    }
    if (k_split > 1u) {
        // reduce_chunks_listed (mrt_adapt.hip), restated: per listed in-frame pixel, acc += chunk sums in chunk order, half alike
        for (u32 e = 0; e < n_listed; ++e)
            for (u32 l = 0; l < 64u; ++l) {
                u32 p;
                if (!rays_tile_pixel(list[e], l, nw, nh, p)) continue;
                for (u32 c = 0; c < 3u; ++c) {
                    float a = accum[3 * p + c];
                    for (u32 j = 0; j < nc; ++j) a += partial[(size_t)j * plane + 3 * p + c];
                    accum[3 * p + c] = a;
                    if (half) {
                        float h = half[3 * p + c];
                        for (u32 j = 0; j < nc; ++j) h += partial[(size_t)j * plane + 3 * p + c];
                        half[3 * p + c] = h;
                    }
                }
            }
    }
    if (segments) *segments = segs;
    return 0;
}

}
