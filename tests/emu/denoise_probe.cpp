// TEST INFRASTRUCTURE: x86 build of csrc/mrt_denoise.h (first-hit AOVs, a-trous filter) and the host packer, for
// tests/test_denoise_host.py and tests/test_gpu_denoise.py.
// Built by the tests themselves: g++ -O2 [-mfma] -std=c++17 -ffp-contract=off -shared -fPIC (no fast-math) with mrt_pack.cpp.
#include <stddef.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_denoise.h"
#include "../../micro_raytracer_amd/csrc/mrt_pack.h"

using namespace mrt;

static std::string g_err;

extern "C" {

const char *dn_error(void) { return g_err.c_str(); }

// mrt_aov of a scene: guide[nh][nw][8] (normal, depth, world point, hit flag), albedo[nh][nw][3], renderer / instance[nh][nw]
// (instance within its renderer, as mrt_aov reports it)
int dn_aov(const mrt_render_desc *d, float *guide, float *albedo, int32_t *renderer, int32_t *instance)
{
    Packed pk;
    const int rc = pack_scene(d, pk, g_err);
    if (rc) return rc;
    Params P = pk.P;
    unsigned long long seg[8] = {0};
    P.segments = seg;
    Scn S;
    S.F = reinterpret_cast<const float *>(pk.blob.data());
    S.U = S.F; S.G = S.F; S.P = &P; S.wk = nullptr; S.wk_stride = 1;
    std::vector<u32> first(P.n_rend, 0u);
    for (u32 i = P.n_inst; i-- > 0;) first[pk.blob[P.off_instx + i * INSTX_WORDS + INSTX_REND]] = i;
    for (u32 y = 0; y < pk.nh; ++y)
        for (u32 x = 0; x < pk.nw; ++x) {
            const AovPixel a = (pk.features & F_BVH) ? aov_pixel<F_ALL | F_BVH>(S, x, y) : aov_pixel<F_ALL>(S, x, y);
            const size_t p = (size_t)y * pk.nw + x;
            memcpy(guide + 8 * p, &a.g, sizeof(DnGuide));
            albedo[3 * p] = a.albedo.x; albedo[3 * p + 1] = a.albedo.y; albedo[3 * p + 2] = a.albedo.z;
            renderer[p] = a.rend;
            instance[p] = a.rend < 0 ? -1 : a.inst - (i32)first[(u32)a.rend];
        }
    return 0;
}

// mrt_denoise: the filtered means out[nh][nw][3] of the sums A[nh][nw][3] at per-pixel counts[nh][nw], guided by guide / albedo
void dn_filter(const float *A, const uint32_t *counts, const float *guide, const float *albedo, uint32_t nw, uint32_t nh, uint32_t passes,
               float sc, float sn, float sp, float *out)
{
    const size_t np = (size_t)nw * nh;
    const DnGuide *g = reinterpret_cast<const DnGuide *>(guide);
    std::vector<float> e(np * 3), t(np * 3);
    for (size_t p = 0; p < np; ++p) {
        const float rc = 1.0f / (float)counts[p];
        for (int k = 0; k < 3; ++k) {
            const float c = A[3 * p + k] * rc;
            if (passes == 0u) out[3 * p + k] = c;
            else e[3 * p + k] = c / dn_demod(albedo[3 * p + k], g[p].hit);
        }
    }
    if (passes == 0u) return;
    for (u32 i = 0; i < passes; ++i) {
        dn_pass_host(e.data(), g, nw, nh, 1u << i, dn_pass_sc(sc, i), sn, sp, t.data());
        e.swap(t);
    }
    for (size_t p = 0; p < np; ++p)
        for (int k = 0; k < 3; ++k) out[3 * p + k] = e[3 * p + k] * dn_demod(albedo[3 * p + k], g[p].hit);
}

}
