// TEST INFRASTRUCTURE: x86 build of csrc/mrt_denoise_var.h (the variance-guided denoiser mode), for
// tests/test_denoise_var_host.py and tests/test_gpu_denoise_var.py.
// Built by the tests themselves through tests/emu/build.py: the flags of tests/emu/Makefile.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_denoise_var.h"

using namespace mrt;

extern "C" {

// dnv_prep: ev[nh][nw][4] = (e, h2) of the sums A and half sums H at per-pixel counts, the firefly clamp applied (f = +inf: off)
void dv_prep(const float *A, const float *H, const uint32_t *counts, const float *guide, const float *albedo, uint32_t nw, uint32_t nh, uint32_t env,
             float f, float *ev)
{
    dnv_prep_host(A, H, counts, reinterpret_cast<const DnGuide *>(guide), albedo, nw, nh, env != 0u, f, ev);
}

// mrt_denoise in MRT_DN_VARIANCE: out[nh][nw][3]; sv, sn, sp = 1/sigma^2 as the host forms them; var (may be null): the variance
// plane [nh][nw] after the last pass (passes = 0: after the 7x7 estimate)
void dv_filter(const float *A, const float *H, const uint32_t *counts, const float *guide, const float *albedo, uint32_t nw, uint32_t nh, uint32_t passes,
               float sv, float sn, float sp, float f, uint32_t env, float *out, float *var)
{
    const size_t np = (size_t)nw * nh;
    const DnGuide *g = reinterpret_cast<const DnGuide *>(guide);
    if (passes == 0u && !var) {
        for (size_t p = 0; p < np; ++p) {
            const float rc = 1.0f / (float)counts[p];
            for (int k = 0; k < 3; ++k) out[3 * p + k] = A[3 * p + k] * rc;
        }
        return;
    }
    std::vector<float> a(np * 4), b(np * 4);
    dnv_prep_host(A, H, counts, g, albedo, nw, nh, env != 0u, f, a.data());
    dnv_init_host(a.data(), g, nw, nh, sn, sp, b.data());
    for (u32 i = 0; i < passes; ++i) {
        dnv_pass_host(b.data(), g, nw, nh, 1u << i, sv, sn, sp, a.data());
        a.swap(b);
    }
    for (size_t p = 0; p < np; ++p) {
        if (passes == 0u) {
            const float rc = 1.0f / (float)counts[p];
            for (int k = 0; k < 3; ++k) out[3 * p + k] = A[3 * p + k] * rc;
        } else {
            for (int k = 0; k < 3; ++k) out[3 * p + k] = b[4 * p + k] * dn_demod(albedo[3 * p + k], g[p].hit, env != 0u);
        }
        if (var) var[p] = b[4 * p + 3];
    }
}

}
