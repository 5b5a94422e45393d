// TEST INFRASTRUCTURE: x86 build of csrc/mrt_adapt.h (the adaptive stop rule), for tests/test_adaptive_host.py.
// Built by the test itself through tests/emu/build.py: the flags of tests/emu/Makefile.
#include <stddef.h>

#include "../../micro_raytracer_amd/csrc/mrt_adapt.h"

using namespace mrt;

extern "C" {

// e_pixel of every pixel of an nw x nh frame of sums A, H ([nh][nw][3]) at count n
void adapt_pixel_errors(const float *A, const float *H, u32 nw, u32 nh, u32 n, float *e)
{
    const float rc = adapt_recip(n), rh = adapt_recip(n / 2u);
    for (size_t p = 0; p < (size_t)nw * nh; ++p) e[p] = adapt_pixel_error(A + 3 * p, H + 3 * p, rc, rh);
}

// e_tile, its NaN flag and the stop decision of every 8x8 tile ([n_ty][n_tx])
void adapt_tile_errors(const float *A, const float *H, u32 nw, u32 nh, u32 n, float threshold, float *e_tile, u32 *nan, u32 *conv)
{
    const u32 n_tx = (nw + 7u) / 8u, n_ty = (nh + 7u) / 8u;
    for (u32 ty = 0; ty < n_ty; ++ty)
        for (u32 tx = 0; tx < n_tx; ++tx) {
            bool any_nan = false;
            const float m = adapt_tile_error(A, H, nw, nh, tx, ty, n, &any_nan);
            e_tile[ty * n_tx + tx] = m;
            nan[ty * n_tx + tx] = any_nan ? 1u : 0u;
            conv[ty * n_tx + tx] = adapt_converged(m, any_nan, threshold) ? 1u : 0u;
        }
}

}
