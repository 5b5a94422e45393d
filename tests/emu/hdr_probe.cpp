// TEST INFRASTRUCTURE: x86 build of the per-element bodies of the linear float image (csrc/mrt_hdr.h) and of the
// host's tap tables (box_taps / lanczos3_taps of csrc/mrt_pack.cpp) for tests/test_hdr_host.py.
// Built by the test itself through tests/emu/build.py: the flags of tests/emu/Makefile.
#include <string.h>

#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_hdr.h"
#include "../../micro_raytracer_amd/csrc/mrt_pack.h"

using namespace mrt;

namespace {

void taps_of(uint32_t filter, uint32_t src, uint32_t dst, ResampleTaps &t)
{
    if (filter == 1u) box_taps(src, dst, t); else lanczos3_taps(src, dst, t);
}

template <u32 R>
void vertical(const HdrSrc &S, uint32_t rh, const ResampleTaps &v, std::vector<float> &tmp)
{
    const u32 row = S.nw * 3u;
    for (u32 oy0 = 0; oy0 < rh; oy0 += R)
        for (u32 e = 0; e < row; ++e) {
            float t[R];
            hdr_vertical<R>(S, e, oy0, rh, v.left.data(), v.count.data(), v.weight.data(), v.cap, t);
            for (u32 r = 0; r < R && oy0 + r < rh; ++r) tmp[(size_t)(oy0 + r) * row + e] = t[r];
        }
}

}  // namespace

extern "C" {

// The tap table of one axis (filter 0: Lanczos3, 1: box).  Returns cap; with cap_in >= cap writes left[dst], count[dst] and
// weight[dst][cap_in] (unused entries 0).
uint32_t hd_taps(uint32_t filter, uint32_t src, uint32_t dst, uint32_t *left, uint32_t *count, float *weight, uint32_t cap_in)
{
    ResampleTaps t;
    taps_of(filter, src, dst, t);
    if (left && count && weight && cap_in >= t.cap) {
        memset(weight, 0, sizeof(float) * (size_t)dst * cap_in);
        for (uint32_t o = 0; o < dst; ++o) {
            left[o] = t.left[o]; count[o] = t.count[o];
            memcpy(weight + (size_t)o * cap_in, t.weight.data() + (size_t)o * t.cap, sizeof(float) * t.cap);
        }
    }
    return t.cap;
}

// mrt_img_hdr's arithmetic on sums[nh][nw][3] with rc (tile_count null) or per-tile counts: out[rh][rw][3]; rows = the output
// rows one call of the vertical body forms (1 or 4).  Returns 0, or 1 for another value of rows.
int hd_img(const float *sums, float rc, const uint32_t *tile_count, uint32_t nw, uint32_t nh, uint32_t rw, uint32_t rh, uint32_t filter,
           uint32_t rows, float *out)
{
    const HdrSrc S = {sums, rc, tile_count, nw};
    if (nw == rw && nh == rh) {
        for (u32 y = 0; y < nh; ++y)
            for (u32 e = 0; e < nw * 3u; ++e) out[(size_t)y * nw * 3u + e] = hdr_clamp(hdr_mean(S, y, e));
        return 0;
    }
    ResampleTaps v, h;
    taps_of(filter, nh, rh, v);
    taps_of(filter, nw, rw, h);
    std::vector<float> tmp((size_t)rh * nw * 3u);
    if (rows == 1u) vertical<1>(S, rh, v, tmp);
    else if (rows == 4u) vertical<4>(S, rh, v, tmp);
    else return 1;
    for (u32 y = 0; y < rh; ++y)
        for (u32 ox = 0; ox < rw; ++ox)
            hdr_horizontal(tmp.data() + (size_t)y * nw * 3u, h.left[ox], h.count[ox], h.weight.data() + (size_t)ox * h.cap,
                           out + ((size_t)y * rw + ox) * 3u);
    return 0;
}

}
