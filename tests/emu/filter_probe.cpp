// TEST INFRASTRUCTURE: x86 build of the bilinear texture filter of csrc/mrt_trace.h -- tex_bilinear alone, the
// material lookup tex_fetch_bilinear and the environment's env_color on a hand-made blob -- for tests/test_filter_host.py.  (The
// packer, the AOV pass and render_pixel with the filter switches go through tests/emu/env_probe.cpp, which takes any ext.)
// Built by the test itself through tests/emu/build.py: the flags of tests/emu/Makefile.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../../micro_raytracer_amd/csrc/mrt_trace.h"

using namespace mrt;

namespace {

// A blob that holds one texture as a material texture (TEX record 0) and as the environment (ENV record):
//   [0..3] TEX  [4..259] the k/255 LUT as the packer writes it  [260..267] ENV  [268..] the texels (f32 words, or RGB8 bytes)
enum : u32 { kTex = 0, kLut = 4, kEnv = 260, kTexels = 268 };

struct Blob {
    std::vector<u32> w;
    Params P;
    Scn S;
    Blob(u32 tw, u32 th, u32 fmt, const void *texels, u32 mapping, float rot, u32 env_flags)
    {
        const size_t n = (size_t)tw * th * 3;
        w.assign(kTexels + (fmt == TEXFMT_U8 ? (n + 3) / 4 : n), 0u);
        w[kTex + TEX_W] = tw; w[kTex + TEX_H] = th; w[kTex + TEX_FMT] = fmt; w[kTex + TEX_OFF] = fmt == TEXFMT_U8 ? kTexels * 4u : (u32)kTexels;
        for (int k = 0; k < 256; ++k) w[kLut + k] = f2u((float)k / 255.0f);
        w[kEnv + ENV_W] = tw; w[kEnv + ENV_H] = th; w[kEnv + ENV_OFF] = w[kTex + TEX_OFF]; w[kEnv + ENV_FMT] = fmt;
        w[kEnv + ENV_MAP] = mapping; w[kEnv + ENV_ROT] = f2u(rot); w[kEnv + ENV_PWR] = f2u(0.5f); w[kEnv + ENV_FLAGS] = env_flags;
        if (fmt != TEXFMT_NONE) memcpy(w.data() + kTexels, texels, fmt == TEXFMT_U8 ? n : n * sizeof(float));
        memset(&P, 0, sizeof P);
        P.off_tex = kTex; P.off_lut = kLut; P.off_env = kEnv;
        P.sky[0] = 1.0f; P.sky[1] = 1.0f; P.sky[2] = 1.0f;
        S.F = reinterpret_cast<const float *>(w.data());
        S.U = S.F; S.G = S.F; S.P = &P; S.wk = nullptr; S.wk_stride = 1;
    }
};

}  // namespace

extern "C" {

// byte offsets of the Params members the packing test reads: off_mat, n_rend, off_env, off_rend
void fl_params_offsets(uint32_t *out /*[4]*/)
{
    out[0] = (uint32_t)offsetof(Params, off_mat); out[1] = (uint32_t)offsetof(Params, n_rend);
    out[2] = (uint32_t)offsetof(Params, off_env); out[3] = (uint32_t)offsetof(Params, off_rend);
}

// tex_bilinear on n coordinates uv[n][2] of a tw x th texture (fmt 1: f32 texels, 2: RGB8): out[n][3]
void fl_core(uint32_t tw, uint32_t th, uint32_t fmt, const void *texels, uint32_t clamp_v, uint32_t n, const float *uv, float *out)
{
    const Blob b(tw, th, fmt, texels, 0u, 0.0f, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        const V3 r = tex_bilinear(b.S.F + kTex, b.S.G, b.S.F + kLut, uv[2 * i], uv[2 * i + 1], clamp_v);
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}

// the material lookups: filtered != 0 tex_fetch_bilinear (with its fall-back to the nearest rule), else tex_fetch; fmt 0: a
// texture without texels; cold != 0: the F_COLD instantiation (texels through S.G)
void fl_tex(uint32_t tw, uint32_t th, uint32_t fmt, const void *texels, uint32_t filtered, uint32_t clamp_v, uint32_t cold, uint32_t n,
            const float *uv, float *out)
{
    const Blob b(tw, th, fmt, texels, 0u, 0.0f, 0u);
    constexpr u32 A = F_ALL | F_VATTR | F_ENV;
    for (uint32_t i = 0; i < n; ++i) {
        UV c; c.x = uv[2 * i]; c.y = uv[2 * i + 1];
        V3 r;
        const u32 fl = MATF_BILINEAR | (clamp_v ? (u32)MATF_CLAMP_V : 0u);
        if (filtered) r = cold ? tex_fetch_bilinear<A | F_COLD>(b.S, 0, c, fl) : tex_fetch_bilinear<A>(b.S, 0, c, fl);
        else r = cold ? tex_fetch<A | F_COLD>(b.S, 0, c) : tex_fetch<A>(b.S, 0, c);
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    }
}

// env_color (sky.color = 1) for n directions d[n][3]; flags = word 7 of the ENV record; uv[n][2] = env_uv of the direction
void fl_env(uint32_t tw, uint32_t th, uint32_t fmt, const void *texels, uint32_t mapping, float rot, uint32_t flags, uint32_t n,
            const float *d, float *out, float *uv)
{
    const Blob b(tw, th, fmt, texels, mapping, rot, flags);
    for (uint32_t i = 0; i < n; ++i) {
        const V3 dir = v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        float pwr;
        const V3 r = env_color<F_ALL | F_VATTR | F_ENV>(b.S, dir, pwr);
        out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
        const UV c = env_uv(mapping, rot, dir);
        uv[2 * i] = c.x; uv[2 * i + 1] = c.y;
    }
}

}
