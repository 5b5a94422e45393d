// mrt_gather.h — per-ray and per-lane bodies and launchers of mrt_gather: the direction set of a point gather, the
// rays formed from it, and the per-lane part of the reduction of their radiance sums to a mean or to 9 SH coefficients.  Shared by
// the kernels of mrt_gather.hip and an x86 build (tests/emu/gather_probe.cpp), so that both run the same text.  A header of its own
// over mrt_math.h alone: no text another kernel source reads changes with it.
// Everything is f32 and unfused (-ffp-contract=off) except inside sincos_; every product and sum is written in the order it is
// evaluated in.
#pragma once
#include "../../include/mrt.h"
#include "mrt_math.h"

namespace mrt {

struct G3 { float x, y, z; };

// What forms the rays of one call: the context's seed and the words of mrt_gather that the directions depend on
struct GatherSet {
    u32 seed_lo, seed_hi;
    u32 key_base, n_dirs, dist;
    float offset;
};

constexpr float kTwoPi = 6.28318548f;
constexpr u32 kGatherRot = 0x85EBCA6Bu;

// The hashed turn of point i about its axis: mix32 of the point's pix_key (the hash key key_base + i) plus a constant
MRT_HD u32 gather_rot(const GatherSet &g, u32 i)
{
    const u32 pix_key = mix32(g.key_base + i + g.seed_lo) ^ g.seed_hi;
    return mix32(pix_key + kGatherRot);
}

// (sin, cos) of the azimuth of direction j: the golden-ratio lattice on the 23-bit unit lattice, turned by rot
MRT_HD void gather_azimuth(u32 rot, u32 j, float &s, float &c)
{
    const u32 a = rot + j * kGold;
    const float phi = kTwoPi * u32_to_unit(a);
    sincos_(phi, s, c);
}

// MRT_GATHER_SPHERE: spherical Fibonacci point j of n_dirs, uniform in solid angle
MRT_HD G3 gather_dir_sphere(u32 j, u32 n_dirs, float s, float c)
{
    const float z = 1.0f - div_((float)(2u * j + 1u), (float)n_dirs);
    const float q = sqrt_(fmax_(0.0f, 1.0f - z * z));
    return {q * c, q * s, z};
}

// n = normal * (1 / sqrt(|normal|^2)): Vec3f::norm as the path tracer forms it (mrt_trace.h norm)
MRT_HD G3 gather_unit(G3 v)
{
    const float r = recip_sqrt_(v.x * v.x + v.y * v.y + v.z * v.z);
    return {v.x * r, v.y * r, v.z * r};
}

// The branchless orthonormal frame of Duff et al. 2017 about the unit vector n: tangent t, bitangent bt
MRT_HD void gather_frame(G3 n, G3 &t, G3 &bt)
{
    const float sg = __builtin_copysignf(1.0f, n.z);
    const float a = -recip_(sg + n.z);
    const float b = (n.x * n.y) * a;
    t = {1.0f + ((sg * n.x) * n.x) * a, sg * b, -(sg * n.x)};
    bt = {b, sg + (n.y * n.y) * a, -n.y};
}

// MRT_GATHER_HEMI_COS: point j of n_dirs of the cosine-distributed set about the unit vector n (Malley: a disc lattice lifted)
MRT_HD G3 gather_dir_hemi(u32 j, u32 n_dirs, float s, float c, G3 n)
{
    const float u = div_((float)(2u * j + 1u), (float)(2u * n_dirs));
    const float r = sqrt_(u);
    const float lx = r * c, ly = r * s, lz = sqrt_(1.0f - u);
    G3 t, bt;
    gather_frame(n, t, bt);
    return {(t.x * lx + bt.x * ly) + n.x * lz, (t.y * lx + bt.y * ly) + n.y * lz, (t.z * lx + bt.z * ly) + n.z * lz};
}

// Ray (i, j) of the call: point i (pos3, normal3: its three floats each; normal3 is read for HEMI_COS only), direction j.  The
// direction is stored as formed -- no renormalisation --, the origin is pos + dir * offset (SPHERE) or pos + n * offset (HEMI_COS),
// the hash key key_base + i * n_dirs + j (mod 2^32)
MRT_HD void gather_ray(const GatherSet &g, u32 i, u32 j, const float *pos3, const float *normal3, G3 &o, G3 &d, u32 &key)
{
    float s, c;
    gather_azimuth(gather_rot(g, i), j, s, c);
    G3 along;
    if (g.dist == MRT_GATHER_HEMI_COS) {
        const G3 n = gather_unit({normal3[0], normal3[1], normal3[2]});
        d = gather_dir_hemi(j, g.n_dirs, s, c, n);
        along = n;
    } else {
        d = gather_dir_sphere(j, g.n_dirs, s, c);
        along = d;
    }
    o = {pos3[0] + along.x * g.offset, pos3[1] + along.y * g.offset, pos3[2] + along.z * g.offset};
    key = g.key_base + i * g.n_dirs + j;
}

// The 9 real spherical harmonics of bands 0..2 at the stored direction d, in the order of mrt.h
MRT_HD void gather_sh9(G3 d, float (&Y)[9])
{
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * d.y;
    Y[2] = 0.488602512f * d.z;
    Y[3] = 0.488602512f * d.x;
    Y[4] = 1.092548431f * (d.x * d.y);
    Y[5] = 1.092548431f * (d.y * d.z);
    Y[6] = 0.315391565f * (3.0f * (d.z * d.z) - 1.0f);
    Y[7] = 1.092548431f * (d.x * d.z);
    Y[8] = 0.546274215f * (d.x * d.x - d.y * d.y);
}

// floats per point of an output: out[n][3] (MEAN) or out[n][9][3] (SH9)
MRT_HD constexpr u32 gather_words(u32 out) { return out == MRT_GATHER_SH9 ? 27u : 3u; }

// Lane `lane` of the wavefront that reduces one point: the sum, from +0 in rising j, of the terms of directions j = lane, lane + 64,
// ... -- L_ij = S_ij * (1 / n_samples) (MEAN), L_ij.c * Y_k(d_ij) at p[3 k + c] (SH9).  sums, dirs: the point's [n_dirs][3] radiance
// sums and stored directions (dirs is not read for MEAN)
template <u32 OUT>
MRT_HD void gather_lane_partial(const float *sums, const float *dirs, u32 n_dirs, u32 lane, u32 n_samples, float (&p)[gather_words(OUT)])
{
    const float inv = div_(1.0f, (float)n_samples);
    for (u32 w = 0; w < gather_words(OUT); ++w) p[w] = 0.0f;
    for (u32 j = lane; j < n_dirs; j += 64u) {
        const float L[3] = {sums[(size_t)j * 3u] * inv, sums[(size_t)j * 3u + 1u] * inv, sums[(size_t)j * 3u + 2u] * inv};
        if constexpr (OUT == MRT_GATHER_SH9) {
            float Y[9];
            gather_sh9({dirs[(size_t)j * 3u], dirs[(size_t)j * 3u + 1u], dirs[(size_t)j * 3u + 2u]}, Y);
            for (u32 k = 0; k < 9u; ++k)
                for (u32 c = 0; c < 3u; ++c) p[k * 3u + c] += L[c] * Y[k];
        } else {
            for (u32 c = 0; c < 3u; ++c) p[c] += L[c];
        }
    }
}

// What the combined sum p[0] of the 64 lanes (p[l] += p[l + 32], then 16, 8, 4, 2, 1) is scaled by: 1 / n_dirs, or 4 pi / n_dirs
template <u32 OUT>
MRT_HD float gather_scale(u32 n_dirs)
{
    return OUT == MRT_GATHER_SH9 ? div_(12.566370614f, (float)n_dirs) : div_(1.0f, (float)n_dirs);
}

#if defined(__HIPCC__) || defined(__HIP__)
// mrt_gather.hip.  gather_gen: the rays of points [first, first + count) as gather_ray forms them, ray (i - first) * n_dirs + j of
// the outputs (each may be null); pos and normal are the call's whole arrays on the device; count * n_dirs < 2^30.
hipError_t launch_gather_gen(const GatherSet &g, const float *pos, const float *normal, u32 first, u32 count, float *orig, float *dir, u32 *key,
                             hipStream_t stream);
// gather_reduce<out>: one wavefront per point, sums and dirs [count][n_dirs][3] -> res[count][gather_words(out)]
hipError_t launch_gather_reduce(u32 out, const float *sums, const float *dirs, u32 count, u32 n_dirs, u32 n_samples, float *res, hipStream_t stream);
#endif

}  // namespace mrt
