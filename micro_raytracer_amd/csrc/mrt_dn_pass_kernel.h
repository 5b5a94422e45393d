// mrt_dn_pass_kernel.h -- one a-trous pass of the denoiser (mrt_denoise.hip), included twice (no include guard): with MRT_DN_ENV 0
// as dn_pass, and with MRT_DN_ENV 1 as dn_pass_env, the kernel of contexts with an environment texture, whose
// miss pixels are demodulated by their backdrop E(d) too (mrt_denoise.h dn_demod).  The preprocessor, not a shared function, as
// mrt_pt_kernel.h: dn_pass is then exactly the text it was, and the compiler's decisions for it do not move.
#ifndef MRT_DN_ENV
#error "define MRT_DN_ENV (0: dn_pass, 1: dn_pass_env) before including mrt_dn_pass_kernel.h"
#endif
#if MRT_DN_ENV
__global__ void __launch_bounds__(256) dn_pass_env(const DnPassArgs A)
#else
__global__ void __launch_bounds__(256) dn_pass(const DnPassArgs A)
#endif
{
    __shared__ float4 s_e[kDnT * kDnT];
    __shared__ float4 s_g0[kDnT * kDnT];
    __shared__ float4 s_g1[kDnT * kDnT];
    // block -> residue class (rx, ry) and block (bx, by) of that class's sub-image; sub-image pixel (i, j) is frame pixel
    // (rx + s * i, ry + s * j)
    const u32 rx = blockIdx.x % A.cx, bx = blockIdx.x / A.cx;
    const u32 ry = blockIdx.y % A.cy, by = blockIdx.y / A.cy;
    const u32 s = A.step;
    const size_t np = (size_t)A.nw * A.nh;
    for (u32 t = threadIdx.x; t < kDnT * kDnT; t += 256u) {
        const u32 lj = t / kDnT, li = t - lj * kDnT;
        const long long si = (long long)(bx * kDnB + li) - 2, sj = (long long)(by * kDnB + lj) - 2;
        const long long fx = (long long)rx + (long long)s * si, fy = (long long)ry + (long long)s * sj;
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g0 = e, g1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        if (si >= 0 && sj >= 0 && fx < (long long)A.nw && fy < (long long)A.nh) {
            const size_t p = (size_t)fy * A.nw + (size_t)fx;
            g0 = A.guide[p];
            g1 = A.guide[np + p];
            if (A.first) {
                const float r = mean_rc({A.accum, A.rc, A.tile_count, A.nw}, (u32)fx, (u32)fy);
                e.x = (A.accum[3 * p] * r) / dn_demod(A.albedo[3 * p], g1.w, MRT_DN_ENV != 0);
                e.y = (A.accum[3 * p + 1] * r) / dn_demod(A.albedo[3 * p + 1], g1.w, MRT_DN_ENV != 0);
                e.z = (A.accum[3 * p + 2] * r) / dn_demod(A.albedo[3 * p + 2], g1.w, MRT_DN_ENV != 0);
            } else {
                e = A.e_in[p];
            }
        }
        s_e[t] = e; s_g0[t] = g0; s_g1[t] = g1;
    }
    __syncthreads();
    const u32 li = threadIdx.x & 15u, lj = threadIdx.x >> 4;
    const u32 fx = rx + s * (bx * kDnB + li), fy = ry + s * (by * kDnB + lj);
    if ((unsigned long long)rx + (unsigned long long)s * (bx * kDnB + li) >= A.nw ||
        (unsigned long long)ry + (unsigned long long)s * (by * kDnB + lj) >= A.nh) return;
    const u32 c = (lj + 2u) * kDnT + li + 2u;
    auto guide_of = [&](u32 k) { const float4 a = s_g0[k], b = s_g1[k]; DnGuide g; g.nx = a.x; g.ny = a.y; g.nz = a.z; g.t = a.w; g.px = b.x; g.py = b.y; g.pz = b.z; g.hit = b.w; return g; };
    const DnGuide gp = guide_of(c);
    const float4 ep4 = s_e[c];
    const float ep[3] = {ep4.x, ep4.y, ep4.z};
    DnAcc acc;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const u32 k = (u32)((int)(lj + 2u) + dy) * kDnT + (u32)((int)(li + 2u) + dx);
            const float4 eq4 = s_e[k];
            const float eq[3] = {eq4.x, eq4.y, eq4.z};
            acc.add(dn_tap_weight(dn_k5(dx) * dn_k5(dy), ep, eq, gp, guide_of(k), A.sc, A.sn, A.sp), eq);
        }
    float r[3];
    acc.result(ep, r);
    const size_t p = (size_t)fy * A.nw + fx;
    if (A.last) {
        for (u32 ch = 0; ch < 3u; ++ch) A.out[3 * p + ch] = r[ch] * dn_demod(A.albedo[3 * p + ch], gp.hit, MRT_DN_ENV != 0);
    } else {
        A.e_out[p] = make_float4(r[0], r[1], r[2], 0.0f);
    }
}
