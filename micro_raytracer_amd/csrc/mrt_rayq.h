// mrt_rayq.h — per-ray body of the ray-query test hook (mrt_selftest_trace): one closest-hit query and one shadow
// query of trace on a caller-supplied ray.  Shared by the kernel of mrt_rayq.hip and an x86 build (tests/emu/rayq_probe.cpp), so
// that both run the same text.
#pragma once
#include "../../include/mrt.h"
#include "mrt_trace.h"

namespace mrt {

// out[MRT_TRACE_WORDS]: hit, any, renderer, flat instance (both 0xffffffff on a miss), t0 bits, t1 bits, world normal at t0 (bits).
// The ray is traced as given (the path tracer's rays arrive with their origin already shifted by kE along the direction); the
// normal is formed as aov_pixel forms it (mrt_denoise.h).
// ref_walk (the x86 probe only; the kernel passes a constant false): the ray's d.d reads NaN, which sends every mesh query to the
// reference's octree walk and steers nothing else in a scene of meshes alone (tests/emu/emu.cpp emu_mesh_probe)
template <u32 FEAT>
MRT_HD void rayq_body(const Scn &S, V3 o, V3 d, u32 *out, bool ref_walk = false)
{
    RayPre ray = ray_pre<FEAT>(o, d);
    if (ref_walk) ray.dd = __builtin_nanf("");
    Hit h, ha;
    const bool hit = trace<false, FEAT>(S, ray, h);
    const bool any = trace<true, FEAT>(S, ray, ha);
    out[1] = any ? 1u : 0u;
    if (!hit) {
        out[0] = 0u; out[2] = 0xffffffffu; out[3] = 0xffffffffu;
        for (int k = 4; k < (int)MRT_TRACE_WORDS; ++k) out[k] = 0u;
        return;
    }
    const Obj ob = obj_of(S, h);
    const V3 p0 = add(o, muls(d, h.t0));
    const V3 nh0 = to_object(ob, p0);
    const V3 n = hit_normal<FEAT>(S, ob, nh0, h.i0);
    out[0] = 1u; out[2] = (u32)h.rend; out[3] = h.inst;
    out[4] = f2u(h.t0); out[5] = f2u(h.t1);
    out[6] = f2u(n.x); out[7] = f2u(n.y); out[8] = f2u(n.z);
}

// The instantiations of the hook (MRT_RQ(LDS, F) is defined at each use): one per distinct closest-hit code path, each at 256 threads
// (F_BOX | F_LIGHTS: the kernel a scene takes that is F_IDENT | F_BOX | F_LIGHTS but for the sign of a zero in one instance's dir)
#define MRT_RAYQ_LIST \
    MRT_RQ(true, F_IDENT) MRT_RQ(true, F_IDENT | F_BOX | F_LIGHTS) MRT_RQ(true, F_BOX | F_LIGHTS) MRT_RQ(true, F_IDENT | F_BVH) \
    MRT_RQ(true, F_ALL & ~F_TRI) MRT_RQ(true, F_ALL) MRT_RQ(true, F_ALL | F_BVH) \
    MRT_RQ(true, F_ALL | F_COLD) MRT_RQ(true, F_ALL | F_COLD | F_DEEP) MRT_RQ(true, F_ALL | F_BVH | F_COLD | F_DEEP) \
    MRT_RQ(true, F_ALL | F_VATTR) MRT_RQ(true, F_ALL | F_VATTR | F_ENV) \
    MRT_RQ(false, F_ALL) MRT_RQ(false, F_ALL | F_BVH)

}  // namespace mrt
