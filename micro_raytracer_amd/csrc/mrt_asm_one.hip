// mrt_asm_one.hip — ONE instantiation of pt_megakernel, for reading its assembly (`make asm-one INST=... THREADS=...`).
// Not part of libmrt_hip.so.  The kernel is mrt_pt_kernel.h's, compiled as in the library, so its code and its resource usage
// are the library's; only the other instantiations are missing (seconds instead of the minutes of `make asm`).
//   MRT_ONE_INST      the feature set, as the lists of mrt_megakernel.h spell it (default F_IDENT, the headline frame's kernel)
//   MRT_ONE_THREADS   the workgroup size, 64 / 256 / 512 / 1024 (default 256)
//   MRT_ONE_LDS       1: scene staged in LDS (default), 0: the scene-in-L2 kernel (256 threads)
//   MRT_ONE_LIST      1: the tile-list kernel of mrt_adapt.hip (default 0: the ordinary one)
#include <hip/hip_runtime.h>

#include "mrt_pt_kernel.h"

#ifndef MRT_ONE_INST
#define MRT_ONE_INST F_IDENT
#endif
#ifndef MRT_ONE_THREADS
#define MRT_ONE_THREADS 256
#endif
#ifndef MRT_ONE_LDS
#define MRT_ONE_LDS 1
#endif
#ifndef MRT_ONE_LIST
#define MRT_ONE_LIST 0
#endif

namespace mrt {

#if MRT_ONE_LIST
template __global__ void pt_megakernel<MRT_ONE_LDS != 0, MRT_ONE_THREADS, (MRT_ONE_INST), TileList>(const Params, const u32 *__restrict__, const TileList);
#else
template __global__ void pt_megakernel<MRT_ONE_LDS != 0, MRT_ONE_THREADS, (MRT_ONE_INST)>(const Params, const u32 *__restrict__);
#endif

}  // namespace mrt
