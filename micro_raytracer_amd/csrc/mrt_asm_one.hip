// mrt_asm_one.hip — ONE instantiation of pt_megakernel, for reading its assembly (`make asm-one INST=... THREADS=...`).
// Not part of libmrt_hip.so.  The kernel is the text of mrt_pt_kernel.h as mrt_kernels.hip includes it, so its code and its
// resource usage are the library's; only the other instantiations are missing (seconds instead of the minutes of `make asm`).
//   MRT_ONE_INST      the feature set, as the lists of mrt_megakernel.h spell it (default F_IDENT, the headline frame's kernel)
//   MRT_ONE_THREADS   the workgroup size, 64 / 256 / 512 / 1024 (default 256)
//   MRT_ONE_LDS       1: scene staged in LDS (default), 0: the scene-in-L2 kernel (256 threads)
#include <hip/hip_runtime.h>

#include "mrt_kernels.h"
#include "mrt_megakernel.h"
#include "mrt_post.h"
#include "mrt_trace.h"

#ifndef MRT_ONE_INST
#define MRT_ONE_INST F_IDENT
#endif
#ifndef MRT_ONE_THREADS
#define MRT_ONE_THREADS 256
#endif
#ifndef MRT_ONE_LDS
#define MRT_ONE_LDS 1
#endif

namespace mrt {

// the host side at the end of mrt_pt_kernel.h expands these lists: empty here, the kernel below is instantiated by name
#undef MRT_SHAPES_64
#undef MRT_SHAPES_256
#undef MRT_SHAPES_512
#undef MRT_SHAPES_1024
#undef MRT_SHAPES_L2
#define MRT_SHAPES_64
#define MRT_SHAPES_256
#define MRT_SHAPES_512
#define MRT_SHAPES_1024
#define MRT_SHAPES_L2

#define MRT_PT_LIST 0
#include "mrt_pt_kernel.h"
#undef MRT_PT_LIST

template __global__ void pt_megakernel<MRT_ONE_LDS != 0, MRT_ONE_THREADS, (MRT_ONE_INST)>(const Params, const u32 *__restrict__);

}  // namespace mrt
