// TEST INFRASTRUCTURE: the band planner of the launch policy (mrt_plan.cpp plan_bands) and the MRT_BANDS knob (Knobs::from_env)
// on the host, for tests/test_bands_host.py.  No device, no HIP: mrt_plan.cpp is plain C++ and is compiled into the probe.
#include <stdint.h>
#include <stdlib.h>

#include "../../micro_raytracer_amd/csrc/mrt_plan.cpp"

extern "C" {

// The bands of a launch of n_chunks chunks over `tiles` wave tiles on `slots` resident wavefronts, under MRT_BANDS = bands
// (NULL: unset).  out: [0] listed bands  [1] tail  [2] items  [3..11) first  [11..19) len.  Returns the knob's entry count.
uint32_t bp_plan(uint32_t n_chunks, uint64_t tiles, uint64_t slots, const char *bands, uint32_t *out)
{
    if (bands) setenv("MRT_BANDS", bands, 1); else unsetenv("MRT_BANDS");
    const mrt::Knobs k = mrt::Knobs::from_env();
    unsetenv("MRT_BANDS");
    const mrt::Bands b = mrt::plan_bands(n_chunks, tiles, slots, k);
    out[0] = b.n; out[1] = b.tail; out[2] = b.items;
    for (uint32_t i = 0; i < mrt::kMaxBands; ++i) { out[3 + i] = b.first[i]; out[3 + mrt::kMaxBands + i] = b.len[i]; }
    return k.n_bands;
}

uint32_t bp_max_bands() { return mrt::kMaxBands; }

}  // extern "C"
