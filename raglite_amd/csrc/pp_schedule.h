// Workgroup -> (row range, pass) of the sixteen-query MaxSim pass (maxsim_pp.hip MODE 0).  Plain C++ with no HIP dependency, so that
// tests/test_pp_schedule.py compiles this same code on the host and checks it is a bijection.
//
// A launch covers `passes` passes (16 queries each) over `ranges` chunk-aligned row ranges.  Two grid shapes:
//   * pass-major (RL_OPT_PP_SCHEDULE = 0): grid (ranges, passes), range = blockIdx.x, pass = blockIdx.y.  The hardware dispatches x first,
//     so one pass fills the GPU, and each pass streams the whole image from HBM again: passes x the image's bytes per launch;
//   * co-scheduled (1): a 1-D grid of ranges x passes.  Within each block of 8 x passes consecutive ids, range = 8 (id / (8 passes)) + id % 8
//     and pass = (id / 8) % passes.  The passes over one range get ids that are equal mod 8 and close together, and workgroups are dealt
//     round-robin over the 8 XCDs, so they run at the same time on the same XCD and one HBM read of a corpus slab serves all of them through
//     that XCD's L2.  That is a speed property only: nothing depends on where or in which order the workgroups run.  The last ranges % 8
//     ranges, which do not fill a block of eight, keep the pass-major order among themselves.
// With one pass both shapes are the same grid.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RL_PP_HD __host__ __device__
#else
#define RL_PP_HD
#endif

namespace rl {

struct PpSlot {
    int32_t ranges;  // row ranges of the launch (the kernel's G)
    int32_t range;   // this workgroup's row range (b)
    int32_t pass;    // this workgroup's pass (queries 16 pass .. 16 pass + 15)
};

// (x, y) = blockIdx, (gx, gy) = gridDim of a launch of `passes` passes.  A grid of one row with passes > 1 is the co-scheduled shape.
RL_PP_HD inline PpSlot pp_schedule(int32_t x, int32_t y, int32_t gx, int32_t gy, int32_t passes) {
    if (gy > 1 || passes <= 1) return PpSlot{gx, x, y};
    const int32_t ranges = gx / passes;
    const int32_t whole = ranges & ~7, head = whole * passes;  // ranges in whole blocks of eight, and their ids
    if (x < head) return PpSlot{ranges, 8 * (x / (8 * passes)) + x % 8, (x / 8) % passes};
    const int32_t t = x - head, rest = ranges - whole;
    return PpSlot{ranges, whole + t % rest, t / rest};
}

}  // namespace rl
