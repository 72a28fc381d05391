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
//   * XCD-affine (RL_OPT_PP_SCHEDULE = 1 with RL_OPT_PP_XCD_PASSES = w in {4, 2, 1}): the same 1-D grid in another order, pp_schedule_affine
//     below.  The co-scheduled order runs ALL passes over a few ranges on an XCD, so the query fragments of all passes (1 MiB each) cycle
//     through that XCD's 4-MiB L2.  Here an XCD serves only w passes per block of eight passes, for the whole launch, and the eight XCDs
//     walk the row ranges in the same order at the same time: the XCD's query image (w MiB) stays in its L2, and a corpus slab is read by
//     8 / w XCDs within a few tiles of each other (one HBM read, the others from the Infinity Cache).
// With one pass all shapes are the same grid.
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

// The XCD-affine order of the 1-D grid (gx = ranges x passes ids, G = ranges), w = passes that share an XCD at a time.  Inside each block of
// eight passes (8 G consecutive ids), with S = 8 / w:
//     blk = id / (8 G);  l = id % (8 G);  x = l % 8;  n = l / 8;  s = x % S;  j = x / S
//     pass = 8 blk + w s + n % w;   range = w (n / w) + j
// Slot x (ids equal mod 8: one XCD under round-robin dealing) serves passes w s .. w s + w - 1 only; sequence number n names the same
// ranges on every slot, so the XCDs stay in step.  Again a speed property only: no workgroup waits for another.
// What falls back to the co-scheduled map of pp_schedule():
//   * the whole launch when w is not 1, 2 or 4 (w = 8 IS the co-scheduled order), when ranges % w != 0, or with fewer than eight passes
//     (pp_affine_blocks() == 0);
//   * the trailing passes % 8 passes of a longer launch: their ids (from 8 G pp_affine_blocks() on) take the co-scheduled map of a launch
//     of those passes alone.
RL_PP_HD inline int32_t pp_affine_blocks(int32_t ranges, int32_t passes, int32_t w) {  // blocks of eight passes in the affine order
    return ((w == 1 || w == 2 || w == 4) && ranges > 0 && ranges % w == 0) ? passes / 8 : 0;
}
RL_PP_HD inline PpSlot pp_schedule_affine(int32_t x, int32_t gx, int32_t passes, int32_t w) {
    const int32_t ranges = passes > 0 ? gx / passes : gx;
    const int32_t blocks = pp_affine_blocks(ranges, passes, w), head = 8 * ranges * blocks;
    if (blocks == 0) return pp_schedule(x, 0, gx, 1, passes);
    if (x >= head) {  // trailing passes: co-scheduled among themselves
        const int32_t rest = passes - 8 * blocks;
        const PpSlot m = pp_schedule(x - head, 0, ranges * rest, 1, rest);
        return PpSlot{ranges, m.range, 8 * blocks + m.pass};
    }
    const int32_t S = 8 / w, blk = x / (8 * ranges), l = x % (8 * ranges), slot = l % 8, n = l / 8, s = slot % S, j = slot / S;
    return PpSlot{ranges, w * (n / w) + j, 8 * blk + w * s + n % w};
}

}  // namespace rl
