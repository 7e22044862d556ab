// Test-only C entry to plan_decode_ragged (lrf_amd/csrc/lrf_plan.cpp) for tests/test_decode_ragged_plan.py: built with the host
// compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

enum { LAUNCH_INTS = 5 };

// kind / cls / units: one entry per image (RaggedWork).  launches: (kind, cls, block0, nblocks, reps) per launch, at most
// max_launches of them; blocks: (image, tile) per workgroup, at most max_blocks.  too_many: RaggedPlan::too_many.
// Returns the number of launches, or -1 when an output does not fit.
extern "C" int lrf_test_plan_decode_ragged(int n, const int* kind, const int* cls, const long* units, long* launches, int max_launches, int* blocks,
                                           long max_blocks, long* nblocks, long* too_many)
{
    std::vector<RaggedWork> w((size_t)n);
    for (int i = 0; i < n; i++) w[(size_t)i] = RaggedWork{kind[i], cls[i], units[i]};
    const RaggedPlan p = plan_decode_ragged(w);
    *too_many = p.too_many;
    *nblocks = (long)p.blocks.size();
    if ((int)p.launches.size() > max_launches || (long)p.blocks.size() > max_blocks) return -1;
    for (size_t j = 0; j < p.launches.size(); j++) {
        const RaggedLaunch& l = p.launches[j];
        const long v[LAUNCH_INTS] = {l.kind, l.cls, l.block0, l.nblocks, l.reps};
        for (int i = 0; i < LAUNCH_INTS; i++) launches[j * LAUNCH_INTS + i] = v[i];
    }
    for (size_t j = 0; j < p.blocks.size(); j++) {
        blocks[2 * j] = p.blocks[j].image;
        blocks[2 * j + 1] = p.blocks[j].tile;
    }
    return (int)p.launches.size();
}

// decode_plan of an H x W image at ranks (r0, r1, r2): kind * 8 + cls, or -(what geom_of answers) when it refuses the size
extern "C" int lrf_test_decode_plan(long H, long W, int r0, int r1, int r2, int aligned8, int no_tiled)
{
    ImageGeom g;
    int64_t bh, bw;
    const int bad = geom_of(H, W, &g, &bh, &bw);
    if (bad) return -bad;
    const int R[3] = {r0, r1, r2};
    const DecodePlan p = decode_plan(g, H, W, R, aligned8 != 0, no_tiled != 0);
    return p.kind * 8 + p.cls;
}
