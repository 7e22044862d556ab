// Test-only C entry to plan_bcd (lrf_amd/csrc/lrf_plan.cpp) for tests/test_bcd_plan.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

enum { HEAD_INTS = 10, RUN_INTS = 15 };

// settings: persist, family_split_blocks, bcdw16_min_blocks, bcdw32_min_blocks (negative: the library's default), then the seven
// developer switches in PlanSettings' order, then persist_arch.  Returns the number of runs (at most max_runs are written).
extern "C" int lrf_test_plan_bcd(int nplanes, const int* M, const int* R, int K, int lo, int hi, int first_mode, int sweep, const long* settings,
                                 int* head, int* runs, int max_runs)
{
    Tables t;
    for (int i = 0; i < nplanes; i++) add_plane(t, 0, 0, 0, 0, 0, M[i], R[i], -1);
    PlanSettings s;
    s.persist = (int)settings[0];
    s.family_split_blocks = settings[1];
    if (settings[2] >= 0) s.bcdw16_min_blocks = settings[2];
    if (settings[3] >= 0) s.bcdw32_min_blocks = settings[3];
    s.bcd_wg = settings[4]; s.no_family_split = settings[5]; s.no_family_streams = settings[6]; s.no_bcdw32 = settings[7];
    s.generic_gs = settings[8]; s.no_persist_first = settings[9]; s.no_init_fork = settings[10];
    s.persist_arch = settings[11];
    const BcdPlan p = plan_bcd(t.planes, K, lo, hi, first_mode, s, sweep != 0);
    const int h[HEAD_INTS] = {p.persist, p.persist_f16, p.persist_np32, p.persist_first, (int)p.streams, p.mixed, p.split, p.rp, p.rmax, (int)t.blocks.size()};
    for (int i = 0; i < HEAD_INTS; i++) head[i] = h[i];
    for (int j = 0; j < (int)p.runs.size() && j < max_runs; j++) {
        const FamRun& r = p.runs[j];
        const int v[RUN_INTS] = {r.plane0, r.nplanes, r.block0, r.nblocks, r.rmin, r.rmax, r.fam, r.pitch, r.exact_int, (int)r.first.k, r.first.arg,
                                 (int)r.later.k, r.later.arg, r.nbase, r.any_native};
        for (int i = 0; i < RUN_INTS; i++) runs[j * RUN_INTS + i] = v[i];
    }
    return (int)p.runs.size();
}
