// Test-only C entries for tests/test_x_residency_plan.py: which X of a k_bcd_p call stays on the default cache policy and which
// blocks stream non-temporal (plan_x_residency, lrf_amd/csrc/lrf_plan.cpp).  Built with the host compiler, no device.
#include <string.h>

#include "../lrf_amd/csrc/lrf_plan.h"

static_assert(sizeof(BlockDesc) == 16 && sizeof(PlaneDesc) == 80, "the table layouts the test writes out by hand");

// plan_bcd on the planes (M, R) with LRF_PERSIST = persist on the validated device, then — when `apply` — plan_x_residency with
// a budget of keep_bytes, the first nluma planes being the images' luma planes (read from the image bytes or from fp32 X).  Out: the block table's bytes [nblocks][16], the
// plane table's [nplanes][80], the decision {policy on, kept planes} and the kept bytes.  Returns the number of blocks.
extern "C" int lrf_test_plan_x_residency(int nplanes, const int* M, const int* R, int K, int first_mode, int persist, int nluma, int luma_from_bytes,
                                         int piped,
                                         long keep_bytes, int apply, unsigned char* blocks_out, unsigned char* planes_out, int* decision,
                                         long* kept_bytes)
{
    Tables t;
    for (int i = 0; i < nplanes; i++) add_plane(t, 0, 0, 0, 0, 0, M[i], R[i], -1);
    PlanSettings s;
    s.persist = persist;
    s.persist_arch = true;
    s.x_keep_bytes = keep_bytes;
    const BcdPlan p = plan_bcd(t.planes, K, -16, 15, first_mode, s);
    decision[0] = decision[1] = 0;
    *kept_bytes = 0;
    if (apply) {
        const XResidency x = plan_x_residency(p, t, nluma, luma_from_bytes != 0, piped != 0, s);
        decision[0] = x.on ? 1 : 0;
        decision[1] = x.kept_planes;
        *kept_bytes = x.kept_bytes;
    }
    memcpy(blocks_out, t.blocks.data(), t.blocks.size() * sizeof(BlockDesc));
    memcpy(planes_out, t.planes.data(), t.planes.size() * sizeof(PlaneDesc));
    return (int)t.blocks.size();
}

// LRF_X_KEEP_MB as the library reads it (once per process)
extern "C" long lrf_test_env_x_keep_bytes() { return plan_settings_env().x_keep_bytes; }
