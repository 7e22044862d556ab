// Test-only C entries to describe_images and geom_of (lrf_amd/csrc/lrf_plan.cpp) for tests/test_decode_images_host.py: built with
// the host compiler, no device.
#include <string.h>

#include "../lrf_amd/csrc/lrf_plan.h"

extern "C" long lrf_test_sizeof_ragged_desc() { return (long)sizeof(RaggedDesc); }

// refusal: (check, image, a, b).  descs: room for n descriptors, filled with their bytes when the list is accepted; work: null, or
// room for (kind, cls, units) per image.  The vectors start out filled with 0xFF bytes, so that the zeroing is describe_images'.
// Returns the refusal's check (DESC_OK = 0: accepted).
extern "C" int lrf_test_describe_images(long n, const lrf_ragged_image* images, long u_len, long v_len, int check_rgb, long rgb_len, int aligned8,
                                        unsigned long rgb_base, int no_tiled, long* refusal, void* descs, long* work)
{
    DescribeOptions o;
    o.check_rgb = check_rgb != 0;
    o.rgb_len = rgb_len;
    o.aligned8 = aligned8 != 0;
    o.rgb_base = (uintptr_t)rgb_base;
    o.no_tiled = no_tiled != 0;
    std::vector<RaggedDesc> d((size_t)n);
    memset((void*)d.data(), 0xFF, d.size() * sizeof(RaggedDesc));
    std::vector<RaggedWork> w((size_t)n, RaggedWork{-1, -1, -1});
    const DescribeRefusal r = describe_images(n, images, u_len, v_len, o, d, work ? &w : nullptr);
    refusal[0] = r.check; refusal[1] = r.image; refusal[2] = r.a; refusal[3] = r.b;
    if (r.check != DESC_OK) return r.check;
    if ((long)d.size() != n || (work && (long)w.size() != n)) return -1;
    if (descs) memcpy(descs, d.data(), d.size() * sizeof(RaggedDesc));
    for (long i = 0; work && i < n; i++) {
        work[3 * i] = w[(size_t)i].kind;
        work[3 * i + 1] = w[(size_t)i].cls;
        work[3 * i + 2] = w[(size_t)i].units;
    }
    return DESC_OK;
}

extern "C" int lrf_test_geom_of(long H, long W, void* geom)
{
    ImageGeom g;
    memset((void*)&g, 0, sizeof(g));
    int64_t bh, bw;
    const int bad = geom_of(H, W, &g, &bh, &bw);
    memcpy(geom, &g, sizeof(g));
    return bad;
}
