// Test-only C entry to plan_encode_ragged (lrf_amd/csrc/lrf_plan.cpp) for tests/test_encode_ragged_plan.py: built with the host
// compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

enum { LAUNCH_INTS = 4, DESC_INTS = 6, PLANE_INTS = 10 };

// Per image: H, W, R[3], rgb_off, u_off, v_off, sign_off, aligned8 (EncRaggedImage).  family_split_blocks: PlanSettings (-1: the default).
//   launches  (body, block0, nblocks, xcd_chunk) per launch, at most max_launches; blocks: (image, unit) per workgroup, at most max_blocks
//   descs     per image (body, per_strip, x_off, rgb_off, H, W)
//   planes    per plane of the table, 3 n of them (image, ch, x_off, u_off, v_off, M, R, sign_off, blk0, nblk)
//   out       (nblocks of the workgroup table, BCD blocks of the plane table, split, x_floats, too_many)
// Returns the number of launches, or -1 when an output does not fit.
extern "C" int lrf_test_plan_encode_ragged(int n, const long* H, const long* W, const int* R, const long* rgb_off, const long* u_off, const long* v_off,
                                           const long* sign_off, const int* aligned8, long family_split_blocks, long* launches, int max_launches,
                                           int* blocks, long max_blocks, long* descs, long* planes, long* out)
{
    std::vector<EncRaggedImage> ims((size_t)n);
    for (int i = 0; i < n; i++)
        ims[(size_t)i] = EncRaggedImage{H[i], W[i], {R[3 * i], R[3 * i + 1], R[3 * i + 2]}, rgb_off[i], u_off[i], v_off[i], sign_off[i], aligned8[i] != 0};
    PlanSettings s;
    s.family_split_blocks = family_split_blocks;
    const EncRaggedPlan p = plan_encode_ragged(ims, s);
    out[0] = (long)p.blocks.size();
    out[1] = (long)p.t.blocks.size();
    out[2] = p.split ? 1 : 0;
    out[3] = p.x_floats;
    out[4] = p.too_many;
    if ((int)p.launches.size() > max_launches || (long)p.blocks.size() > max_blocks) return -1;
    if (p.too_many) return 0;
    for (size_t j = 0; j < p.launches.size(); j++) {
        const EncRaggedLaunch& l = p.launches[j];
        const long v[LAUNCH_INTS] = {l.body, l.block0, l.nblocks, l.xcd_chunk};
        for (int i = 0; i < LAUNCH_INTS; i++) launches[j * LAUNCH_INTS + i] = v[i];
    }
    for (size_t j = 0; j < p.blocks.size(); j++) {
        blocks[2 * j] = p.blocks[j].image;
        blocks[2 * j + 1] = p.blocks[j].tile;
    }
    for (size_t j = 0; j < p.descs.size(); j++) {
        const EncRaggedDesc& d = p.descs[j];
        const long v[DESC_INTS] = {d.body, d.per_strip, d.x_off, d.rgb_off, d.H, d.W};
        for (int i = 0; i < DESC_INTS; i++) descs[j * DESC_INTS + i] = v[i];
    }
    for (size_t j = 0; j < p.t.planes.size(); j++) {
        const PlaneDesc& pd = p.t.planes[j];
        const long v[PLANE_INTS] = {p.order[j].image, p.order[j].ch, pd.x_off, pd.u_off, pd.v_off, pd.M, pd.R, pd.sign_off, pd.blk0, pd.nblk};
        for (int i = 0; i < PLANE_INTS; i++) planes[j * PLANE_INTS + i] = v[i];
    }
    // the block table must name every plane's blocks in order: checked here, where the table is
    for (size_t j = 0; j < p.t.planes.size(); j++)
        for (int b = 0; b < p.t.planes[j].nblk; b++) {
            const BlockDesc& bd = p.t.blocks[(size_t)p.t.planes[j].blk0 + (size_t)b];
            if (bd.plane != (int)j || bd.blk != b || bd.row0 != b * LRF_KC) return -2;
        }
    return (int)p.launches.size();
}
