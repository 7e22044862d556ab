// Test-only C entries to plan_encode_ragged_sweep (lrf_amd/csrc/lrf_plan.cpp) for tests/test_ragged_sweep_plan.py: built with the
// host compiler, no device.
#include <string.h>

#include "../lrf_amd/csrc/lrf_plan.h"

enum { PLANE_INTS = 11 };

static std::vector<EncSweepImage> images_of(int n, const long* H, const long* W, const long* rgb_off, const long* sign_off, const int* aligned8)
{
    std::vector<EncSweepImage> ims((size_t)n);
    for (int i = 0; i < n; i++) ims[(size_t)i] = EncSweepImage{H[i], W[i], rgb_off[i], sign_off[i], aligned8[i] != 0};
    return ims;
}
static std::vector<EncSweepCand> cands_of(int m, const int* image, const int* R, const long* u_off, const long* v_off)
{
    std::vector<EncSweepCand> cs((size_t)m);
    for (int j = 0; j < m; j++) cs[(size_t)j] = EncSweepCand{image[j], {R[3 * j], R[3 * j + 1], R[3 * j + 2]}, u_off[j], v_off[j]};
    return cs;
}

// Per image: H, W, rgb_off, sign_off, aligned8 (EncSweepImage); per candidate: image, R[3], u_off, v_off (EncSweepCand).
//   planes    per plane of the table, 3 m of them (cand, ch, x_off, u_off, v_off, M, R, sign_off, blk0, nblk, init_src)
//   x_offs    per image, where its matrices start in X
//   runs      per run of plan_bcd(sweep = true, K = 2, bounds (-16, 15)) (plane0, nplanes, nbase, fam), at most max_runs
//   out       (planes workgroups, BCD blocks of the plane table, split, x_floats, too_many, planes launches, runs)
// Returns 0, -1 when an output does not fit, -2 when the block table does not name every plane's blocks in order.
extern "C" int lrf_test_plan_ragged_sweep(int n, const long* H, const long* W, const long* rgb_off, const long* sign_off, const int* aligned8, int m,
                                          const int* image, const int* R, const long* u_off, const long* v_off, long family_split_blocks, long* planes,
                                          long* x_offs, long* runs, int max_runs, long* out)
{
    PlanSettings s;
    s.family_split_blocks = family_split_blocks;
    const EncRaggedSweepPlan p = plan_encode_ragged_sweep(images_of(n, H, W, rgb_off, sign_off, aligned8), cands_of(m, image, R, u_off, v_off), s);
    out[0] = (long)p.blocks.size();
    out[1] = (long)p.t.blocks.size();
    out[2] = p.split ? 1 : 0;
    out[3] = p.x_floats;
    out[4] = p.too_many;
    out[5] = (long)p.launches.size();
    out[6] = 0;
    if (p.too_many) return 0;
    if (p.t.planes.size() != 3 * (size_t)m || p.order.size() != 3 * (size_t)m || p.descs.size() != (size_t)n) return -1;
    for (int i = 0; i < n; i++) x_offs[i] = p.descs[(size_t)i].x_off;
    for (size_t j = 0; j < p.t.planes.size(); j++) {
        const PlaneDesc& pd = p.t.planes[j];
        const long v[PLANE_INTS] = {p.order[j].cand, p.order[j].ch, pd.x_off, pd.u_off, pd.v_off, pd.M, pd.R, pd.sign_off, pd.blk0, pd.nblk, pd.init_src};
        for (int i = 0; i < PLANE_INTS; i++) planes[j * PLANE_INTS + i] = v[i];
        if (pd.gram_fused) return -2;
        for (int b = 0; b < pd.nblk; b++) {
            const BlockDesc& bd = p.t.blocks[(size_t)pd.blk0 + (size_t)b];
            if (bd.plane != (int)j || bd.blk != b || bd.row0 != b * LRF_KC) return -2;
        }
    }
    const BcdPlan bcd = plan_bcd(p.t.planes, 2, -16, 15, PLAN_FIRST_W0, s, true);
    if ((int)bcd.runs.size() > max_runs || bcd.split != p.split) return -1;
    out[6] = (long)bcd.runs.size();
    for (size_t r = 0; r < bcd.runs.size(); r++) {
        const long v[4] = {bcd.runs[r].plane0, bcd.runs[r].nplanes, bcd.runs[r].nbase, bcd.runs[r].fam};
        for (int i = 0; i < 4; i++) runs[4 * r + i] = v[i];
    }
    return 0;
}

// One candidate per image, in image order (n = m, image[j] = j): the tables against plan_encode_ragged's for the same list, field by
// field.  Returns 0 when all agree, else the number of the first group of fields that differs.
extern "C" int lrf_test_ragged_sweep_equals_ragged(int n, const long* H, const long* W, const long* rgb_off, const long* sign_off, const int* aligned8,
                                                   const int* R, const long* u_off, const long* v_off, long family_split_blocks)
{
    PlanSettings s;
    s.family_split_blocks = family_split_blocks;
    std::vector<int> image((size_t)n);
    std::vector<EncRaggedImage> ims((size_t)n);
    for (int i = 0; i < n; i++) {
        image[(size_t)i] = i;
        ims[(size_t)i] = EncRaggedImage{H[i], W[i], {R[3 * i], R[3 * i + 1], R[3 * i + 2]}, rgb_off[i], u_off[i], v_off[i], sign_off[i], aligned8[i] != 0};
    }
    const EncRaggedSweepPlan a = plan_encode_ragged_sweep(images_of(n, H, W, rgb_off, sign_off, aligned8), cands_of(n, image.data(), R, u_off, v_off), s);
    const EncRaggedPlan b = plan_encode_ragged(ims, s);
    if (a.too_many != b.too_many || a.split != b.split || a.x_floats != b.x_floats) return 1;
    if (a.descs.size() != b.descs.size() || memcmp((const void*)a.descs.data(), (const void*)b.descs.data(), a.descs.size() * sizeof(EncRaggedDesc)) != 0) return 2;
    if (a.launches.size() != b.launches.size()) return 3;
    for (size_t j = 0; j < a.launches.size(); j++) {
        const EncRaggedLaunch &x = a.launches[j], &y = b.launches[j];
        if (x.body != y.body || x.block0 != y.block0 || x.nblocks != y.nblocks || x.xcd_chunk != y.xcd_chunk) return 3;
    }
    if (a.blocks.size() != b.blocks.size()) return 4;
    for (size_t j = 0; j < a.blocks.size(); j++)
        if (a.blocks[j].image != b.blocks[j].image || a.blocks[j].tile != b.blocks[j].tile) return 4;
    if (a.order.size() != b.order.size() || a.t.planes.size() != b.t.planes.size()) return 5;
    for (size_t j = 0; j < a.order.size(); j++)
        if (a.order[j].cand != b.order[j].image || a.order[j].ch != b.order[j].ch) return 5;
    for (size_t j = 0; j < a.t.planes.size(); j++) {
        const PlaneDesc &x = a.t.planes[j], &y = b.t.planes[j];
        if (x.x_off != y.x_off || x.u_off != y.u_off || x.v_off != y.v_off || x.u0_off != y.u0_off || x.v0_off != y.v0_off || x.M != y.M || x.R != y.R ||
            x.blk0 != y.blk0 || x.nblk != y.nblk || x.native_t2_u != y.native_t2_u || x.sign_off != y.sign_off || x.gch0 != y.gch0 || x.ngch != y.ngch ||
            x.init_src != y.init_src || x.gram_fused != y.gram_fused)
            return 6;
    }
    if (a.t.blocks.size() != b.t.blocks.size()) return 7;
    for (size_t j = 0; j < a.t.blocks.size(); j++) {
        const BlockDesc &x = a.t.blocks[j], &y = b.t.blocks[j];
        if (x.plane != y.plane || x.row0 != y.row0 || x.blk != y.blk || x.pad != y.pad) return 7;
    }
    return 0;
}
