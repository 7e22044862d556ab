// Test-only C entries to describe_gray_encode and plan_encode_gray_ragged_sweep (lrf_amd/csrc/lrf_plan.cpp) for
// tests/test_gray_encode_plan.py: built with the host compiler, no device.
#include <string.h>

#include "../lrf_amd/csrc/lrf_plan.h"

enum { PLANE_INTS = 10, DESC_INTS = 8 };

// The list as a caller of lrf_qmf_encode_gray_ragged_sweep_u8 hands it over -> out: (check, candidate, index, a, b, images
// built, candidates built, then per accepted image aligned16 and sign_off at out[7 + 2 i], out[8 + 2 i])
// n, m: the counts the call names; n_have, m_have: the entries the arrays hold (a refused count is never read past them)
extern "C" void lrf_test_describe_gray_encode(long n, long n_have, const long* H, const long* W, const long* gray_off, const long* sign_off, long m,
                                              long m_have, const int* image, const int* R, const long* u_off, const long* v_off, long gray_len, long sign_len, long u_len, long v_len,
                                              long gray_base, int K, int lo, int hi, long* out)
{
    std::vector<lrf_gray_sweep_image> ims((size_t)n_have);
    std::vector<lrf_gray_sweep_candidate> cds((size_t)m_have);
    for (size_t i = 0; i < ims.size(); i++) ims[i] = lrf_gray_sweep_image{H[i], W[i], gray_off[i], sign_off[i]};
    for (size_t j = 0; j < cds.size(); j++) cds[j] = lrf_gray_sweep_candidate{image[j], R[j], u_off[j], v_off[j]};
    const GrayEncCall k = {gray_len, sign_len, u_len, v_len, (uintptr_t)gray_base, K, lo, hi};
    std::vector<EncGrayImage> eims;
    std::vector<EncGrayCand> ecs;
    const GrayEncRefusal r = describe_gray_encode(n, ims.data(), m, cds.data(), k, eims, ecs);
    const long v[7] = {r.check, r.candidate, (long)r.index, (long)r.a, (long)r.b, (long)eims.size(), (long)ecs.size()};
    for (int i = 0; i < 7; i++) out[i] = v[i];
    for (size_t i = 0; i < eims.size(); i++) {
        out[7 + 2 * i] = eims[i].aligned16 ? 1 : 0;
        out[8 + 2 * i] = eims[i].sign_off;
    }
}

// Per image: H, W, gray_off, sign_off, aligned16 (EncGrayImage); per candidate: image, R, u_off, v_off (EncGrayCand).
//   planes    per plane of the table, m of them (cand, x_off, u_off, v_off, M, R, sign_off, blk0, nblk, init_src)
//   descs     per image (gray_off, x_off, H, W, top, left, nw, items)
//   launches  per planes launch (body, block0, nblocks), at most two
//   blocks    the workgroup table (image, tile), at most max_blocks entries
//   runs      per run of plan_bcd(sweep = m > n, K = 2, bounds (-16, 15)) (plane0, nplanes, nbase, fam), at most max_runs
//   out       (planes workgroups, BCD blocks of the plane table, split, x_floats, too_many, planes launches, runs)
// Returns 0, -1 when an output does not fit, -2 when the block table does not name every plane's blocks in order.
extern "C" int lrf_test_plan_gray_encode(int n, const long* H, const long* W, const long* gray_off, const long* sign_off, const int* aligned16, int m,
                                         const int* image, const int* R, const long* u_off, const long* v_off, long family_split_blocks, long* planes,
                                         long* descs, long* launches, long* blocks, long max_blocks, long* runs, int max_runs, long* out)
{
    PlanSettings s;
    s.family_split_blocks = family_split_blocks;
    std::vector<EncGrayImage> ims((size_t)n);
    std::vector<EncGrayCand> cs((size_t)m);
    for (int i = 0; i < n; i++) ims[(size_t)i] = EncGrayImage{H[i], W[i], gray_off[i], sign_off[i], aligned16[i] != 0};
    for (int j = 0; j < m; j++) cs[(size_t)j] = EncGrayCand{image[j], R[j], u_off[j], v_off[j]};
    const EncGraySweepPlan p = plan_encode_gray_ragged_sweep(ims, cs, s);
    out[0] = (long)p.blocks.size();
    out[1] = (long)p.t.blocks.size();
    out[2] = p.split ? 1 : 0;
    out[3] = p.x_floats;
    out[4] = p.too_many;
    out[5] = (long)p.launches.size();
    out[6] = 0;
    if (p.too_many) return (p.blocks.empty() && p.descs.empty() && p.t.planes.empty() && p.launches.empty() && p.order.empty()) ? 0 : -3;
    if (p.t.planes.size() != (size_t)m || p.order.size() != (size_t)m || p.descs.size() != (size_t)n || p.rmax.size() != (size_t)n) return -1;
    if ((long)p.blocks.size() > max_blocks || p.launches.size() > 2) return -1;
    for (int i = 0; i < n; i++) {
        const EncGrayDesc& d = p.descs[(size_t)i];
        const long v[DESC_INTS] = {d.gray_off, d.x_off, d.H, d.W, d.top, d.left, d.nw, d.items};
        for (int k = 0; k < DESC_INTS; k++) descs[i * DESC_INTS + k] = v[k];
    }
    for (size_t l = 0; l < p.launches.size(); l++) {
        launches[3 * l] = p.launches[l].body;
        launches[3 * l + 1] = p.launches[l].block0;
        launches[3 * l + 2] = p.launches[l].nblocks;
    }
    for (size_t b = 0; b < p.blocks.size(); b++) {
        blocks[2 * b] = p.blocks[b].image;
        blocks[2 * b + 1] = p.blocks[b].tile;
    }
    for (size_t j = 0; j < p.t.planes.size(); j++) {
        const PlaneDesc& pd = p.t.planes[j];
        const long v[PLANE_INTS] = {p.order[j], pd.x_off, pd.u_off, pd.v_off, pd.M, pd.R, pd.sign_off, pd.blk0, pd.nblk, pd.init_src};
        for (int i = 0; i < PLANE_INTS; i++) planes[j * PLANE_INTS + i] = v[i];
        if (pd.gram_fused) return -2;
        for (int b = 0; b < pd.nblk; b++) {
            const BlockDesc& bd = p.t.blocks[(size_t)pd.blk0 + (size_t)b];
            if (bd.plane != (int)j || bd.blk != b || bd.row0 != b * LRF_KC) return -2;
        }
    }
    const BcdPlan bcd = plan_bcd(p.t.planes, 2, -16, 15, PLAN_FIRST_W0, s, m > n);
    if ((int)bcd.runs.size() > max_runs || bcd.split != p.split) return -1;
    out[6] = (long)bcd.runs.size();
    for (size_t r = 0; r < bcd.runs.size(); r++) {
        const long v[4] = {bcd.runs[r].plane0, bcd.runs[r].nplanes, bcd.runs[r].nbase, bcd.runs[r].fam};
        for (int i = 0; i < 4; i++) runs[4 * r + i] = v[i];
    }
    return 0;
}
