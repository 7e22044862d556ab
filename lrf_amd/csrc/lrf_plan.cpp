// lrf_plan.cpp — the launch plan of a call of the 64-column path (lrf_plan.h): every rule that picks a kernel, the persistent
// launch or a stream layout lives in plan_bcd, every bound is written once.  Host C++ only.
#include "lrf_plan.h"

#include <math.h>
#include <algorithm>
#include <array>
#include <string.h>

#include "lrf_env.h"

void add_plane(Tables& t, long x_off, long u_off, long v_off, long u0_off, long v0_off, int M, int R, int sign_off)
{
    PlaneDesc pd;
    memset(&pd, 0, sizeof(pd));
    pd.x_off = x_off; pd.u_off = u_off; pd.v_off = v_off; pd.u0_off = u0_off; pd.v0_off = v0_off;
    pd.M = M; pd.R = R;
    pd.blk0 = (int)t.blocks.size();
    pd.nblk = (M + LRF_KC - 1) / LRF_KC;
    pd.native_t2_u = ((long)(R - 1) * M < 400) ? 1 : 0;
    pd.sign_off = sign_off;
    int pi = (int)t.planes.size();
    pd.init_src = pi; // (a sweep call's table builder points the lower-rank planes of a matrix at its largest-rank plane)
    for (int b = 0; b < pd.nblk; b++) t.blocks.push_back(BlockDesc{pi, b * LRF_KC, b, 0});
    pd.gch0 = 0; // the Gram chunks are cut when the table is complete (finish_gram_chunks)
    pd.ngch = 0;
    t.planes.push_back(pd);
}

const PlanSettings& plan_settings_env()
{
    static const PlanSettings s{(int)env_long("LRF_PERSIST", -1), env_long("LRF_FAMILY_SPLIT_BLOCKS", -1),
                                env_long("LRF_BCDW16_MIN_BLOCKS", LRF_BCDW16_MIN_BLOCKS), env_long("LRF_BCDW32_MIN_BLOCKS", LRF_BCDW32_MIN_BLOCKS),
                                dev_flag("LRF_BCD_WG"), dev_flag("LRF_NO_FAMILY_SPLIT"), dev_flag("LRF_NO_FAMILY_STREAMS"), dev_flag("LRF_NO_BCDW32"),
                                dev_flag("LRF_GENERIC_GS"), dev_flag("LRF_NO_PERSIST_FIRST"), dev_flag("LRF_NO_INIT_FORK"), false,
                                (int)env_long("LRF_LUMA_BYTES", -1), env_long("LRF_X_KEEP_MB", LRF_X_KEEP_MB_DEFAULT) * 1000000L};
    return s;
}

XResidency plan_x_residency(const BcdPlan& p, Tables& t, int nluma, bool luma_from_bytes, bool piped, const PlanSettings& s)
{
    XResidency x;
    for (BlockDesc& b : t.blocks) b.x_nt = 0;
    if (s.x_keep_bytes <= 0 || piped || !p.persist || p.persist_f16 || p.persist_np32 != 0) return x;
    const int np = (int)t.planes.size();
    // a call whose sources all fit stays as it is: passes 2..K find every one of them in the cache, and a non-temporal load
    // would give that up (96 x 512x768, 189 MB: 0.845 -> 0.855 ms with luma streamed, 0.865 with everything streamed)
    long total = 0;
    for (int pi = 0; pi < np; pi++) total += (long)t.planes[(size_t)pi].M * 64 * (pi < nluma && luma_from_bytes ? 3L : (long)sizeof(float));
    if (total <= s.x_keep_bytes) return x;
    x.on = true;
    bool full = false; // (a plane that does not fit ends the kept run: the planes behind it stream, as it does)
    for (int pi = 0; pi < np; pi++) {
        const PlaneDesc& pd = t.planes[(size_t)pi];
        const long bytes = (long)pd.M * 64 * (long)sizeof(float);
        const bool keep = pi >= nluma && !full && x.kept_bytes + bytes <= s.x_keep_bytes;
        if (pi >= nluma && !keep) full = true;
        if (keep) {
            x.kept_planes++;
            x.kept_bytes += bytes;
        } else
            for (int b = 0; b < pd.nblk; b++) t.blocks[(size_t)(pd.blk0 + b)].x_nt = 1;
    }
    return x;
}

bool plan_luma_bytes(const BcdPlan& p, const std::vector<PlaneDesc>& planes, int nluma, int64_t H, int64_t W, uintptr_t rgb_addr, bool rgb_released,
                     const PlanSettings& s)
{
    if (s.luma_bytes == 0 || rgb_released) return false;
    if (H < 16 || W < 16 || H % 16 != 0 || W % 16 != 0 || (rgb_addr & 7) != 0 || (long)H * W * 3 >= (1L << 31)) return false;
    if (!p.persist || !p.persist_first || p.persist_f16 || p.persist_np32 != 0) return false;
    if (nluma < 1 || nluma > (int)planes.size()) return false;
    for (int i = 0; i < nluma; i++)
        if (fam_of_rank(planes[i].R) != 0 || planes[i].M != (H / 8) * (W / 8)) return false;
    return true;
}

// A small call takes ONE family, the one its largest rank needs: its launches are latency chains per block and a second launch
// per iteration costs more than a faster kernel saves.  Since the families of a call run side by side on streams of their own
// (round 3) — or in one persistent launch (round 5) — the split pays from 1024 blocks on (64 x 512x768: (16,8,8) 0.93 -> 0.89 ms,
// (20,10,10) 2.04 -> 1.36 with k_bcd_w32 on the luma run; 256 images: (16,8,8) 4.05 -> 3.78 ms); calls with a rank above 16
// split from 256 blocks (24 images: (20,10,10) 1.27 -> 1.04 ms, 12 images 1.06 -> 0.99).
bool plan_splits(long nblocks, int rmax_t, const PlanSettings& s)
{
    const long min_blocks = s.family_split_blocks >= 0 ? s.family_split_blocks : (rmax_t > 16 ? 256 : 1024);
    return !s.no_family_split && !s.bcd_wg && rmax_t <= LRF_BIG_TO_ANY_RANK && nblocks >= min_blocks;
}

// What the wave kernel of a run's family asks of the numbers (its size thresholds and switches: bcd_kernel), by the mode of
// the U update — 0: iterations >= 2 (old U from int8); 1: the first, old U = X W0; 2: the first, old U = the caller's U0.
//   mode 0: every term and partial sum of `uu @ bb` is an exact integer in fp32 for the largest rank of the run (exact_int:
//           (R - 1) 64 mx^3 < 2^24), so the order of that sum is immaterial, which lets ranks 9..16 (gs_row_lds) and 17..32
//           (k_bcd_w32) replace the reference's dependent chain by independent fmas, bit for bit; ranks 17..32 also need |b|
//           within int16 (64 mx^2 <= 32767): the lane = row Gauss-Seidel on int16 pairs;
//   mode 1: no plane small enough for ATen's native order of `uu @ bb`; ranks 17..32: one rank for the whole run (k_bcd_w32f).
// Ranks <= 8 (k_bcd_w) keep the reference's order: any bounds, any mode.
static bool wave_numbers_ok(const FamRun& r, int mode, bool int16_b)
{
    if (r.fam == 0) return true;
    if (mode == 0) return r.exact_int && (r.fam == 1 || int16_b);
    if (mode == 1) return !r.any_native && (r.fam == 1 || r.rmin == r.rmax);
    return false;
}

static BcdChoice bcd_kernel(const FamRun& r, int mode, bool int16_b, const PlanSettings& s)
{
    const bool ok = !s.bcd_wg && wave_numbers_ok(r, mode, int16_b);
    // k_bcd_w (one wave per block, no barriers) for rank <= 8 runs of LRF_BCDW_MIN_BLOCKS blocks or more: with fewer than a
    // wave per SIMD what counts is the latency of ONE block, and there the four waves of the workgroup kernel k_bcd share a
    // block's sub-tile (one 512x768 image: 27.9 -> 17.0 us per launch, 8 images 28.5 -> 18.2, 32 images 31.7 -> 27.6; equal at 48)
    if (r.fam == 0) return BcdChoice{ok && r.nblocks >= LRF_BCDW_MIN_BLOCKS ? BCD_K_W : BCD_K_WG8, 0};
    // ranks 9..16 (and the lower-rank planes of such a run)
    if (r.fam == 1) return BcdChoice{ok && r.nblocks >= s.bcdw16_min_blocks ? BCD_K_W16 : BCD_K_WG16, 0};
    // ranks 17..32: a run whose planes all have such ranks, else the workgroup kernel k_bcd_mid (small runs, wide bounds, caller's U0)
    if (!ok || s.no_bcdw32 || r.rmin < 17 || r.nblocks < s.bcdw32_min_blocks) return BcdChoice{BCD_K_MID, 0};
    return mode == 0 ? BcdChoice{BCD_K_W32, (r.rmax + 1) >> 1} : BcdChoice{BCD_K_W32F, r.rmax};
}

BcdPlan plan_bcd(const std::vector<PlaneDesc>& planes, int K, int lo, int hi, int first_mode, const PlanSettings& s, bool sweep)
{
    BcdPlan p;
    p.K = K; p.lo = lo; p.hi = hi; p.first_mode = first_mode;
    long nblocks = 0;
    for (const PlaneDesc& pd : planes) {
        p.rmax = pd.R > p.rmax ? pd.R : p.rmax;
        nblocks += pd.nblk;
    }
    p.rp = p.rmax <= 16 ? 16 : LRF_RPB;
    p.split = plan_splits(nblocks, p.rmax, s);
    // the runs: the planes of the fused encode are ordered by channel (a sweep's by family), so that is at most three
    int blk = 0;
    for (int pi = 0; pi < (int)planes.size(); pi++) {
        const PlaneDesc& pd = planes[pi];
        const int fam = p.split ? fam_of_rank(pd.R) : (p.rmax > 16 ? 2 : fam_of_rank(p.rmax));
        if (p.runs.empty() || p.runs.back().fam != fam)
            p.runs.push_back(FamRun{pi, 0, blk, 0, 1, fam, fam == 2 ? LRF_RPB : 16, pd.R, false, 0, false, {BCD_K_WG8, 0}, {BCD_K_WG8, 0}});
        FamRun& r = p.runs.back();
        r.any_native = r.any_native || pd.native_t2_u != 0;
        if (pd.init_src == pi && r.nbase == r.nplanes) r.nbase++; // (the table builders put a run's self-initialising planes first)
        r.nplanes++;
        r.nblocks += pd.nblk;
        r.rmax = pd.R > r.rmax ? pd.R : r.rmax;
        r.rmin = pd.R < r.rmin ? pd.R : r.rmin;
        blk += pd.nblk;
    }
    bool p16 = false, p64 = false;
    for (const FamRun& r : p.runs) (r.pitch == 16 ? p16 : p64) = true;
    p.mixed = p16 && p64;
    if (first_mode == PLAN_INIT_ONLY || p.rmax > LRF_BIG_TO_ANY_RANK) return p; // (ranks 33..64 iterate on the any-shape kernels)

    const long mx = bounds_mx(lo, hi);
    const bool int16_b = 64 * mx * mx <= 32767;
    for (FamRun& r : p.runs) {
        r.exact_int = !s.generic_gs && (long)(r.rmax - 1) * 64 * mx * mx * mx < (1L << 24);
        r.first = bcd_kernel(r, first_mode, int16_b, s);
        r.later = bcd_kernel(r, 0, int16_b, s);
    }

    // Iterations 2..K of a large call in ONE launch (k_bcd_p<F16, NP32>): the U updates of all iterations and planes pulled from
    // a queue, each matrix's V update done by the last of its blocks to finish.  The persistent kernel takes a call when
    //   * the device is the part its in-launch hand-offs were validated on (gfx950);
    //   * every plane sits on the kernel family of its own rank (the split plan) and the families' wave kernels accept the
    //     numbers for iterations >= 2 (wave_numbers_ok), with one pair count NP for all planes of ranks 17..32; no plane of
    //     ranks above 8 small enough for ATen's native order of `uu @ bb`;
    //   * the call has LRF_PERSIST_MIN_BLOCKS blocks or more (256 x 512x768 at ranks <= 8: 2.05 -> 1.92 ms per step; 48 / 64 such
    //     images lose 15 %: a round and a half of the 2048 wave slots; tools/dev_persist_threshold.py) — from
    //     LRF_PERSIST_MIN_BLOCKS_ONE_FAMILY when all planes are of one rank family (96 x 512x768: (7,3,3) 0.96 -> 0.92 ms, (12,12,12)
    //     1.25 -> 1.13, (20,20,20) 1.83 -> 1.72; calls that mix families lose at 96 and 128 images: tools/run_r05_o.sh).
    //     LRF_PERSIST=0 turns it off, =1 lowers the threshold to LRF_BCDW_MIN_BLOCKS (tests).
    bool persist = s.persist_arch && s.persist != 0 && !s.bcd_wg && K >= 2 && !p.runs.empty();
    bool f16 = false;
    int np32 = 0;
    for (const FamRun& r : p.runs) {
        if (fam_of_rank(r.rmin) != r.fam || fam_of_rank(r.rmax) != r.fam) persist = false; // a small call: one family for all planes
        if (r.fam == 0) continue;
        if (!wave_numbers_ok(r, 0, int16_b) || r.any_native) persist = false;
        if (r.fam == 1) {
            f16 = true;
        } else {
            const int np = (r.rmax + 1) >> 1;
            if (r.rmin < 2 * np - 1 || (np32 != 0 && np32 != np)) persist = false;
            np32 = np;
        }
    }
    const long min_blocks = p.runs.size() == 1 ? LRF_PERSIST_MIN_BLOCKS_ONE_FAMILY : LRF_PERSIST_MIN_BLOCKS;
    if (persist && nblocks >= (s.persist == 1 ? LRF_BCDW_MIN_BLOCKS : min_blocks)) {
        p.persist = true;
        p.persist_f16 = f16 || np32 != 0;
        p.persist_np32 = np32;
        // ... and the first iteration as well (k_bcd_p<.., 0, true>: ranks <= 16 only) when its old U is X @ W0 of the
        // initialisation just run: then the b tables are the last launch before k_bcd_p
        p.persist_first = np32 == 0 && !s.no_persist_first && first_mode == PLAN_FIRST_W0;
    }

    // Streams.  The runs touch disjoint planes, so the whole chain of a run — initialisation, b table, K x (U update, V update)
    // — is independent of the other runs': a call that initialises and iterates (first_mode 1) forks them for its whole length.
    // Not when its iterations run in the persistent kernel — one launch for all families, behind a first iteration whose family
    // kernels run one after the other (side by side they were SLOWER: k_bcd_w32f 305 us and k_bcd_w16<1> 80 us alone, 590 us
    // together) — and not in a sweep call, whose shared initialisations tie the families together: those fork for the
    // initialisation kernels only (run_init says why that pays).
    if (first_mode == PLAN_FIRST_W0 && !s.no_family_streams)
        p.streams = !(p.persist || sweep) ? FAM_STREAMS_CALL : (s.no_init_fork ? FAM_STREAMS_NONE : FAM_STREAMS_INIT);
    return p;
}

// ---- the any-shape path ---------------------------------------------------------------------------------------------------
AnyProdPlan plan_any_prod(int I, int D, int R, int B, long sai, long sak, bool native, bool prod_small)
{
    AnyProdPlan p;
    p.nblk = (D + LRF_KC - 1) / LRF_KC;
    p.fold = p.nblk > 1;
    p.fold_gx = (unsigned)(((long)I * R + 255) / 256);
    p.tpw = p.tiles = 1;
    p.native = false;
    p.refused = false;
    if (!native && !prod_small && R <= 16) { // thin products (4 x 4 patches): operands straight from global memory
        if (I <= 16 && D > 64) {
            p.k = ANY_PROD_THIN_LONG;
            p.gx = (unsigned)p.nblk; p.gy = (unsigned)B; p.gz = 1; p.threads = 64;
            return p;
        }
        if (D <= 64 && I >= 256) {
            const long nt16 = (I + 15) / 16;
            while (p.tpw < 16 && nt16 * (long)B / (2 * p.tpw) >= 8192) p.tpw *= 2;
            p.k = D <= 16 ? ANY_PROD_THIN_SHORT4 : D <= 32 ? ANY_PROD_THIN_SHORT8 : ANY_PROD_THIN_SHORT16;
            p.gx = (unsigned)((nt16 + p.tpw - 1) / p.tpw); p.gy = (unsigned)B; p.gz = 1; p.threads = 64;
            p.fold = false; // (D <= 64 < LRF_KC: one block, the kernel writes the result)
            return p;
        }
    }
    const bool fits32 = (double)I * (double)sai + 32.0 * (double)sak + (double)LRF_KC * (double)sak < 2147483648.0 && (double)LRF_KC * R < 2147483648.0;
    if (!native && D > 32 && I > 64 && R > 16 && fits32 && !prod_small) { // the 128 x 64 tiled kernel
        p.k = ANY_PROD_BIG;
        p.gx = (unsigned)((I + 127) / 128); p.gy = (unsigned)(((R + 63) / 64) * p.nblk); p.gz = (unsigned)B; p.threads = 256;
        p.refused = p.gy > 65535u;
        return p;
    }
    p.k = ANY_PROD_TILED;
    p.native = native;
    p.gy = (unsigned)(((R + 31) / 32) * p.nblk);
    p.refused = p.gy > 65535u;
    // 64-row tiles per workgroup: more for tall matrices with a short contraction, as long as ~4096 workgroups remain
    const long ntile = (I + 63) / 64;
    while (p.tiles < 8 && D <= 64 && ntile * p.gy * (long)B / (2 * p.tiles) >= 4096) p.tiles *= 2;
    p.gx = (unsigned)((ntile + p.tiles - 1) / p.tiles); p.gz = (unsigned)B; p.threads = 256;
    return p;
}

AnyGsPlan plan_any_gs(int rows, int R, int B, bool int_rows, bool gs_f32)
{
    AnyGsPlan g;
    g.native_gs = ((long)(R - 1) * rows < LRF_ANY_NATIVE_BELOW) ? 1 : 0;
    g.gx = (unsigned)((rows + 63) / 64); g.gy = (unsigned)B;
    if (int_rows && !gs_f32) { // the factor holds integers of the int8 range: byte rows in LDS
        g.k = ANY_GS_I8;
        g.lds = (((size_t)64 * 4 * (((R + 3) >> 2) | 1) + 15) & ~(size_t)15) + (size_t)R * sizeof(float);
        return g;
    }
    const size_t rows_lds = ((size_t)64 * (R | 1) * sizeof(float) + 15) & ~(size_t)15;
    const bool diag = rows_lds + (size_t)R * sizeof(float) <= LRF_ANY_GS_MAX_LDS;
    g.k = diag ? ANY_GS_F32_LDS : ANY_GS_F32_NOLDS;
    g.lds = diag ? rows_lds + (size_t)R * sizeof(float) : rows_lds;
    return g;
}

AnyUpdatePlan plan_any_update(int B, int M, int N, int R, bool trans, bool int_rows, bool prod_small, bool gs_f32)
{
    const int rows = trans ? N : M, depth = trans ? M : N;
    AnyUpdatePlan u;
    u.a = plan_any_prod(rows, depth, R, B, trans ? 1 : N, trans ? N : 1, (long)depth * rows * R < LRF_ANY_NATIVE_BELOW, prod_small);
    u.b = plan_any_prod(R, depth, R, B, 1, R, (long)depth * R * R < LRF_ANY_NATIVE_BELOW, prod_small);
    u.gs = plan_any_gs(rows, R, B, int_rows, gs_f32);
    return u;
}

long plan_any_init_chunk(int n, int Rc, long B)
{
    const size_t per = sizeof(double) * ((size_t)n * n + (size_t)3 * n * Rc);
    long chunk = (long)(LRF_ANY_INIT_WORK_BYTES / per);
    if (chunk < 1) chunk = 1;
    return chunk > B ? B : chunk;
}

// ---- which decode body serves an image, and the image list of a decode or SSE entry ------------------------------------------
DecodePlan decode_plan(const ImageGeom& g, int64_t H, int64_t W, const int R[3], bool aligned8, bool no_tiled)
{
    // the tiled kernels (k_decode16: sides multiples of 16; k_decode_strip: any height, four-aligned chroma columns) are
    // instantiated for the rank bounds (chroma, luma) = (4,8) (8,8) (8,16) (16,16) (16,32): the reference's quality sweep up to 40
    const int rcm = R[1] > R[2] ? R[1] : R[2];
    const int RCb = rcm <= 4 ? 4 : (rcm <= 8 ? 8 : 16), RLb = R[0] <= 8 ? 8 : (R[0] <= 16 ? 16 : 32);
    const bool tiled_ranks = R[0] <= 32 && rcm <= 16 && !no_tiled;
    const bool sides16 = H % 16 == 0 && W % 16 == 0 && aligned8;
    const bool strip_ok = W % 2 == 0 && g.p[0].left_crop % 2 == 0 && (g.p[1].left_crop - g.p[0].left_crop / 2) % 4 == 0 && g.p[1].w == W / 2;
    if (tiled_ranks && (sides16 || strip_ok)) {
        int cls;
        if (RLb == 8 && RCb == 4) cls = 0;
        else if (RLb == 8 && RCb == 8) cls = 1;
        else if (RLb == 16 && RCb <= 8) cls = 2;
        else if (RLb <= 16) cls = 3;
        else cls = 4;
        return DecodePlan{sides16 ? DEC_TILE16 : DEC_STRIP, cls};
    }
    return DecodePlan{(R[0] <= 8 && R[1] <= 8 && R[2] <= 8) ? DEC_R8 : DEC_ANY, 0};
}

DescribeRefusal describe_images(int64_t n, const lrf_ragged_image* images, int64_t u_len, int64_t v_len, const DescribeOptions& o,
                                std::vector<RaggedDesc>& descs, std::vector<RaggedWork>* work)
{
    descs.resize((size_t)n);
    memset((void*)descs.data(), 0, descs.size() * sizeof(RaggedDesc)); // (the bytes are the table's key: padding included)
    if (work) work->resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const lrf_ragged_image& im = images[i];
        RaggedDesc& d = descs[(size_t)i];
        if (im.H < 1 || im.W < 1 || im.H > INT32_MAX || im.W > INT32_MAX) return DescribeRefusal{DESC_SIZE, i, im.H, im.W};
        int64_t bh, bw;
        if (geom_of(im.H, im.W, &d.g, &bh, &bw)) return DescribeRefusal{DESC_GEOM, i, im.H, im.W};
        for (int ch = 0; ch < 3; ch++)
            if (im.R[ch] < 1 || im.R[ch] > 64) return DescribeRefusal{DESC_RANK, i, im.R[ch], 0};
        if (im.u_off < 0 || im.v_off < 0 || (o.check_rgb && im.rgb_off < 0)) return DescribeRefusal{DESC_NEGATIVE, i, 0, 0};
        long u_img = 0, v_img = 0;
        for (int ch = 0; ch < 3; ch++) {
            u_img += (long)d.g.p[ch].M * im.R[ch];
            v_img += 64L * im.R[ch];
        }
        if (u_img > u_len || im.u_off > u_len - u_img) return DescribeRefusal{DESC_U, i, u_len, 0};
        if (v_img > v_len || im.v_off > v_len - v_img) return DescribeRefusal{DESC_V, i, v_len, 0};
        if (o.check_rgb && (o.rgb_len < 3 || im.H * im.W > o.rgb_len / 3 || im.rgb_off > o.rgb_len - 3 * im.H * im.W))
            return DescribeRefusal{DESC_RGB, i, o.rgb_len, 0};
        const bool aligned8 = o.aligned8 || ((o.rgb_base + (uintptr_t)im.rgb_off) & 7) == 0;
        const DecodePlan plan = decode_plan(d.g, im.H, im.W, im.R, aligned8, o.no_tiled);
        d.u_off = im.u_off; d.v_off = im.v_off;
        if (o.check_rgb) d.rgb_off = im.rgb_off;
        d.H = (int)im.H; d.W = (int)im.W;
        d.R0 = im.R[0]; d.R1 = im.R[1]; d.R2 = im.R[2];
        d.kind = plan.kind; d.cls = plan.cls;
        d.per_strip = (d.g.p[0].nw + 31) / 32;
        if (!work) continue;
        RaggedWork& w = (*work)[(size_t)i];
        w.kind = plan.kind; w.cls = plan.cls;
        if (plan.kind == DEC_TILE16) w.units = (long)(im.H / 16) * d.per_strip;
        else if (plan.kind == DEC_STRIP) w.units = (long)((d.g.p[0].nh + 1) / 2) * d.per_strip;
        else w.units = (long)im.H * ((im.W + 3) / 4);
    }
    return DescribeRefusal{};
}

// ---- the launches of a ragged decode -----------------------------------------------------------------------------------------
// All DEC_TILE16 images share one launch (the 16-aligned body under a class switch keeps the registers of its largest class);
// the strip body does not (204 registers under a switch), so DEC_STRIP images take one launch per class present; DEC_R8 and
// DEC_ANY one each.  A workgroup finds its work through blocks[blockIdx.x].
RaggedPlan plan_decode_ragged(const std::vector<RaggedWork>& images)
{
    RaggedPlan p;
    const int nslots = 3 + LRF_DEC_CLASSES;
    auto slot_of = [](const RaggedWork& w) { return w.kind == DEC_TILE16 ? 0 : (w.kind == DEC_STRIP ? 1 + w.cls : (w.kind == DEC_R8 ? 1 + LRF_DEC_CLASSES : 2 + LRF_DEC_CLASSES)); };
    long quads8 = 0; // DEC_R8: groups of 256 pixel quads of the whole launch
    for (const RaggedWork& w : images)
        if (w.kind == DEC_R8) quads8 += (w.units + 255) / 256;
    const long reps = decode8_reps_of(quads8);
    auto blocks_of = [&](const RaggedWork& w) {
        if (w.kind == DEC_R8) return (w.units + 256 * reps - 1) / (256 * reps);
        if (w.kind == DEC_ANY) return (w.units + 255) / 256;
        return w.units;
    };
    std::vector<long> count((size_t)nslots, 0);
    for (const RaggedWork& w : images) count[(size_t)slot_of(w)] += blocks_of(w);
    long total = 0;
    for (int s = 0; s < nslots; s++) {
        if (count[(size_t)s] >= (1L << 31)) {
            p.too_many = count[(size_t)s];
            return p;
        }
        total += count[(size_t)s];
    }
    p.blocks.reserve((size_t)total);
    for (int s = 0; s < nslots; s++) {
        if (!count[(size_t)s]) continue;
        RaggedLaunch l;
        l.kind = s == 0 ? DEC_TILE16 : (s <= LRF_DEC_CLASSES ? DEC_STRIP : (s == 1 + LRF_DEC_CLASSES ? DEC_R8 : DEC_ANY));
        l.cls = l.kind == DEC_TILE16 ? -1 : (l.kind == DEC_STRIP ? s - 1 : 0);
        l.block0 = (long)p.blocks.size();
        l.nblocks = count[(size_t)s];
        l.reps = l.kind == DEC_R8 ? (int)reps : 1;
        for (size_t i = 0; i < images.size(); i++) {
            if (slot_of(images[i]) != s) continue;
            const long nb = blocks_of(images[i]);
            for (long t = 0; t < nb; t++) p.blocks.push_back(RaggedBlock{(int)i, (int)t});
        }
        p.launches.push_back(l);
    }
    return p;
}

// ---- the tables of the ragged metrics ------------------------------------------------------------------------------------------
static int metrics_vec_of(uintptr_t bits) { return (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1); }

MetricsRaggedPlan plan_metrics_ragged(int64_t n, const lrf_image_pair* pairs, const MetricsCall& k)
{
    MetricsRaggedPlan p;
    auto refuse = [&](int check, int64_t pair, int64_t a, int64_t b) {
        p = MetricsRaggedPlan();
        p.refusal.check = check;
        p.refusal.pair = pair;
        p.refusal.a = a;
        p.refusal.b = b;
        return p;
    };
    if (n < 1 || n > 65535) return refuse(MTR_N, 0, n, 0);
    if (k.C < 1 || k.C > 65535) return refuse(MTR_C, 0, k.C, 0);
    const int64_t side_min = k.want_ssim ? 7 : 1;
    for (int64_t i = 0; i < n; i++) {
        const lrf_image_pair& q = pairs[i];
        if (q.H < side_min || q.W < side_min || q.H > (1 << 20) || q.W > (1 << 20) || q.H * q.W >= ((int64_t)1 << 40) / k.C)
            return refuse(MTR_SIZE, i, q.H, q.W);
        if (q.a_off < 0 || q.b_off < 0) return refuse(MTR_NEGATIVE, i, 0, 0);
        const int64_t bytes = (int64_t)k.C * q.H * q.W;
        if (bytes > k.a_len || q.a_off > k.a_len - bytes) return refuse(MTR_A, i, k.a_len, 0);
        if (bytes > k.b_len || q.b_off > k.b_len - bytes) return refuse(MTR_B, i, k.b_len, 0);
    }
    // the counts first: a refused list builds nothing
    long tile_wgs = 0, span_wgs = 0;
    for (int64_t i = 0; i < n; i++) {
        const lrf_image_pair& q = pairs[i];
        if (k.want_ssim) tile_wgs += (long)k.C * metrics_tiles_x(q.W) * metrics_tiles_y(q.H);
        span_wgs += ((long)k.C * q.H * q.W + LRF_MTR_PRE_BYTES - 1) / LRF_MTR_PRE_BYTES; // (an upper bound with the SSIM: shared sources count once)
        if (tile_wgs >= (1L << 31)) return refuse(MTR_TOO_MANY, i, tile_wgs, 0);
        if (span_wgs >= (1L << 31)) return refuse(MTR_TOO_MANY, i, span_wgs, 0);
    }
    p.pairs.resize((size_t)n);
    memset(p.pairs.data(), 0, (size_t)n * sizeof(MetricsPairDesc));
    std::vector<int> src((size_t)n, 0);
    if (k.want_ssim) {
        std::vector<int64_t> order((size_t)n);
        for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
        auto key = [&](int64_t i) { return std::array<int64_t, 3>{pairs[i].a_off, pairs[i].H, pairs[i].W}; };
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key(x) < key(y); });
        // the first pair (in call order) of every group of equal keys stands for it; spans in order of first appearance
        std::vector<int64_t> rep((size_t)n);
        for (size_t j = 0; j < order.size(); j++) rep[(size_t)order[j]] = j && key(order[j]) == key(order[j - 1]) ? rep[(size_t)order[j - 1]] : order[j];
        std::vector<int> span_of((size_t)n, -1);
        for (int64_t i = 0; i < n; i++) {
            if (rep[(size_t)i] == i) {
                span_of[(size_t)i] = (int)p.spans.size();
                MetricsSpanDesc s;
                memset(&s, 0, sizeof s);
                s.a_off = pairs[i].a_off;
                s.n = (long)k.C * pairs[i].H * pairs[i].W;
                p.spans.push_back(s);
            }
            src[(size_t)i] = span_of[(size_t)rep[(size_t)i]]; // (a group's first pair comes first in call order: already set)
        }
    } else {
        for (int64_t i = 0; i < n; i++) {
            MetricsSpanDesc s;
            memset(&s, 0, sizeof s);
            s.a_off = pairs[i].a_off;
            s.b_off = pairs[i].b_off;
            s.n = (long)k.C * pairs[i].H * pairs[i].W;
            p.spans.push_back(s);
            src[(size_t)i] = (int)i;
        }
    }
    for (MetricsSpanDesc& s : p.spans) {
        s.wg0 = (int)p.span_wgs;
        s.vec = metrics_vec_of((k.a_base + (uintptr_t)s.a_off) | (k.want_ssim ? 0 : k.b_base + (uintptr_t)s.b_off) | (uintptr_t)s.n);
        p.span_wgs += (s.n + LRF_MTR_PRE_BYTES - 1) / LRF_MTR_PRE_BYTES;
    }
    for (int64_t i = 0; i < n; i++) {
        const lrf_image_pair& q = pairs[i];
        MetricsPairDesc& d = p.pairs[(size_t)i];
        d.a_off = q.a_off;
        d.b_off = q.b_off;
        d.H = (int)q.H;
        d.W = (int)q.W;
        d.src = src[(size_t)i];
        d.vec = metrics_vec_of((k.a_base + (uintptr_t)q.a_off) | (k.b_base + (uintptr_t)q.b_off) | (uintptr_t)q.W);
        d.wg0 = (int)p.tile_wgs;
        if (k.want_ssim) {
            d.ntx = (int)metrics_tiles_x(q.W);
            d.nt = (int)(metrics_tiles_x(q.W) * metrics_tiles_y(q.H));
            p.tile_wgs += (long)k.C * d.nt;
        }
    }
    return p;
}

MetricsChunks plan_metrics_chunks(int64_t n, const lrf_ragged_image* items, int64_t cap)
{
    MetricsChunks c;
    c.off.resize((size_t)n);
    MetricsChunk cur = {0, 0, 0};
    for (int64_t i = 0; i < n; i++) {
        const int64_t bytes = (3 * items[i].H * items[i].W + 15) / 16 * 16;
        if (cur.nitems && cur.bytes + bytes > cap) {
            c.chunks.push_back(cur);
            cur = MetricsChunk{i, 0, 0};
        }
        c.off[(size_t)i] = cur.bytes;
        cur.bytes += bytes;
        cur.nitems++;
    }
    if (cur.nitems) c.chunks.push_back(cur);
    for (const MetricsChunk& k : c.chunks) c.max_bytes = std::max(c.max_bytes, k.bytes);
    return c;
}

// ---- the launches of a decode of windows -----------------------------------------------------------------------------------------
// One launch per rank-bound class of the tiled body present (the strip body under a class switch: 204 registers), one each for
// DEC_R8 and DEC_ANY.  The table is a stable sort of the call's list by launch.
CropPlan plan_decode_crops(const std::vector<RaggedWork>& images, const std::vector<CropEntry>& crops, int h, int w)
{
    CropPlan p;
    const int nslots = LRF_DEC_CLASSES + 2;
    auto slot_of = [&](const CropEntry& e) {
        const RaggedWork& im = images[(size_t)e.image];
        return im.kind == DEC_TILE16 || im.kind == DEC_STRIP ? im.cls : (im.kind == DEC_R8 ? LRF_DEC_CLASSES : LRF_DEC_CLASSES + 1);
    };
    std::vector<long> count((size_t)nslots, 0);
    for (const CropEntry& e : crops) count[(size_t)slot_of(e)]++;
    const long wgs_tiled = crop_tiled_wgs(h, w), wgs_quad = crop_quad_wgs(h, w);
    for (int s = 0; s < nslots; s++) {
        const long wgs = s < LRF_DEC_CLASSES ? wgs_tiled : wgs_quad;
        if (count[(size_t)s] && (wgs >= (1L << 31) || count[(size_t)s] * wgs >= (1L << 31))) {
            p.too_many = wgs >= (1L << 31) ? wgs : count[(size_t)s] * wgs;
            return p;
        }
    }
    p.table.reserve(crops.size());
    for (int s = 0; s < nslots; s++) {
        if (!count[(size_t)s]) continue;
        CropLaunch l;
        l.kind = s < LRF_DEC_CLASSES ? DEC_STRIP : (s == LRF_DEC_CLASSES ? DEC_R8 : DEC_ANY);
        l.cls = s < LRF_DEC_CLASSES ? s : 0;
        l.crop0 = (long)p.table.size();
        l.ncrops = count[(size_t)s];
        l.wgs = s < LRF_DEC_CLASSES ? wgs_tiled : wgs_quad;
        for (size_t j = 0; j < crops.size(); j++)
            if (slot_of(crops[j]) == s) p.table.push_back(CropEntry{crops[j].image, crops[j].y0, crops[j].x0, (int)j});
        p.launches.push_back(l);
    }
    return p;
}

// ---- the launches of a decode at 1/2, 1/4, 1/8 scale ----------------------------------------------------------------------------
// The table is a stable sort of the call's items by (path, f, class): the tiled body is instantiated per scale and rank-bound
// class, the general body reads the scale from the item and takes one launch per scale (the items of a scale are of a similar
// size, and a launch's grid is its largest item's).  The tiled items of one (image, f) share one set of pooled tables.
ScaledPlan plan_decode_scaled(const std::vector<ScaledImage>& images, const std::vector<ScaledItem>& items)
{
    ScaledPlan p;
    const int nslots = LRF_SCALED_MAX_LAUNCHES;
    auto fi = [](int f) { return f == 2 ? 0 : (f == 4 ? 1 : 2); };
    auto slot_of = [&](const ScaledItem& e) {
        const ScaledImage& im = images[(size_t)e.image];
        return im.tiled ? fi(e.f) * LRF_DEC_CLASSES + im.cls : 3 * LRF_DEC_CLASSES + fi(e.f);
    };
    auto wgs_of = [&](const ScaledItem& e) { return images[(size_t)e.image].tiled ? scaled_tiled_wgs(e.f, e.y0, e.x0, e.h, e.w) : scaled_any_wgs(e.h, e.w); };
    std::vector<long> count((size_t)nslots, 0), wgs((size_t)nslots, 0);
    for (const ScaledItem& e : items) {
        const int s = slot_of(e);
        const long g = wgs_of(e);
        count[(size_t)s]++;
        if (g > wgs[(size_t)s]) wgs[(size_t)s] = g;
    }
    for (int s = 0; s < nslots; s++)
        if (count[(size_t)s] && (wgs[(size_t)s] >= (1L << 31) || count[(size_t)s] * wgs[(size_t)s] >= (1L << 31))) {
            p.too_many = wgs[(size_t)s] >= (1L << 31) ? wgs[(size_t)s] : count[(size_t)s] * wgs[(size_t)s];
            return p;
        }
    std::vector<long> pool_of(images.size() * 3, -1); // (image, f) -> its tables
    p.table.reserve(items.size());
    for (int s = 0; s < nslots; s++) {
        if (!count[(size_t)s]) continue;
        ScaledLaunch l;
        l.tiled = s < 3 * LRF_DEC_CLASSES;
        l.f = 2 << (l.tiled ? s / LRF_DEC_CLASSES : s - 3 * LRF_DEC_CLASSES);
        l.cls = l.tiled ? s % LRF_DEC_CLASSES : 0;
        l.item0 = (long)p.table.size();
        l.nitems = count[(size_t)s];
        l.wgs = wgs[(size_t)s];
        for (size_t j = 0; j < items.size(); j++) {
            if (slot_of(items[j]) != s) continue;
            ScaledItem e = items[j];
            e.place = (int)j;
            e.pad = 0;
            e.pool_off = 0;
            if (l.tiled) {
                long& at = pool_of[(size_t)e.image * 3 + (size_t)fi(e.f)];
                if (at < 0) {
                    at = p.pool_elems;
                    p.jobs.push_back(ScaledPoolJob{e.image, e.f, at});
                    p.pool_elems += scaled_pool_elems(images[(size_t)e.image].R, e.f);
                }
                e.pool_off = at;
            }
            p.table.push_back(e);
        }
        p.launches.push_back(l);
    }
    return p;
}

// The table is a stable sort of the call's boxes by (path, level, rank class): one launch per group that occurs, so at most
// LRF_RESIZED_MAX_LAUNCHES.  Every box of a call has the same output size, so the workgroups per box depend on the path alone.
ResizedPlan plan_decode_resized(const std::vector<int>& r8, const std::vector<ResizedItem>& crops, int oh, int ow)
{
    ResizedPlan p;
    const int nslots = LRF_RESIZED_MAX_LAUNCHES;
    auto fi = [](int f) { return f == 1 ? 0 : (f == 2 ? 1 : (f == 4 ? 2 : 3)); };
    auto slot_of = [&](const ResizedItem& e, int f) { return (resized_staged(e.hb, e.wb, oh, ow, f) ? 0 : 8) + fi(f) * 2 + (r8[(size_t)e.image] ? 0 : 1); };
    std::vector<int> level(crops.size()), slot(crops.size());
    std::vector<long> count((size_t)nslots, 0);
    for (size_t j = 0; j < crops.size(); j++) {
        level[j] = resized_level(crops[j].hb, crops[j].wb, oh, ow);
        slot[j] = slot_of(crops[j], level[j]);
        count[(size_t)slot[j]]++;
    }
    const long wgs[2] = {resized_staged_wgs(oh, ow), resized_direct_wgs(oh, ow)};
    for (int s = 0; s < nslots; s++) {
        const long g = wgs[s >> 3];
        if (count[(size_t)s] && (g >= (1L << 31) || count[(size_t)s] * g >= (1L << 31))) {
            p.too_many = g >= (1L << 31) ? g : count[(size_t)s] * g;
            return p;
        }
    }
    p.table.reserve(crops.size());
    for (int s = 0; s < nslots; s++) {
        if (!count[(size_t)s]) continue;
        ResizedLaunch l;
        l.direct = s >> 3;
        l.f = 1 << ((s >> 1) & 3);
        l.r8 = !(s & 1);
        l.item0 = (long)p.table.size();
        l.nitems = count[(size_t)s];
        l.wgs = wgs[l.direct];
        for (size_t j = 0; j < crops.size(); j++) {
            if (slot[j] != s) continue;
            ResizedItem e = crops[j];
            e.f = level[j];
            e.place = (int)j;
            e.flip = e.flip != 0;
            p.table.push_back(e);
        }
        p.launches.push_back(l);
    }
    return p;
}

// ---- the gray loader ----------------------------------------------------------------------------------------------------------
GrayRefusal describe_gray_images(int64_t n, const lrf_gray_image* images, int64_t u_len, int64_t v_len, int scale, int64_t out_len,
                                 std::vector<GrayDesc>& descs)
{
    static_assert(sizeof(GrayDesc) == 2 * sizeof(long) + 6 * sizeof(int), "GrayDesc has padding bytes: they would be part of the table's key");
    descs.assign((size_t)n, GrayDesc{});
    for (int64_t i = 0; i < n; i++) {
        const lrf_gray_image& im = images[i];
        GrayDesc& d = descs[(size_t)i];
        if (im.H < 1 || im.W < 1 || im.H > (1 << 20) || im.W > (1 << 20) || im.H * im.W >= (1LL << 31)) return GrayRefusal{GDESC_SIZE, i, im.H, im.W};
        // reflect padding to multiples of 8, top = pad / 2 (lrf_chan_dims; lrf/compression/utils.py:108-132)
        const int64_t ph = (8 - im.H % 8) % 8, pw = (8 - im.W % 8) % 8;
        if (ph / 2 >= im.H || ph - ph / 2 >= im.H || pw / 2 >= im.W || pw - pw / 2 >= im.W) return GrayRefusal{GDESC_GEOM, i, im.H, im.W};
        if (im.R < 1 || im.R > 64) return GrayRefusal{GDESC_RANK, i, im.R, 0};
        if (im.u_off < 0 || im.v_off < 0 || (scale && im.out_off < 0)) return GrayRefusal{GDESC_NEGATIVE, i, 0, 0};
        const int64_t M = ((im.H + ph) / 8) * ((im.W + pw) / 8); // < 2^25 + ...: M R and 64 R cannot wrap
        const int64_t u_img = M * im.R, v_img = 64LL * im.R;
        if (u_img > u_len || im.u_off > u_len - u_img) return GrayRefusal{GDESC_U, i, u_len, 0};
        if (v_img > v_len || im.v_off > v_len - v_img) return GrayRefusal{GDESC_V, i, v_len, 0};
        if (scale) {
            const int64_t px = ((im.H + scale - 1) / scale) * ((im.W + scale - 1) / scale);
            if (px > out_len || im.out_off > out_len - px) return GrayRefusal{GDESC_OUT, i, out_len, 0};
        }
        d.u_off = im.u_off; d.v_off = im.v_off;
        d.H = (int)im.H; d.W = (int)im.W; d.R = im.R;
        d.top = (int)(ph / 2); d.left = (int)(pw / 2);
        d.nw = (int)((im.W + pw) / 8);
    }
    return GrayRefusal{};
}

// The table is a stable sort of the call's items by slot; one launch per slot that occurs.  wgs_of: the workgroups item j needs
template <class SlotOf, class WgsOf, class Finish>
static GrayPlan plan_gray(const std::vector<GrayItem>& items, int nslots, SlotOf slot_of, WgsOf wgs_of, Finish finish)
{
    GrayPlan p;
    std::vector<int> slot(items.size());
    std::vector<long> count((size_t)nslots, 0), wgs((size_t)nslots, 0);
    for (size_t j = 0; j < items.size(); j++) {
        slot[j] = slot_of(items[j]);
        count[(size_t)slot[j]]++;
        const long g = wgs_of(items[j], slot[j]);
        if (g > wgs[(size_t)slot[j]]) wgs[(size_t)slot[j]] = g;
    }
    for (int s = 0; s < nslots; s++)
        if (count[(size_t)s] && (wgs[(size_t)s] >= (1L << 31) || count[(size_t)s] * wgs[(size_t)s] >= (1L << 31))) {
            p.too_many = wgs[(size_t)s] >= (1L << 31) ? wgs[(size_t)s] : count[(size_t)s] * wgs[(size_t)s];
            return p;
        }
    p.table.reserve(items.size());
    for (int s = 0; s < nslots; s++) {
        if (!count[(size_t)s]) continue;
        GrayLaunch l;
        l.f = 1 << (s & 3);
        l.direct = s >> 2;
        l.item0 = (long)p.table.size();
        l.nitems = count[(size_t)s];
        l.wgs = wgs[(size_t)s];
        for (size_t j = 0; j < items.size(); j++) {
            if (slot[j] != s) continue;
            GrayItem e = items[j];
            e.f = l.f;
            e.place = (int)j;
            e.flip = e.flip != 0;
            finish(e);
            p.table.push_back(e);
        }
        p.launches.push_back(l);
    }
    return p;
}
static int gray_level_slot(int f) { return f == 1 ? 0 : (f == 2 ? 1 : (f == 4 ? 2 : 3)); }

GrayPlan plan_gray_windows(const std::vector<GrayDesc>& descs, const std::vector<GrayItem>& items)
{
    return plan_gray(
        items, 4, [](const GrayItem& e) { return gray_level_slot(e.f); },
        [&](const GrayItem& e, int) {
            const GrayDesc& d = descs[(size_t)e.image];
            return e.f == 1 ? gray_tile_wgs(d.top, d.left, e.y0, e.x0, e.h, e.w) : crop_quad_wgs(e.h, e.w);
        },
        [](GrayItem&) {});
}

GrayPlan plan_gray_resized(const std::vector<GrayItem>& boxes, int oh, int ow)
{
    return plan_gray(
        boxes, 8,
        [&](const GrayItem& e) {
            const int f = resized_level(e.h, e.w, oh, ow);
            return (resized_staged(e.h, e.w, oh, ow, f) ? 0 : 4) + gray_level_slot(f);
        },
        [&](const GrayItem&, int s) { return s >> 2 ? resized_direct_wgs(oh, ow) : resized_staged_wgs(oh, ow); },
        [&](GrayItem& e) {
            e.out_off = (long)e.place * oh * ow;
            e.pitch = ow;
        });
}

// ---- the window list of the entries that decode crops ----------------------------------------------------------------------------
WindowRefusal check_window_call(const WindowCall& k)
{
    WindowRefusal r;
    if (k.n_images < 1 || k.n_images > 65535) r.check = WIN_N_IMAGES;
    else if (k.n_crops < 1 || k.n_crops > LRF_WIN_MAX_CROPS) r.check = WIN_N_CROPS;
    else if (k.h < 1 || k.w < 1 || k.h > (k.resized ? LRF_WIN_MAX_RESIZED_SIDE : INT32_MAX) || k.w > (k.resized ? LRF_WIN_MAX_RESIZED_SIDE : INT32_MAX))
        r.check = WIN_SIZE;
    return r;
}

namespace {
// what the three ABI shapes differ in: whether a crop carries a scale (else it is at scale 1) and sides of its own (else the call's)
template <class Crop> struct CropShape { static constexpr bool scaled = false, boxed = false; };
template <> struct CropShape<lrf_scaled_crop> { static constexpr bool scaled = true, boxed = false; };
template <> struct CropShape<lrf_resized_crop> { static constexpr bool scaled = false, boxed = true; };
struct Window { int image, scale, y0, x0; int64_t h, w; int flip; }; // an accepted crop of any shape
// the validated window j as each plan takes it (sides and j fit an int: checked)
template <class Item>
Item item_of(const Window& v, int64_t j, const WindowCall& k);
template <> inline CropEntry item_of(const Window& v, int64_t j, const WindowCall&) { return CropEntry{v.image, v.y0, v.x0, (int)j}; }
template <> inline ScaledItem item_of(const Window& v, int64_t j, const WindowCall& k)
{
    return ScaledItem{v.image, v.scale, v.y0, v.x0, (int)v.h, (int)v.w, (int)j, 0, (long)(k.channels * v.h * v.w * j), 0};
}
template <> inline ResizedItem item_of(const Window& v, int64_t j, const WindowCall&)
{
    return ResizedItem{v.image, 1, v.y0, v.x0, (int)v.h, (int)v.w, v.flip, (int)j};
}
template <> inline GrayItem item_of(const Window& v, int64_t j, const WindowCall& k) // (boxes: plan_gray_resized sets out_off and pitch)
{
    return GrayItem{v.image, v.scale, v.y0, v.x0, (int)v.h, (int)v.w, v.flip, (int)j, k.resized ? 0 : (long)(j * v.h * v.w), k.resized ? 0 : (long)v.w};
}
}

template <class Desc, class Crop, class Item>
WindowRefusal check_windows(const WindowCall& call, const std::vector<Desc>& descs, const Crop* crops, std::vector<Item>& items)
{
    using Shape = CropShape<Crop>;
    const WindowCall k = call; // (locals, like `size` and `out` below: the item stores cannot alias them, so the loop keeps them in registers)
    // (h <= len / channels / w first: then channels h w cannot wrap)
    if (k.out_len < k.channels || k.h > k.out_len / k.channels / k.w || k.n_crops > k.out_len / (k.channels * k.h * k.w))
        return WindowRefusal{WIN_CAPACITY};
    items.resize((size_t)k.n_crops);
    Item* const out = items.data();
    // (H, W) per image, compact and as wide as the comparisons: the loop reads nothing else of a descriptor
    std::vector<int64_t> sizes(2 * (size_t)k.n_images);
    for (int64_t i = 0; i < k.n_images; i++) { sizes[2 * (size_t)i] = descs[(size_t)i].H; sizes[2 * (size_t)i + 1] = descs[(size_t)i].W; }
    const int64_t* const size = sizes.data();
    // one crop: what the shape does not carry is the call's, constants of the loop (the call's sides are >= 1: check_window_call).
    // r: null in the loop; the refusal's operands, filled on the way out
    auto check_crop = [&](const Crop& c, int64_t j, WindowRefusal* r) -> int {
        int scale = 1, flip = 0;
        int64_t h = k.h, w = k.w;
        if constexpr (Shape::scaled) scale = c.scale;
        if constexpr (Shape::boxed) { h = c.h; w = c.w; flip = c.flip != 0; }
        int check = WIN_OK;
        int64_t H = 0, W = 0; // the image at the window's scale
        if (c.image < 0 || c.image >= k.n_images) check = WIN_IMAGE;
        else if (Shape::scaled && (scale < 0 || scale > 8 || !((k.scales >> scale) & 1u))) check = WIN_SCALE;
        else if (Shape::boxed && (h < 1 || w < 1)) check = WIN_SIDES;
        else {
            H = size[2 * c.image]; W = size[2 * c.image + 1];
            if constexpr (Shape::scaled) { H = scaled_dim(H, scale); W = scaled_dim(W, scale); }
            const int64_t dy = H - h, dx = W - w; // (all four below 2^31: the room below and right of the window's origin)
            if (c.y0 < 0 || c.x0 < 0 || dy < 0 || dx < 0 || c.y0 > dy || c.x0 > dx) check = WIN_BOX;
        }
        if (r) *r = WindowRefusal{check, j, c.image, scale, c.y0, c.x0, h, w, H, W};
        else if (check == WIN_OK) out[j] = item_of<Item>(Window{c.image, scale, c.y0, c.x0, h, w, flip}, j, k);
        return check;
    };
    for (int64_t j = 0; j < k.n_crops; j++)
        if (check_crop(crops[j], j, nullptr) != WIN_OK) { // (the loop carries no operand of a refusal: the first offender is looked at again)
            WindowRefusal r;
            check_crop(crops[j], j, &r);
            return r;
        }
    return WindowRefusal{};
}
template WindowRefusal check_windows(const WindowCall&, const std::vector<RaggedDesc>&, const lrf_crop*, std::vector<CropEntry>&);
template WindowRefusal check_windows(const WindowCall&, const std::vector<RaggedDesc>&, const lrf_scaled_crop*, std::vector<ScaledItem>&);
template WindowRefusal check_windows(const WindowCall&, const std::vector<RaggedDesc>&, const lrf_resized_crop*, std::vector<ResizedItem>&);
template WindowRefusal check_windows(const WindowCall&, const std::vector<GrayDesc>&, const lrf_scaled_crop*, std::vector<GrayItem>&);
template WindowRefusal check_windows(const WindowCall&, const std::vector<GrayDesc>&, const lrf_resized_crop*, std::vector<GrayItem>&);

// ---- geometry -----------------------------------------------------------------------------------------------------------------
void plane_dims(int64_t H, int64_t W, int c, int64_t* h, int64_t* w, int64_t* hp, int64_t* wp, int64_t* M)
{
    // F.interpolate(scale_factor=0.5): output size = floor(input * 0.5) (lrf/compression/qmf.py:230)
    int64_t ph = c ? (int64_t)floor((double)H * 0.5) : H, pw = c ? (int64_t)floor((double)W * 0.5) : W;
    *h = ph;
    *w = pw;
    *hp = ph + (8 - ph % 8) % 8;
    *wp = pw + (8 - pw % 8) % 8;
    *M = (*hp / 8) * (*wp / 8);
}

int geom_of(int64_t H, int64_t W, ImageGeom* g, int64_t* bad_h, int64_t* bad_w)
{
    long xoff = 0;
    for (int c = 0; c < 3; c++) {
        int64_t h, w, hp, wp, M;
        plane_dims(H, W, c, &h, &w, &hp, &wp, &M);
        *bad_h = h;
        *bad_w = w;
        if (h < 1 || w < 1) return c + 1;
        // reflect padding needs pad < size (torch raises otherwise)
        if ((hp - h) / 2 >= h || (hp - h) - (hp - h) / 2 >= h || (wp - w) / 2 >= w || (wp - w) - (wp - w) / 2 >= w) return 10 + c + 1;
        PlaneGeom& p = g->p[c];
        p.h = (int)h; p.w = (int)w; p.hp = (int)hp; p.wp = (int)wp;
        p.top = (int)((hp - h) / 2); p.left = (int)((wp - w) / 2);
        p.top_crop = p.top; p.left_crop = p.left;
        p.nw = (int)(wp / 8);
        p.nh = (int)(hp / 8);
        p.pr0 = c ? g->p[c - 1].pr0 + g->p[c - 1].nh : 0;
        p.M = (int)M;
        p.xoff = xoff;
        p.o4 = xoff / 4;
        xoff += M * 64;
    }
    g->img_floats = xoff;
    g->tot4 = xoff / 4;
    return 0;
}

// ---- the tables of a ragged encode ----------------------------------------------------------------------------------------------
// The planes stage: all ENC_TILE16 images share one launch, the others one launch per window size present.  A workgroup finds
// its work through blocks[i].  Behind it the call is the table of its planes: everything from the Gram pass on reads PlaneDesc.
// the descriptors of the planes stage (geometry, body, units, the X workspace as a running sum) -> its workgroups in all
struct PlanesStage {
    std::vector<EncRaggedDesc> descs;
    std::vector<long> units;
    long count[LRF_ENC_BODIES] = {0, 0, 0, 0, 0}, total = 0, x_floats = 0;
};
static PlanesStage planes_stage_descs(const std::vector<EncRaggedImage>& images)
{
    PlanesStage st;
    const size_t n = images.size();
    st.descs.resize(n);
    memset((void*)st.descs.data(), 0, n * sizeof(EncRaggedDesc)); // (the bytes are the device table's key: padding included)
    st.units.resize(n);
    for (size_t i = 0; i < n; i++) {
        const EncRaggedImage& im = images[i];
        EncRaggedDesc& d = st.descs[i];
        int64_t bh, bw;
        (void)geom_of(im.H, im.W, &d.g, &bh, &bw); // (validated by the caller)
        const ImageGeom& g = d.g;
        d.rgb_off = im.rgb_off;
        d.x_off = st.x_floats;
        st.x_floats += g.img_floats;
        d.H = (int)im.H; d.W = (int)im.W;
        if (im.H % 16 == 0 && im.W % 16 == 0 && im.aligned8) {
            d.body = ENC_TILE16;
            d.per_strip = (g.p[0].nw + 31) / 32;
            st.units[i] = (im.H / 16) * d.per_strip;
        } else { // k_planes16's tiling laid over the padded planes (lrf_qmf_planes_from_rgb_u8)
            d.body = ENC_STRIP22 + 2 * (int)(im.H & 1) + (int)(im.W & 1);
            const int ncols = g.p[0].nw > 2 * g.p[1].nw ? g.p[0].nw : 2 * g.p[1].nw;
            const int nstrips = (g.p[0].nh + 1) / 2 > g.p[1].nh ? (g.p[0].nh + 1) / 2 : g.p[1].nh;
            d.per_strip = (ncols + 31) / 32;
            st.units[i] = (long)nstrips * d.per_strip;
        }
        st.count[d.body] += st.units[i];
    }
    for (int b = 0; b < LRF_ENC_BODIES; b++) st.total += st.count[b];
    return st;
}
// its launches and workgroup table: by body, inside a launch the images in call order, an image's units ascending
static void planes_stage_launches(const PlanesStage& st, std::vector<EncRaggedLaunch>& launches, std::vector<RaggedBlock>& blocks)
{
    blocks.reserve((size_t)st.total);
    for (int b = 0; b < LRF_ENC_BODIES; b++) {
        if (!st.count[b]) continue;
        launches.push_back(EncRaggedLaunch{b, (long)blocks.size(), st.count[b], b == ENC_TILE16 ? 0 : (int)((st.count[b] + 7) / 8)});
        for (size_t i = 0; i < st.descs.size(); i++) {
            if (st.descs[i].body != b) continue;
            for (long u = 0; u < st.units[i]; u++) blocks.push_back(RaggedBlock{(int)i, (int)u});
        }
    }
}

EncRaggedPlan plan_encode_ragged(const std::vector<EncRaggedImage>& images, const PlanSettings& s)
{
    EncRaggedPlan p;
    const size_t n = images.size();
    PlanesStage st = planes_stage_descs(images);
    long bcd_blocks = 0;
    int rmax_t = 1;
    for (size_t i = 0; i < n; i++)
        for (int ch = 0; ch < 3; ch++) {
            bcd_blocks += (st.descs[i].g.p[ch].M + LRF_KC - 1) / LRF_KC;
            rmax_t = images[i].R[ch] > rmax_t ? images[i].R[ch] : rmax_t;
        }
    if (bcd_blocks >= (1L << 31) || st.total >= (1L << 31)) {
        p.too_many = bcd_blocks > st.total ? bcd_blocks : st.total;
        return p;
    }
    planes_stage_launches(st, p.launches, p.blocks);
    p.descs.swap(st.descs);
    p.x_floats = st.x_floats;
    p.split = plan_splits(bcd_blocks, rmax_t, s);
    p.order.reserve(3 * n);
    for (int fam = 0; fam < (p.split ? 3 : 1); fam++)
        for (int ch = 0; ch < 3; ch++)
            for (size_t i = 0; i < n; i++)
                if (!p.split || fam_of_rank(images[i].R[ch]) == fam) p.order.push_back(EncRaggedPlane{(int)i, ch});
    for (const EncRaggedPlane& o : p.order) {
        const EncRaggedImage& im = images[(size_t)o.image];
        const ImageGeom& g = p.descs[(size_t)o.image].g;
        long uo = im.u_off, vo = im.v_off, so = im.sign_off;
        for (int c2 = 0; c2 < o.ch; c2++) {
            uo += (long)g.p[c2].M * im.R[c2];
            vo += 64L * im.R[c2];
            so += im.R[c2];
        }
        add_plane(p.t, p.descs[(size_t)o.image].x_off + g.p[o.ch].xoff, uo, vo, 0, 0, g.p[o.ch].M, im.R[o.ch], im.sign_off < 0 ? -1 : (int)so);
    }
    return p;
}

// ---- the tables of a ragged sweep -------------------------------------------------------------------------------------------------
// The planes stage is plan_encode_ragged's for the list of images (its kernels do not look at ranks).  Behind it the call is a
// table of 3 m planes on 3 n matrices: per (image, channel) the first candidate of the largest rank computes the initialisation
// (and alone owns Gram chunks: finish_gram_chunks), the others name it in init_src and take its leading columns (k_init_share).
EncRaggedSweepPlan plan_encode_ragged_sweep(const std::vector<EncSweepImage>& images, const std::vector<EncSweepCand>& cands, const PlanSettings& s)
{
    EncRaggedSweepPlan p;
    const size_t n = images.size(), m = cands.size();
    p.rmax.assign(3 * n, 0);
    std::vector<int> base(3 * n, -1); // the candidate that initialises (image, channel)
    int rmax_t = 1;
    for (size_t j = 0; j < m; j++)
        for (int ch = 0; ch < 3; ch++) {
            const size_t k = 3 * (size_t)cands[j].image + ch;
            if (cands[j].R[ch] > p.rmax[k]) { p.rmax[k] = cands[j].R[ch]; base[k] = (int)j; }
            rmax_t = cands[j].R[ch] > rmax_t ? cands[j].R[ch] : rmax_t;
        }
    std::vector<EncRaggedImage> ims(n);
    for (size_t i = 0; i < n; i++) {
        EncRaggedImage& e = ims[i];
        e.H = images[i].H; e.W = images[i].W;
        for (int ch = 0; ch < 3; ch++) e.R[ch] = p.rmax[3 * i + ch];
        e.rgb_off = images[i].rgb_off; e.u_off = e.v_off = 0; e.sign_off = images[i].sign_off;
        e.aligned8 = images[i].aligned8;
    }
    PlanesStage st = planes_stage_descs(ims);
    long bcd_blocks = 0; // of the candidates' table: the only plane table this call has
    for (size_t j = 0; j < m; j++)
        for (int ch = 0; ch < 3; ch++) bcd_blocks += (st.descs[(size_t)cands[j].image].g.p[ch].M + LRF_KC - 1) / LRF_KC;
    if (bcd_blocks >= (1L << 31) || st.total >= (1L << 31)) {
        p.too_many = bcd_blocks > st.total ? bcd_blocks : st.total;
        return p;
    }
    planes_stage_launches(st, p.launches, p.blocks);
    p.descs.swap(st.descs);
    p.x_floats = st.x_floats;
    p.split = plan_splits(bcd_blocks, rmax_t, s);
    p.order.reserve(3 * m);
    for (int fam = 0; fam < (p.split ? 3 : 1); fam++)
        for (int self = 1; self >= 0; self--)
            for (int ch = 0; ch < 3; ch++)
                for (size_t j = 0; j < m; j++) {
                    if (p.split && fam_of_rank(cands[j].R[ch]) != fam) continue;
                    if ((base[3 * (size_t)cands[j].image + ch] == (int)j) != (self == 1)) continue;
                    p.order.push_back(EncSweepPlane{(int)j, ch});
                }
    std::vector<int> base_plane(3 * n, -1);
    for (const EncSweepPlane& o : p.order) {
        const EncSweepCand& cd = cands[(size_t)o.cand];
        const size_t i = (size_t)cd.image;
        const ImageGeom& g = p.descs[i].g;
        long uo = cd.u_off, vo = cd.v_off, so = images[i].sign_off;
        for (int c2 = 0; c2 < o.ch; c2++) {
            uo += (long)g.p[c2].M * cd.R[c2];
            vo += 64L * cd.R[c2];
            so += p.rmax[3 * i + c2];
        }
        if (base[3 * i + o.ch] == o.cand) base_plane[3 * i + o.ch] = (int)p.t.planes.size();
        add_plane(p.t, p.descs[i].x_off + g.p[o.ch].xoff, uo, vo, 0, 0, g.p[o.ch].M, cd.R[o.ch], images[i].sign_off < 0 ? -1 : (int)so);
    }
    for (size_t pi = 0; pi < p.t.planes.size(); pi++)
        p.t.planes[pi].init_src = base_plane[3 * (size_t)cands[(size_t)p.order[pi].cand].image + p.order[pi].ch];
    return p;
}

// ---- the tables of a ragged gray sweep ----------------------------------------------------------------------------------------------
GrayEncRefusal describe_gray_encode(int64_t n, const lrf_gray_sweep_image* images, int64_t m, const lrf_gray_sweep_candidate* cands,
                                    const GrayEncCall& k, std::vector<EncGrayImage>& ims, std::vector<EncGrayCand>& cs)
{
    ims.clear();
    cs.clear();
    if (n < 1 || n > 65535) return GrayEncRefusal{GENC_N, 0, n, 0, 0};
    if (m < n || m > (1 << 20)) return GrayEncRefusal{GENC_M, 0, m, 0, 0};
    std::vector<EncGrayImage> im_out((size_t)n);
    std::vector<int64_t> Ms((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const lrf_gray_sweep_image& im = images[i];
        if (im.H < 1 || im.W < 1 || im.H > (1 << 20) || im.W > (1 << 20)) return GrayEncRefusal{GENC_SIZE, 0, i, im.H, im.W};
        const int64_t ph = (8 - im.H % 8) % 8, pw = (8 - im.W % 8) % 8;
        if (ph / 2 >= im.H || ph - ph / 2 >= im.H || pw / 2 >= im.W || pw - pw / 2 >= im.W) return GrayEncRefusal{GENC_GEOM, 0, i, im.H, im.W};
        if (im.H * im.W >= (1LL << 31)) return GrayEncRefusal{GENC_PIXELS, 0, i, im.H, im.W};
        if (im.gray_off < 0 || im.sign_off < -1) return GrayEncRefusal{GENC_NEGATIVE, 0, i, 0, 0};
        const int64_t bytes = im.H * im.W;
        if (bytes > k.gray_len || im.gray_off > k.gray_len - bytes) return GrayEncRefusal{GENC_GRAY, 0, i, k.gray_len, 0};
        Ms[(size_t)i] = ((im.H + ph) / 8) * ((im.W + pw) / 8);
        EncGrayImage& e = im_out[(size_t)i];
        e.H = (long)im.H; e.W = (long)im.W;
        e.gray_off = (long)im.gray_off;
        e.sign_off = k.sign_len > 0 && im.sign_off >= 0 ? (long)im.sign_off : -1;
        e.aligned16 = ((k.gray_base + (uintptr_t)im.gray_off) & 15) == 0;
    }
    if (k.K < 1) return GrayEncRefusal{GENC_K, 0, 0, k.K, 0};
    if (k.lo > k.hi || k.lo < -128 || k.hi > 127) return GrayEncRefusal{GENC_BOUNDS, 0, 0, k.lo, k.hi};
    std::vector<EncGrayCand> c_out((size_t)m);
    std::vector<int> rmax((size_t)n, 0);
    struct Range { int64_t off, len; };
    std::vector<Range> ur((size_t)m), vr((size_t)m);
    for (int64_t j = 0; j < m; j++) {
        const lrf_gray_sweep_candidate& cd = cands[j];
        if (cd.image < 0 || cd.image >= n) return GrayEncRefusal{GENC_IMAGE, 1, j, cd.image, 0};
        if (cd.R < 1) return GrayEncRefusal{GENC_RANK_LOW, 1, j, cd.R, 0};
        if (cd.R > LRF_BIG_TO_ANY_RANK) return GrayEncRefusal{GENC_RANK_BIG, 1, j, cd.R, 0};
        if (cd.u_off < 0 || cd.v_off < 0) return GrayEncRefusal{GENC_NEGATIVE, 1, j, 0, 0};
        const int64_t u_img = Ms[(size_t)cd.image] * cd.R, v_img = 64LL * cd.R; // (M < 2^25 + ...: no wrap)
        if (u_img > k.u_len || cd.u_off > k.u_len - u_img) return GrayEncRefusal{GENC_U, 1, j, k.u_len, 0};
        if (v_img > k.v_len || cd.v_off > k.v_len - v_img) return GrayEncRefusal{GENC_V, 1, j, k.v_len, 0};
        c_out[(size_t)j] = EncGrayCand{cd.image, cd.R, (long)cd.u_off, (long)cd.v_off};
        if (cd.R > rmax[(size_t)cd.image]) rmax[(size_t)cd.image] = cd.R;
        ur[(size_t)j] = Range{cd.u_off, u_img};
        vr[(size_t)j] = Range{cd.v_off, v_img};
    }
    for (int64_t i = 0; i < n; i++) {
        if (rmax[(size_t)i] == 0) return GrayEncRefusal{GENC_NO_CAND, 0, i, 0, 0};
        const int64_t s = rmax[(size_t)i];
        if (im_out[(size_t)i].sign_off >= 0 && (s > k.sign_len || im_out[(size_t)i].sign_off > k.sign_len - s || k.sign_len > INT32_MAX))
            return GrayEncRefusal{GENC_SIGN, 0, i, k.sign_len, 0};
    }
    for (std::vector<Range>* r : {&ur, &vr}) { // no two candidates may share output bytes
        std::sort(r->begin(), r->end(), [](const Range& a, const Range& b) { return a.off < b.off; });
        for (size_t i = 1; i < r->size(); i++)
            if ((*r)[i].off - (*r)[i - 1].off < (*r)[i - 1].len) return GrayEncRefusal{r == &ur ? GENC_OVERLAP_U : GENC_OVERLAP_V, 1, 0, (*r)[i].off, 0};
    }
    ims.swap(im_out);
    cs.swap(c_out);
    return GrayEncRefusal{};
}

// The planes stage: the ENC_GRAY16 images share one launch, the others another; a workgroup finds its image and its 256 items
// through blocks[i].  Behind it the call is a table of m planes on n matrices: per image the first candidate of the largest
// rank computes the initialisation (and alone owns Gram chunks: finish_gram_chunks), the others name it in init_src and take
// its leading columns (k_init_share).
EncGraySweepPlan plan_encode_gray_ragged_sweep(const std::vector<EncGrayImage>& images, const std::vector<EncGrayCand>& cands, const PlanSettings& s)
{
    static_assert(sizeof(EncGrayDesc) == 2 * sizeof(long) + 6 * sizeof(int), "EncGrayDesc has padding bytes: they would be part of the table's key");
    EncGraySweepPlan p;
    const size_t n = images.size(), m = cands.size();
    std::vector<EncGrayDesc> descs(n, EncGrayDesc{});
    std::vector<int> body(n), Ms(n);
    std::vector<long> units(n);
    long count[2] = {0, 0}, x_floats = 0;
    for (size_t i = 0; i < n; i++) {
        const EncGrayImage& im = images[i];
        EncGrayDesc& d = descs[i];
        const long ph = (8 - im.H % 8) % 8, pw = (8 - im.W % 8) % 8;
        const long nh = (im.H + ph) / 8, nw = (im.W + pw) / 8;
        Ms[i] = (int)(nh * nw);
        d.gray_off = im.gray_off;
        d.x_off = x_floats;
        x_floats += 64L * Ms[i];
        d.H = (int)im.H; d.W = (int)im.W;
        d.top = (int)(ph / 2); d.left = (int)(pw / 2);
        d.nw = (int)nw;
        body[i] = im.W % 16 == 0 && im.aligned16 ? ENC_GRAY16 : ENC_GRAY_ANY;
        d.items = body[i] == ENC_GRAY16 ? (int)(nh * (im.W / 16) * 8) : 16 * Ms[i];
        units[i] = ((long)d.items + 255) / 256;
        count[body[i]] += units[i];
    }
    p.rmax.assign(n, 0);
    std::vector<int> base(n, -1); // the candidate that initialises the image
    int rmax_t = 1;
    long bcd_blocks = 0; // of the candidates' table: the only plane table this call has
    for (size_t j = 0; j < m; j++) {
        const size_t i = (size_t)cands[j].image;
        if (cands[j].R > p.rmax[i]) { p.rmax[i] = cands[j].R; base[i] = (int)j; }
        rmax_t = cands[j].R > rmax_t ? cands[j].R : rmax_t;
        bcd_blocks += (Ms[i] + LRF_KC - 1) / LRF_KC;
    }
    if (bcd_blocks >= (1L << 31) || count[0] >= (1L << 31) || count[1] >= (1L << 31)) {
        p.too_many = bcd_blocks;
        for (long cnt : count) p.too_many = cnt > p.too_many ? cnt : p.too_many;
        p.rmax.clear();
        return p;
    }
    p.blocks.reserve((size_t)(count[0] + count[1]));
    for (int b = 0; b < 2; b++) {
        if (!count[b]) continue;
        p.launches.push_back(EncGrayLaunch{b, (long)p.blocks.size(), count[b]});
        for (size_t i = 0; i < n; i++) {
            if (body[i] != b) continue;
            for (long u = 0; u < units[i]; u++) p.blocks.push_back(RaggedBlock{(int)i, (int)u});
        }
    }
    p.descs.swap(descs);
    p.x_floats = x_floats;
    p.split = plan_splits(bcd_blocks, rmax_t, s);
    p.order.reserve(m);
    for (int fam = 0; fam < (p.split ? 3 : 1); fam++)
        for (int self = 1; self >= 0; self--)
            for (size_t j = 0; j < m; j++) {
                if (p.split && fam_of_rank(cands[j].R) != fam) continue;
                if ((base[(size_t)cands[j].image] == (int)j) != (self == 1)) continue;
                p.order.push_back((int)j);
            }
    std::vector<int> base_plane(n, -1);
    for (int j : p.order) {
        const EncGrayCand& cd = cands[(size_t)j];
        const size_t i = (size_t)cd.image;
        if (base[i] == j) base_plane[i] = (int)p.t.planes.size();
        add_plane(p.t, p.descs[i].x_off, cd.u_off, cd.v_off, 0, 0, Ms[i], cd.R, images[i].sign_off < 0 ? -1 : (int)images[i].sign_off);
    }
    for (size_t pi = 0; pi < p.t.planes.size(); pi++) p.t.planes[pi].init_src = base_plane[(size_t)cands[(size_t)p.order[pi]].image];
    return p;
}

// ---- inflate of factor columns -------------------------------------------------------------------------------------------------
std::vector<InflateSlot> plan_inflate(const std::vector<InflateMatDim>& mats)
{
    std::vector<int> order(mats.size());
    for (size_t i = 0; i < mats.size(); i++) order[i] = (int)i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        if (mats[(size_t)a].rows != mats[(size_t)b].rows) return mats[(size_t)a].rows > mats[(size_t)b].rows;
        if (mats[(size_t)a].cols != mats[(size_t)b].cols) return mats[(size_t)a].cols > mats[(size_t)b].cols;
        return a < b;
    });
    std::vector<InflateSlot> slots;
    for (int m : order)
        for (int j = 0; j < mats[(size_t)m].cols; j++) slots.push_back(InflateSlot{m, j});
    return slots;
}
