// lrf_plan.h — the descriptor tables of a call of the 64-column path and its launch plan: which kernel iterates which planes,
// whether one persistent launch takes the iterations, how the kernel families share streams.  Decided once per call by
// plan_bcd (lrf_plan.cpp), executed by run_init / run_bcd (lrf_encode8.hip), bcd32_update_u (lrf_bcd32.hip) and bcdp_launch
// (lrf_bcd_persist.hip).  No device, no context, no HIP: the host compiler alone builds it (tests/test_bcd_plan.py does).
#ifndef LRF_PLAN_H
#define LRF_PLAN_H
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "../../include/lrf_hip.h"
#include "lrf_internal.h"

// largest rank of the 64-column BCD kernels (k_bcd_w <= 8, k_bcd <= 16, k_bcd_mid <= 32); above it the any-shape kernels iterate
#define LRF_BIG_TO_ANY_RANK 32
#define LRF_BCDW_MIN_BLOCKS 1024 // smaller rank <= 8 runs iterate on the workgroup kernel k_bcd (plan_bcd)
#define LRF_BCDW16_MIN_BLOCKS 1024 // likewise for rank <= 16 runs and k_bcd_w16
#define LRF_BCDW32_MIN_BLOCKS 128  // likewise for rank 17..32 runs and k_bcd_w32 / k_bcd_w32f (12 images: 1.06 -> 0.99 ms at (20,10,10))
#define LRF_PERSIST_MIN_BLOCKS 3584 // a call of this many blocks runs its iterations in one launch (k_bcd_p) ...
#define LRF_PERSIST_MIN_BLOCKS_ONE_FAMILY 2304 // ... of this many when all its planes are of one rank family
// X bytes (10^6) of a k_bcd_p call that stay on the default cache policy (plan_x_residency): the 256 MiB (268 MB) Infinity Cache
// less the hand-off lines of a pass (U rows, partials, tables: ~30 MB at 256 x 512x768) and a margin.  Measured on 512x768 images
// at ranks (7,3,3), policy against plain loads: 104 / 112 images (204 / 220 MB a pass) lose 0.7 / 1.1 % under the policy — they
// still fit —, 120 (236 MB) gain 0.5 %, 128 (252 MB) 2.2 %, 256 (503 MB, 201 MB of chroma X kept) 5.7 %
#define LRF_X_KEEP_MB_DEFAULT 230

// ---- descriptor tables ------------------------------------------------------------------------
struct Tables {
    std::vector<PlaneDesc> planes;
    std::vector<BlockDesc> blocks;
    std::vector<GramChunk> gchunks; // the chunks k_gram64 computes first, then those of the gram_fused planes (k_planes16_gram)
    int ngram_rest = 0;             // how many of them k_gram64 computes (finish_gram_chunks)
};
void add_plane(Tables& t, long x_off, long u_off, long v_off, long u0_off, long v0_off, int M, int R, int sign_off);

// ---- what the plan depends on besides the call: read once per process (plan_settings_env), persist_arch from the device
struct PlanSettings {
    int persist = -1;              // LRF_PERSIST                    (these four: the test hooks of lrf_env.h)
    long family_split_blocks = -1; // LRF_FAMILY_SPLIT_BLOCKS
    long bcdw16_min_blocks = LRF_BCDW16_MIN_BLOCKS, bcdw32_min_blocks = LRF_BCDW32_MIN_BLOCKS; // the variables of these names
    // developer switches (-DLRF_DEV builds only): LRF_BCD_WG (the workgroup kernels instead of the wave kernels), LRF_NO_FAMILY_SPLIT,
    // LRF_NO_FAMILY_STREAMS, LRF_NO_BCDW32 (k_bcd_mid instead), LRF_GENERIC_GS (never the exact-integer Gauss-Seidel), LRF_NO_PERSIST_FIRST, LRF_NO_INIT_FORK
    bool bcd_wg = false, no_family_split = false, no_family_streams = false, no_bcdw32 = false, generic_gs = false, no_persist_first = false, no_init_fork = false;
    bool persist_arch = false; // the device is the part the in-launch hand-offs of k_bcd_p were validated on (gfx950)
    int luma_bytes = -1;       // LRF_LUMA_BYTES (lrf_env.h): 0 = no call reads luma from the image bytes; else every eligible one
    long x_keep_bytes = LRF_X_KEEP_MB_DEFAULT * 1000000L; // LRF_X_KEEP_MB x 10^6 (plan_x_residency): 0 = no residency policy
};
const PlanSettings& plan_settings_env(); // the environment's part (persist_arch false)

// ---- the plan ---------------------------------------------------------------------------------
inline int fam_of_rank(int R) { return LRF_FAM_OF_RANK(R); }
inline long bounds_mx(int lo, int hi) { return labs((long)lo) > labs((long)hi) ? labs((long)lo) : labs((long)hi); } // mx = max(|lo|, |hi|)

// the U-update kernels; arg: the pair count NP of k_bcd_w32<NP>, the rank of k_bcd_w32f<R>, 0 otherwise
enum BcdKernel { BCD_K_WG8, BCD_K_WG16, BCD_K_MID, BCD_K_W, BCD_K_W16, BCD_K_W32, BCD_K_W32F };
struct BcdChoice { BcdKernel k; int arg; };
// A run: consecutive planes (and their blocks) that iterate on one kernel family — 0: rank <= 8, 1: rank <= 16, 2: rank <= 32
// — with that family's table pitch (16 or LRF_RPB).  Pitch-16 runs of a call whose table pitch is LRF_RPB use the second
// table set (vf16 ...): the regions of the two pitches would overlap in one buffer.
struct FamRun {
    int plane0, nplanes, block0, nblocks, rmax, fam, pitch;
    int rmin;        // smallest rank of the run (k_bcd_w32 takes runs whose ranks are all 17..32)
    bool any_native; // some plane of the run is small enough for ATen's native order of `uu @ bb` ((R-1) M < 400)
    int nbase;       // leading planes of the run that compute their own SVD initialisation (all of them, except in a sweep call:
                     // there the other planes take their columns from a plane of the same matrix, PlaneDesc::init_src)
    bool exact_int;  // GsParams::exact_int of the run's launches
    BcdChoice first, later; // the U update of the first iteration (old U by the plan's first_mode) and of iterations >= 2
};
enum FamStreams { FAM_STREAMS_NONE, FAM_STREAMS_INIT, FAM_STREAMS_CALL }; // the runs on streams of their own: never / the initialisation kernels / to the call's end
enum { PLAN_INIT_ONLY = 0, PLAN_FIRST_W0 = 1, PLAN_FIRST_U0 = 2 }; // first_mode: no iterations (runs and pitches only) / old U = X W0 of the initialisation / the caller's U0
struct BcdPlan {
    int K = 0, lo = 0, hi = 0, first_mode = PLAN_INIT_ONLY;
    std::vector<FamRun> runs;
    int rmax = 1, rp = 16; // largest rank of the table; padded rank of its V / W / partial tables: 16 (one MFMA tile) or LRF_RPB
    bool split = false, mixed = false; // every plane on the kernel family of its own rank (plan_splits); runs of both table pitches occur
    // persist: one launch of k_bcd_p<f16, np32, first> for iterations 2..K — or all K (first: the call's first iteration inside too)
    bool persist = false, persist_first = false;
    bool persist_f16 = false;   // planes of ranks 9..16 occur (the instantiations with ranks 17..32 carry that body too: their chroma planes)
    int persist_np32 = 0;       // pairs of rank columns of the planes of ranks 17..32 (0: none)
    FamStreams streams = FAM_STREAMS_NONE;
    // the luma blocks of k_bcd_p read the caller's image bytes, not X (plan_luma_bytes; set by lrf_qmf_encode_rgb_u8 alone)
    bool luma_bytes = false;
    LumaSrc luma = {nullptr, 0, 0, 0, 0};
};
// whether a call of that size gives every plane the kernel family of its own rank (the sweep entry point orders its planes by it)
bool plan_splits(long nblocks, int rmax_t, const PlanSettings& s);
// reads R, nblk, native_t2_u and init_src of the planes.  sweep: lrf_qmf_encode_sweep_rgb_u8's table
BcdPlan plan_bcd(const std::vector<PlaneDesc>& planes, int K, int lo, int hi, int first_mode, const PlanSettings& s, bool sweep = false);

// ---- luma from the image bytes: a luma element of X is ycc_of(r, g, b, 0), a pure function of three bytes that k_bcd_p would
// read as four from X, K times a call.  Whether the fused encode (lrf_qmf_encode_rgb_u8, nobody else) lets the rank <= 8 body of
// k_bcd_p<false, 0, true> take the luma matrices from the caller's [3][H][W] bytes:
//   * k_planes16's geometry (planes_gram_eligible's, without its batch size): H and W multiples of 16, the bytes 8-byte aligned,
//     3 H W < 2^31;
//   * the plan runs ALL iterations in that instantiation (persist && persist_first, no plane above rank 8 — so every luma plane
//     is of rank family 0), for nobody else reads luma X after the planes kernel;
//   * the bytes stay the caller's to the end of the call: not under a pipe, which frees its upload slot behind the planes
//     kernel (`rgb_released`: lrf_ctx::planes_done is set);
//   * LRF_LUMA_BYTES is not 0.
// nluma: the leading planes of the table that are the images' luma planes, image i at plane i (encode_rgb_prepare's order).
bool plan_luma_bytes(const BcdPlan& p, const std::vector<PlaneDesc>& planes, int nluma, int64_t H, int64_t W, uintptr_t rgb_addr, bool rgb_released,
                     const PlanSettings& s);

// ---- which X stays in the Infinity Cache: k_bcd_p reads every X source of the call once per iteration, K times a call.  What
// fits the cache between two passes is served on-die from the second pass on — but only if the sources that cannot fit do not
// pass through the cache on their way (BlockDesc::x_nt: non-temporal loads, which also land sooner than plain ones).
//   * A call whose sources all fit the budget — luma as it is read, three bytes an element from the image (`luma_from_bytes`) or
//     four from X, plus the chroma planes' X — is left alone: nothing is marked, every load is plain, as without the policy.
//   * Otherwise, in table order, the planes behind the `nluma` leading luma planes — the chroma planes, whose X is fp32 in
//     every call — are KEPT (plain loads) while their X bytes, added up, stay within the budget; every other block of the call
//     streams: luma, from the image bytes or from fp32 X (four times a chroma plane: in a call that does not fit, the part that
//     cannot), and the planes from the first that passes the budget on.  Luma is never among the kept planes.
// The policy applies to calls that k_bcd_p's rank <= 8 body alone iterates (plan.persist, no plane above rank 8) outside a pipe
// (`piped`: two contexts' kernels share the cache); elsewhere, and with a budget of 0, no block is marked and every load is
// plain.  Sets BlockDesc::x_nt of every block of the table; the plane table is not touched.
struct XResidency {
    int kept_planes = 0;  // planes whose X loads plain under the policy
    long kept_bytes = 0;  // their X bytes
    bool on = false;      // the policy applies: the other blocks are marked x_nt
};
XResidency plan_x_residency(const BcdPlan& p, Tables& t, int nluma, bool luma_from_bytes, bool piped, const PlanSettings& s);

// ---- decode: which body serves an image, and the launches of a ragged call (lrf_qmf_decode_ragged_rgb_u8) ------------------
enum { DEC_TILE16 = 0, DEC_STRIP = 1, DEC_R8 = 2, DEC_ANY = 3 }; // decode_plan decides
#define LRF_DEC_CLASSES 5 // rank-bound classes of the tiled bodies
// which decode body serves a geometry and a rank triple: every decode and SSE entry of lrf_encode8.hip rests on it
struct DecodePlan {
    int kind;
    int cls; // tiled kinds: index of the rank bounds (chroma, luma) = (4,8) (8,8) (8,16) (16,16) (16,32)
};
// aligned8: the image's output bytes start at a multiple of 8 (DEC_TILE16 stores 8 bytes at a time; entries that only read the
// bytes, or store through windows, pass true).  no_tiled: the developer switch LRF_DECODE_NO_TILED
DecodePlan decode_plan(const ImageGeom& g, int64_t H, int64_t W, const int R[3], bool aligned8, bool no_tiled = false);
// groups of four pixels per thread of k_decode8 / k_sse8 for a launch of `groups256` groups of 256 pixel quads: as many as leave
// it ~2048 workgroups (small launches keep one group per thread)
inline long decode8_reps_of(long groups256)
{
    const long reps = groups256 / 2048;
    return reps < 1 ? 1 : (reps > 16 ? 16 : reps);
}
// One image of a ragged call as decode_plan classified it.  units: its tiles (DEC_TILE16, DEC_STRIP) or its pixel quads
// H ceil(W / 4) (DEC_R8, DEC_ANY)
struct RaggedWork {
    int kind, cls;
    long units;
};
struct RaggedLaunch {
    int kind;
    int cls;              // DEC_STRIP: the launch's class; DEC_TILE16: -1 (the kernel switches on the image's class); else 0
    long block0, nblocks; // its workgroups: entries block0 .. block0 + nblocks - 1 of the block table
    int reps;             // DEC_R8: pixel quads per thread (decode8_reps_of the launch's total), else 1
};
struct RaggedPlan {
    std::vector<RaggedLaunch> launches; // order: DEC_TILE16, DEC_STRIP by class, DEC_R8, DEC_ANY; at most 3 + LRF_DEC_CLASSES
    std::vector<RaggedBlock> blocks;    // per launch the images in call order, an image's tiles ascending
    long too_many = 0;                  // != 0: a launch would have this many (>= 2^31) workgroups; no table is built
};
RaggedPlan plan_decode_ragged(const std::vector<RaggedWork>& images);

// ---- the image list of a decode or SSE entry: checked, and described as the kernels read it -----------------------------------
// Everything the kernels index the factors with comes from RaggedDesc alone, so this is the one place between a caller's numbers
// and an out-of-bounds read.  Checks per image, in this order: the size, the geometry (geom_of), the ranks 1..64, negative
// offsets, the U and the V extent against u_len / v_len (every term is checked against the length before it is added to an
// offset: no sum can wrap), and — check_rgb — rgb_off and the image's [3][H][W] against rgb_len.
enum { DESC_OK = 0, DESC_SIZE, DESC_GEOM, DESC_RANK, DESC_NEGATIVE, DESC_U, DESC_V, DESC_RGB };
struct DescribeOptions {
    bool check_rgb = false;   // the entry reads or writes full-size images at rgb_off: checked, and copied into the descriptor
    int64_t rgb_len = 0;
    bool aligned8 = true;     // every image counts as 8-byte aligned; false: image i is when (rgb_base + rgb_off) % 8 == 0
    uintptr_t rgb_base = 0;
    bool no_tiled = false;    // LRF_DECODE_NO_TILED (decode_plan)
};
// the first offender: which check, which image, and what its message needs (DESC_SIZE, DESC_GEOM: H, W; DESC_RANK: the rank;
// DESC_U, DESC_V, DESC_RGB: the buffer's length)
struct DescribeRefusal {
    int check = DESC_OK;
    int64_t image = 0, a = 0, b = 0;
};
// descs: n descriptors, zeroed first (their bytes are the device table's key: padding included); rgb_off stays 0 without
// check_rgb.  work: if given, (kind, cls, units) per image for plan_decode_ragged / plan_decode_crops.  On a refusal both are
// left unspecified.
DescribeRefusal describe_images(int64_t n, const lrf_ragged_image* images, int64_t u_len, int64_t v_len, const DescribeOptions& o,
                                std::vector<RaggedDesc>& descs, std::vector<RaggedWork>* work = nullptr);

// ---- metrics of pairs that differ in size: the tables and launches of lrf_image_metrics_ragged_u8, and the chunks of -----------
// lrf_qmf_ssim_ragged_rgb_u8 (kernels: lrf_metrics_ragged_kernel.hip).  tests/test_metrics_ragged_plan.py reads them on the CPU.
#define LRF_MTR_TH 24 // window positions per tile: rows and columns (k_ssim_tiles' tiling, lrf_metrics_kernel.hip: LRF_MT_TH, LRF_MT_TW)
#define LRF_MTR_TW 64
#define LRF_MTR_PRE_BYTES (256 * 16 * 8) // bytes per workgroup of the flat read (LRF_MT_PRE_BYTES)
#define LRF_SSIM_SCRATCH_DEFAULT ((int64_t)256 << 20) // lrf_qmf_ssim_ragged_rgb_u8's cap on decoded bytes (scratch_bytes = 0)
inline long metrics_tiles_x(long W) { return (W - 6 + LRF_MTR_TW - 1) / LRF_MTR_TW; }
inline long metrics_tiles_y(long H) { return (H - 6 + LRF_MTR_TH - 1) / LRF_MTR_TH; }
// Checks, in this order: n in [1,65535], C in [1,65535]; per pair: the sides (>= 7 with the SSIM, else >= 1; <= 2^20; fewer than
// 2^40 samples), negative offsets, the a and the b image against a_len / b_len (the extent is compared with the length before
// it is added to an offset: no sum can wrap); then 2^31 or more workgroups in a launch.
enum { MTR_OK = 0, MTR_N, MTR_C, MTR_SIZE, MTR_NEGATIVE, MTR_A, MTR_B, MTR_TOO_MANY };
struct MetricsRefusal {
    int check = MTR_OK;
    int64_t pair = 0, a = 0, b = 0; // MTR_N, MTR_C: the value in a; MTR_SIZE: H, W; MTR_A, MTR_B: the buffer's length; MTR_TOO_MANY: the count
};
struct MetricsCall {
    int C;
    int64_t a_len, b_len;
    uintptr_t a_base, b_base; // the addresses of a and b: with the offsets and W they decide a pair's load width
    bool want_ssim;
};
struct MetricsRaggedPlan {
    MetricsRefusal refusal;             // != MTR_OK: nothing below is built (every vector empty, every count 0)
    std::vector<MetricsPairDesc> pairs; // in call order; wg0: the running sum of C nt — a pair's workgroups are its slots
    // the flat read's ranges: with the SSIM the DISTINCT a images in order of first appearance (pairs of one (a_off, H, W) share
    // an entry: MetricsPairDesc::src), without it the pairs themselves (the squared error of a against b)
    std::vector<MetricsSpanDesc> spans;
    long tile_wgs = 0;                  // workgroups of k_ragged_ssim_tiles = float64 slots (0 without the SSIM)
    long span_wgs = 0;                  // workgroups of k_ragged_metrics_pre
};
MetricsRaggedPlan plan_metrics_ragged(int64_t n, const lrf_image_pair* pairs, const MetricsCall& k);
// The chunks of the factor entry: consecutive items go into one chunk while their decoded bytes — 3 H W each, rounded up to 16 —
// fit `cap`; an item larger than the cap gets a chunk of its own.  sizes: n validated (H, W).  off[i]: bytes from the chunk's
// start to item i's decoded image
struct MetricsChunk { int64_t item0, nitems, bytes; };
struct MetricsChunks {
    std::vector<MetricsChunk> chunks;
    std::vector<int64_t> off;
    int64_t max_bytes = 0; // the largest chunk: what the scratch buffer holds
};
MetricsChunks plan_metrics_chunks(int64_t n, const lrf_ragged_image* items, int64_t cap);

// ---- decode of windows: the launches of lrf_qmf_decode_crops_rgb_u8 and which pixels a thread answers for --------------------
// The windows of a call share one size (h, w), so a launch's grid is uniform: (workgroups per window) x (its windows), the
// workgroups per window being the worst case over the alignments a window can have inside its image; workgroups a window's
// alignment leaves without pixels exit.  The functions below say which image pixels thread `tid` of workgroup `wg` of a window
// keeps: the kernels store exactly those, and tests/test_decode_crops_plan.py checks on the CPU that they tile every window.
#ifdef __HIPCC__
#define LRF_HD __host__ __device__
#else
#define LRF_HD
#endif
// Luma from the image bytes (LumaSrc; k_bcd_p's body and tests/test_luma_bytes_plan.py call the same functions): row m of a luma
// matrix is patch (m / nwl, m % nwl), column n is pixel (n >> 3, n & 7) of that patch; sides multiples of 16, so no padding.
// luma_patch_byte0: the byte offset of the patch's first pixel inside a channel; luma_byte_off: of the byte of channel ch under
// element (m, n), from the image's first byte (3 H W < 2^31: int)
LRF_HD inline int luma_patch_byte0(int m, int W, int nwl)
{
    const int pr = m / nwl, pc = m - pr * nwl;
    return 8 * pr * W + 8 * pc;
}
LRF_HD inline int luma_byte_off(int m, int n, int ch, int hw, int W, int nwl) { return ch * hw + luma_patch_byte0(m, W, nwl) + (n >> 3) * W + (n & 7); }

struct CropSpan { int y, x, ny, nx; }; // image rows y .. y + ny - 1, columns x .. x + nx - 1; ny == 0 or nx == 0: none
// Tiled body: the tiles of decode_strip_tile (16 padded luma rows x 32 luma patches, a thread two rows of one patch), laid from
// the strip and the patch column that hold the window's origin.  h rows touch at most floor((h + 14) / 16) + 1 strips, w
// columns at most floor((w + 6) / 8) + 1 patches.
LRF_HD inline int crop_tiled_per_strip(int w) { return (((w + 6) >> 3) + 1 + 31) / 32; }
LRF_HD inline long crop_tiled_wgs(int h, int w) { return (long)(((h + 14) >> 4) + 1) * crop_tiled_per_strip(w); }
struct CropTile {
    int strip, ww, rp; // padded luma rows 16 strip + 2 rp, + 1 of luma patch column ww
    CropSpan px;       // what of them lies inside the window
};
// top, left: the luma plane's padding above and left of the image (PlaneGeom::top_crop, left_crop)
LRF_HD inline CropTile crop_tile_of(int top, int left, int y0, int x0, int h, int w, int wg, int tid)
{
    const int per_strip = crop_tiled_per_strip(w), s = wg / per_strip;
    CropTile t;
    t.strip = ((y0 + top) >> 4) + s;
    t.ww = ((x0 + left) >> 3) + (wg - s * per_strip) * 32 + (tid & 31);
    t.rp = tid >> 5;
    const long ya = 16L * t.strip + 2 * t.rp - top, xa = 8L * t.ww - left; // (long: a tile past the window may pass 2^31)
    const long ylo = ya > y0 ? ya : y0, yhi = ya + 2 < (long)y0 + h ? ya + 2 : (long)y0 + h;
    const long xlo = xa > x0 ? xa : x0, xhi = xa + 8 < (long)x0 + w ? xa + 8 : (long)x0 + w;
    t.px.ny = yhi > ylo ? (int)(yhi - ylo) : 0;
    t.px.nx = xhi > xlo ? (int)(xhi - xlo) : 0;
    t.px.y = t.px.ny ? (int)ylo : y0;
    t.px.x = t.px.nx ? (int)xlo : x0;
    return t;
}
// whether workgroup wg of a window holds any of its pixels (its first thread's rows and columns start inside the window's)
LRF_HD inline bool crop_tile_wg_live(int top, int left, int y0, int x0, int h, int w, int wg)
{
    const int per_strip = crop_tiled_per_strip(w), s = wg / per_strip;
    const long ya = 16L * (((y0 + top) >> 4) + s) - top, xa = 8L * (((x0 + left) >> 3) + (wg - s * per_strip) * 32) - left;
    return ya < (long)y0 + h && xa < (long)x0 + w;
}
// Quad bodies (rank <= 8 and general): the window's pixel quads, row by row, 256 to a workgroup
LRF_HD inline long crop_quad_wgs(int h, int w) { return ((long)h * ((w + 3) >> 2) + 255) / 256; }
LRF_HD inline CropSpan crop_quad_of(int y0, int x0, int h, int w, int wg, int tid)
{
    const int w4 = (w + 3) >> 2;
    const long o = (long)wg * 256 + tid;
    CropSpan q = {y0, x0, 0, 0};
    if (o >= (long)h * w4) return q;
    const int r = (int)(o / w4), c = (int)(o - (long)r * w4) * 4;
    q.y = y0 + r;
    q.x = x0 + c;
    q.ny = 1;
    q.nx = w - c < 4 ? w - c : 4;
    return q;
}
// One launch: windows crop0 .. crop0 + ncrops - 1 of the sorted table, wgs workgroups each (grid.x = ncrops * wgs).
// kind: DEC_STRIP (the tiled body, images decode_plan gives DEC_TILE16 or DEC_STRIP; cls: its rank-bound class), DEC_R8, DEC_ANY
struct CropLaunch {
    int kind, cls;
    long crop0, ncrops;
    long wgs;
};
struct CropPlan {
    std::vector<CropLaunch> launches; // order: tiled by class, DEC_R8, DEC_ANY; at most LRF_DEC_CLASSES + 2
    std::vector<CropEntry> table;     // the windows grouped by launch, call order inside a group; out = the place in the call
    long too_many = 0;                // != 0: a launch would have this many (>= 2^31) workgroups; no table is built
};
// images: (kind, cls) per image as decode_plan classified it (units unused); crops: (image, y0, x0) in call order, validated
CropPlan plan_decode_crops(const std::vector<RaggedWork>& images, const std::vector<CropEntry>& crops, int h, int w);

// ---- decode at 1/2, 1/4, 1/8 scale: the footprint of an output pixel, the thread maps and the launches of -----------------------
// lrf_qmf_decode_scaled_rgb_u8 / lrf_qmf_decode_scaled_crops_rgb_u8 (kernels: lrf_decode_scaled_kernel.hip) ---------------------
// Output pixel (i, j) of an H x W image at scale f is the mean of image rows scaled_lo(i, f) .. scaled_hi(i, f, H) - 1 and the
// columns likewise: blocks are aligned to the IMAGE, the partial ones at the bottom and right edge hold the pixels that exist.
// The kernels and tests/test_decode_scaled_plan.py call the same functions.
LRF_HD inline bool scaled_f_ok(int f) { return f == 2 || f == 4 || f == 8; }
LRF_HD inline long scaled_dim(long n, int f) { return (n + f - 1) / f; }
LRF_HD inline int scaled_lo(int i, int f) { return i * f; } // (i < ceil(n / f) <= 2^30: no wrap)
LRF_HD inline int scaled_hi(int i, int f, int n) { return (long)i * f + f < n ? i * f + f : n; }
// the nearest-neighbour chroma row (column) under image row (column) y of n, the chroma plane having nc: ATen's rule in fp32, as
// every decoder of lrf_kernels.hip computes it
LRF_HD inline int scaled_chroma_index(int y, int n, int nc)
{
    const float s = (float)nc / (float)n;
    const int q = (int)floorf((float)y * s);
    return q > nc - 1 ? nc - 1 : q;
}
// the chroma row under image row y and how many of the rows y .. yhi - 1 share it (the index is monotone: they are consecutive)
LRF_HD inline int scaled_chroma_run(int y, int yhi, int n, int nc, int* q)
{
    *q = scaled_chroma_index(y, n, nc);
    int m = 1;
    while (y + m < yhi && scaled_chroma_index(y + m, n, nc) == *q) m++;
    return m;
}
// Tiled body (sides multiples of 16): the unit is the chroma patch, 16 x 16 image pixels = (16 / f)^2 output pixels, a thread one
// patch, the patches of a window row by row, 256 to a workgroup.  y0, x0, h, w: the window in scaled coordinates.
struct ScaledTile {
    int pr, pc;  // the chroma patch (row, column): threads past the window's last patch hold that patch and keep nothing
    CropSpan px; // the output pixels it keeps: rows y .. y + ny - 1, columns x .. x + nx - 1 of the scaled image; ny == 0: none
};
LRF_HD inline long scaled_tiled_wgs(int f, int y0, int x0, int h, int w)
{
    const int nc = 16 / f;
    const long npr = (y0 + h - 1) / nc - y0 / nc + 1, npc = (x0 + w - 1) / nc - x0 / nc + 1;
    return (npr * npc + 255) / 256;
}
LRF_HD inline ScaledTile scaled_tile_of(int f, int y0, int x0, int h, int w, long wg, int tid)
{
    const int nc = 16 / f, pr0 = y0 / nc, pc0 = x0 / nc;
    const long npr = (y0 + h - 1) / nc - pr0 + 1, npc = (x0 + w - 1) / nc - pc0 + 1;
    long o = wg * 256 + tid;
    const bool live = o < npr * npc;
    if (!live) o = npr * npc - 1;
    ScaledTile t;
    t.pr = pr0 + (int)(o / npc);
    t.pc = pc0 + (int)(o % npc);
    const int ya = t.pr * nc > y0 ? t.pr * nc : y0, yb = (long)t.pr * nc + nc < (long)y0 + h ? t.pr * nc + nc : y0 + h;
    const int xa = t.pc * nc > x0 ? t.pc * nc : x0, xb = (long)t.pc * nc + nc < (long)x0 + w ? t.pc * nc + nc : x0 + w;
    t.px.y = ya; t.px.x = xa;
    t.px.ny = live ? yb - ya : 0;
    t.px.nx = live ? xb - xa : 0;
    return t;
}
// General body: a thread one output pixel, the window's pixels row by row, 256 to a workgroup
LRF_HD inline long scaled_any_wgs(int h, int w) { return ((long)h * w + 255) / 256; }
LRF_HD inline CropSpan scaled_pixel_of(int y0, int x0, int h, int w, long wg, int tid)
{
    const long o = wg * 256 + tid;
    CropSpan q = {y0, x0, 0, 0};
    if (o >= (long)h * w) return q;
    q.y = y0 + (int)(o / w);
    q.x = x0 + (int)(o % w);
    q.ny = q.nx = 1;
    return q;
}
// One image as the entry points classified it: tiled = both sides multiples of 16 and ranks inside the tiled decoders' bounds
// (decode_plan's DEC_TILE16), cls its rank-bound class there; R: its ranks (they size its pooled tables)
struct ScaledImage { int tiled, cls, R[3]; };
inline ScaledImage scaled_image_of(const RaggedDesc& d) { return ScaledImage{d.kind == DEC_TILE16, d.cls, {d.R0, d.R1, d.R2}}; }
// int16 elements of the pooled tables of one image at scale f: luma [R_Y][(8/f)^2], then Cb and Cr [R_c][(16/f)^2]
inline long scaled_pool_elems(const int R[3], int f) { return (long)R[0] * (8 / f) * (8 / f) + (long)(R[1] + R[2]) * (16 / f) * (16 / f); }
// One launch: items item0 .. item0 + nitems - 1 of the sorted table, wgs workgroups each (grid.x = nitems * wgs; wgs: the most
// an item of the launch needs, the workgroups an item does not need exit)
struct ScaledLaunch {
    int tiled, f, cls; // cls: tiled launches, else 0
    long item0, nitems, wgs;
};
struct ScaledPoolJob { int image, f; long pool_off; }; // k_pool_v: one workgroup per (image, scale) of the tiled items
struct ScaledPlan {
    std::vector<ScaledLaunch> launches; // order: tiled by (f, class), then general by f; at most LRF_SCALED_MAX_LAUNCHES
    std::vector<ScaledItem> table;      // the items grouped by launch, call order inside a group; place = the place in the call
    std::vector<ScaledPoolJob> jobs;    // in order of first use by the table
    long pool_elems = 0;                // int16 elements of the pooled-table workspace
    long too_many = 0;                  // != 0: a launch would have this many (>= 2^31) workgroups; no table is built
};
#define LRF_SCALED_MAX_LAUNCHES (3 * LRF_DEC_CLASSES + 3)
// items: validated, in call order (place and pool_off are set here)
ScaledPlan plan_decode_scaled(const std::vector<ScaledImage>& images, const std::vector<ScaledItem>& items);

// ---- resized crops: boxes of any size resampled to one output size (lrf_qmf_decode_resized_crops_rgb_u8; kernels: -------------
// lrf_decode_resized_kernel.hip).  The kernels and tests/test_decode_resized_plan.py call the same functions. -------------------
// The level a box is sampled from: the largest f of 8, 4, 2 whose f x output still fits inside the box, else 1 (the full image)
LRF_HD inline int resized_level(int hb, int wb, int oh, int ow)
{
    for (int f = 8; f >= 2; f >>= 1)
        if ((long)f * oh <= hb && (long)f * ow <= wb) return f;
    return 1;
}
// The two level rows (columns) output row (column) r of n_out reads and the weight of the second in 1/256: the centre of
// output sample r lies at ((r + 1/2) nb / n_out + b0) / f - 1/2 of the level, floored to 1/256 and clamped into the level
struct ResizedTap { int i0, i1, t; };
LRF_HD inline ResizedTap resized_tap(int r, int n_out, int b0, int nb, int f, int n_lvl)
{
    const long long N = (2LL * r + 1) * nb + 2LL * n_out * b0 - (long long)n_out * f, D = 2LL * n_out * f; // |N| < 2^47
    const long long a = 256 * N;
    long long q = a / D;
    if (a % D != 0 && a < 0) q--; // floor, not truncation (D > 0)
    const long long top = 256LL * (n_lvl - 1);
    q = q < 0 ? 0 : (q > top ? top : q);
    ResizedTap t;
    t.i0 = (int)(q >> 8);
    t.i1 = t.i0 + 1 < n_lvl ? t.i0 + 1 : n_lvl - 1;
    t.t = (int)(q & 255);
    return t;
}
// The level rows (columns) lo .. lo + n - 1 that output rows (columns) ra .. rb read: the taps are monotone in r
struct ResizedSpan { int lo, n; };
LRF_HD inline ResizedSpan resized_span(int ra, int rb, int n_out, int b0, int nb, int f, int n_lvl)
{
    const int lo = resized_tap(ra, n_out, b0, nb, f, n_lvl).i0, hi = resized_tap(rb, n_out, b0, nb, f, n_lvl).i1;
    return ResizedSpan{lo, hi - lo + 1};
}
// Staged path: a workgroup owns LRF_RS_TH x LRF_RS_TW output pixels, a thread four adjacent pixels of a row, and decodes the
// level pixels its tile reads — at most LRF_RS_FH x LRF_RS_FW of them — into LDS first.  t consecutive outputs advance the tap
// by (t - 1) nb / (n_out f) level pixels, the floor adds less than one, and i1 one more: resized_span_bound >= every span.
#define LRF_RS_TH 16
#define LRF_RS_TW 64
#define LRF_RS_FH 44
#define LRF_RS_FW 192
LRF_HD inline long resized_span_bound(int tile, int n_out, int nb, int f)
{
    const int t = tile < n_out ? tile : n_out;
    return (long)(t - 1) * nb / ((long)n_out * f) + 3;
}
// whether the footprint of every tile of the box fits the LDS tile: else the direct path takes it (extreme aspect ratios, and
// boxes many times the output, which level 8 leaves more than twice the output's size)
LRF_HD inline bool resized_staged(int hb, int wb, int oh, int ow, int f)
{
    return resized_span_bound(LRF_RS_TH, oh, hb, f) <= LRF_RS_FH && resized_span_bound(LRF_RS_TW, ow, wb, f) <= LRF_RS_FW;
}
LRF_HD inline long resized_staged_wgs(int oh, int ow) { return (long)((oh + LRF_RS_TH - 1) / LRF_RS_TH) * ((ow + LRF_RS_TW - 1) / LRF_RS_TW); }
// output rows r0 .. r0 + nr - 1 and columns c0 .. c0 + nc - 1 of tile wg (before the flip: the columns the taps are defined for)
struct ResizedTile { int r0, nr, c0, nc; };
LRF_HD inline ResizedTile resized_tile_of(int oh, int ow, int wg)
{
    const int ntx = (ow + LRF_RS_TW - 1) / LRF_RS_TW, ty = wg / ntx, tx = wg - ty * ntx;
    ResizedTile t;
    t.r0 = ty * LRF_RS_TH;
    t.c0 = tx * LRF_RS_TW;
    t.nr = oh - t.r0 < LRF_RS_TH ? oh - t.r0 : LRF_RS_TH;
    t.nc = ow - t.c0 < LRF_RS_TW ? ow - t.c0 : LRF_RS_TW;
    return t;
}
// thread tid of the tile: row r, columns c .. c + n - 1 (n = 0: none); column s is written at resized_out_col(s, ow, flip)
struct ResizedPx { int r, c, n; };
LRF_HD inline ResizedPx resized_thread_of(const ResizedTile& t, int tid)
{
    const int tr = tid / (LRF_RS_TW / 4), tc = (tid - tr * (LRF_RS_TW / 4)) * 4;
    ResizedPx p = {t.r0 + tr, t.c0 + tc, 0};
    if (tr < t.nr && tc < t.nc) p.n = t.nc - tc < 4 ? t.nc - tc : 4;
    return p;
}
LRF_HD inline int resized_out_col(int s, int ow, int flip) { return flip ? ow - 1 - s : s; }
// Direct path: a thread one output pixel, row by row, 256 to a workgroup (scaled_pixel_of over (0, 0, oh, ow))
LRF_HD inline long resized_direct_wgs(int oh, int ow) { return scaled_any_wgs(oh, ow); }
// One launch: items item0 .. item0 + nitems - 1 of the sorted table, wgs workgroups each (grid.x = nitems * wgs)
struct ResizedLaunch {
    int direct, f, r8; // the path, the level, and whether every rank of the launch's images is <= 8 (the decode8 fill)
    long item0, nitems, wgs;
};
struct ResizedPlan {
    std::vector<ResizedLaunch> launches; // order: (path, level, rank class), staged first; at most LRF_RESIZED_MAX_LAUNCHES
    std::vector<ResizedItem> table;      // the boxes grouped by launch, call order inside a group; place = the place in the call
    long too_many = 0;                   // != 0: a launch would have this many (>= 2^31) workgroups; no table is built
};
#define LRF_RESIZED_MAX_LAUNCHES 16 // 2 paths x 4 levels x 2 rank classes
// r8: per image, whether its three ranks are all <= 8; crops: (image, y0, x0, hb, wb, flip) in call order, validated (f and
// place are set here)
ResizedPlan plan_decode_resized(const std::vector<int>& r8, const std::vector<ResizedItem>& crops, int oh, int ow);

// ---- the gray loader: the image list, the thread maps and the launches of lrf_qmf_decode_gray_ragged_u8, _crops_ and ---------
// _resized_crops_ (kernels: lrf_gray_loader_kernel.hip).  The kernels and tests/test_gray_loader_plan.py call the same functions.
// Level 1, the patch body (k_gray_decode's: a thread two rows of one 8x8 patch): the patches a window touches, row by row, 64 to
// a workgroup.  top, left: GrayDesc's; y0, x0, h, w: the window in image pixels.
LRF_HD inline long gray_tile_wgs(int top, int left, int y0, int x0, int h, int w)
{
    const long npr = ((y0 + h - 1 + top) >> 3) - ((y0 + top) >> 3) + 1, npc = ((x0 + w - 1 + left) >> 3) - ((x0 + left) >> 3) + 1;
    return (npr * npc + 63) / 64;
}
struct GrayTile {
    int pr, pc, ap; // padded rows 8 pr + 2 ap, + 1 of the patch (pr, pc)
    CropSpan px;    // what of them lies inside the window: ny == 0 or nx == 0: nothing
};
LRF_HD inline GrayTile gray_tile_of(int top, int left, int y0, int x0, int h, int w, long wg, int tid)
{
    const int pr0 = (y0 + top) >> 3, pc0 = (x0 + left) >> 3;
    const int npr = ((y0 + h - 1 + top) >> 3) - pr0 + 1, npc = ((x0 + w - 1 + left) >> 3) - pc0 + 1;
    // (an image has fewer than 2^31 / 64 patches, so 32-bit arithmetic: the kernels do this division once per thread)
    const unsigned o = (unsigned)wg * 64u + (unsigned)(tid >> 2);
    GrayTile t = {pr0, pc0, tid & 3, {y0, x0, 0, 0}};
    if (wg < 0 || wg >= gray_tile_wgs(top, left, y0, x0, h, w) || o >= (unsigned)npr * (unsigned)npc) return t;
    t.pr = pr0 + (int)(o / (unsigned)npc);
    t.pc = pc0 + (int)(o - (o / (unsigned)npc) * (unsigned)npc);
    const int ya = 8 * t.pr + 2 * t.ap - top, xa = 8 * t.pc - left;
    const int ylo = ya > y0 ? ya : y0, yhi = ya + 2 < y0 + h ? ya + 2 : y0 + h;
    const int xlo = xa > x0 ? xa : x0, xhi = xa + 8 < x0 + w ? xa + 8 : x0 + w;
    if (yhi > ylo && xhi > xlo) t.px = CropSpan{ylo, xlo, yhi - ylo, xhi - xlo};
    return t;
}
// Levels 2, 4, 8: the window's pixel quads, row by row, 256 to a workgroup (crop_quad_wgs, crop_quad_of above).
// The image list, checked and described as the kernels read it.  Checks per image, in this order: the size (sides in [1,2^20],
// fewer than 2^31 pixels), the reflect padding of lrf_chan_dims(H, W, 1, 8, 8), the rank 1..64, negative offsets, the U and the
// V extent against u_len / v_len, and — scale != 0 — out_off and the image's [Hs][Ws] at that level against out_len.  Every
// term is checked against the length before it is added to an offset: no sum can wrap.
enum { GDESC_OK = 0, GDESC_SIZE, GDESC_GEOM, GDESC_RANK, GDESC_NEGATIVE, GDESC_U, GDESC_V, GDESC_OUT };
struct GrayRefusal {
    int check = GDESC_OK;
    int64_t image = 0, a = 0, b = 0; // GDESC_SIZE, GDESC_GEOM: H, W; GDESC_RANK: the rank; GDESC_U, GDESC_V, GDESC_OUT: the buffer's length
};
// descs: n descriptors (no padding bytes: their bytes are the device table's key).  On a refusal they are left unspecified.
GrayRefusal describe_gray_images(int64_t n, const lrf_gray_image* images, int64_t u_len, int64_t v_len, int scale, int64_t out_len,
                                 std::vector<GrayDesc>& descs);
// One launch: items item0 .. item0 + nitems - 1 of the sorted table, wgs workgroups each (grid.x = nitems * wgs; wgs: the most
// an item of the launch needs, the workgroups an item does not need exit)
struct GrayLaunch {
    int f, direct; // the level; resized crops: the path (0: staged)
    long item0, nitems, wgs;
};
struct GrayPlan {
    std::vector<GrayLaunch> launches; // windows: by level, at most 4; resized crops: by (path, level), staged first, at most 8
    std::vector<GrayItem> table;      // the items grouped by launch, call order inside a group; place = the place in the call
    long too_many = 0;                // != 0: a launch would have this many (>= 2^31) workgroups; no table is built
};
// items: validated windows (image, f, y0, x0, h, w in level coordinates, out_off, pitch) in call order (place is set here)
GrayPlan plan_gray_windows(const std::vector<GrayDesc>& descs, const std::vector<GrayItem>& items);
// boxes: validated (image, y0, x0, h, w in full-resolution pixels, flip) in call order (f, place, out_off and pitch are set
// here: box j is [oh][ow] at oh ow j).  resized_level, resized_staged and the staged / direct thread maps are the colour entry's
GrayPlan plan_gray_resized(const std::vector<GrayItem>& boxes, int oh, int ow);

// ---- the window list of the ten entries that decode crops: checked, and handed on as the items the kernels read ----------------
// (lrf_qmf_decode_crops_, _scaled_crops_, _resized_crops_, _gray_crops_, _gray_resized_crops_, each _u8 and _tensor).  The kernels
// index with the items alone, so next to describe_images this is the one place between a caller's crop list and an
// out-of-bounds read.  tests/test_decode_windows_host.py calls it on the CPU.
enum { WIN_OK = 0, WIN_N_IMAGES, WIN_N_CROPS, WIN_SIZE, WIN_CAPACITY, WIN_IMAGE, WIN_SCALE, WIN_SIDES, WIN_BOX };
#define LRF_WIN_SCALES_COLOUR 0x114u // bit f: scale f is admitted — 2, 4, 8 ...
#define LRF_WIN_SCALES_GRAY 0x116u   // ... and 1, 2, 4, 8
#define LRF_WIN_MAX_CROPS (1 << 20)
#define LRF_WIN_MAX_RESIZED_SIDE 16384
struct WindowCall {
    int64_t n_images, n_crops;
    int64_t h, w;    // the size all windows share; resized: the output size (oh, ow) all boxes are resampled to
    bool resized;    // the crops are boxes with sides of their own (lrf_resized_crop)
    unsigned scales; // the admitted scales of lrf_scaled_crop (LRF_WIN_SCALES_*); 0: the crops carry none (lrf_crop, lrf_resized_crop)
    int channels;    // 3 or 1: crop j is [channels][h][w] at channels h w j
    int64_t out_len; // elements of the output
};
// the first offender: which check, and for the per-crop checks which crop, its fields and — WIN_BOX — its image's size at its scale
struct WindowRefusal {
    int check = WIN_OK;
    int64_t crop = 0;
    int image = 0, scale = 1, y0 = 0, x0 = 0;
    int64_t h = 0, w = 0, H = 0, W = 0;
};
// the ranges of the call alone, in this order: n_images in [1,65535], n_crops in [1,2^20], both sides >= 1 and <= INT32_MAX
// (resized: <= 16384)
WindowRefusal check_window_call(const WindowCall& k);
// k: accepted by check_window_call; descs: describe_images' or describe_gray_images' table of the k.n_images images.  First the
// output's capacity (k.channels k.h k.w k.n_crops elements), then per crop, in this order: the image index, the scale, box
// sides >= 1, the window inside its image at its scale (ceil(H / f) x ceil(W / f)).  Every comparison comes before the sum or
// product it guards: nothing wraps.  items: the n_crops items in call order as plan_decode_crops, plan_decode_scaled,
// plan_decode_resized, plan_gray_windows (lrf_scaled_crop) and plan_gray_resized (lrf_resized_crop) take them; on a refusal
// they are left unspecified.  Instantiated in lrf_plan.cpp for those five (Desc, Crop, Item).
template <class Desc, class Crop, class Item>
WindowRefusal check_windows(const WindowCall& k, const std::vector<Desc>& descs, const Crop* crops, std::vector<Item>& items);

// ---- inflate of factor columns: which lane decodes which column (lrf_inflate_columns_i8; tests/test_inflate_plan.py) ----------
// One lane per stream, 64 consecutive slots to a wave.  The slots are the matrices' columns, matrix after matrix, a matrix's
// columns ascending — so a wave's lanes hold adjacent columns of one matrix (adjacent bytes of every row) until the matrix
// ends — and the matrices by descending `rows`: the long U columns start first and share no wave with the 64-row V columns
// except where the two groups meet.  Ties: more columns first, then the order of the call.
struct InflateMatDim { long rows; int cols; };
struct InflateSlot { int mat, col; };
std::vector<InflateSlot> plan_inflate(const std::vector<InflateMatDim>& mats);

// ---- geometry of the default branch (lrf/compression/qmf.py:230-242): plain arithmetic, so it lives with the plans --------------
void plane_dims(int64_t H, int64_t W, int c, int64_t* h, int64_t* w, int64_t* hp, int64_t* wp, int64_t* M);
// 0, or the number (1..3) of the first plane the reference could not form — 10 + that number when its reflect padding would
// exceed the plane, else the plane is empty — with that plane's size in *bad_h / *bad_w (make_geom words the refusal)
int geom_of(int64_t H, int64_t W, ImageGeom* g, int64_t* bad_h, int64_t* bad_w);

// ---- encode: the tables of a ragged call (lrf_qmf_encode_ragged_rgb_u8) -------------------------------------------------------
// the planes body that serves an image: k_planes16's when both sides are multiples of 16 and its bytes start at a multiple of 8,
// else k_planes_strip<KH, KW>'s with window sizes 2 (even side) or 3 (odd side): ENC_STRIP22 + 2 (H & 1) + (W & 1)
enum { ENC_TILE16 = 0, ENC_STRIP22 = 1, ENC_STRIP23 = 2, ENC_STRIP32 = 3, ENC_STRIP33 = 4 };
#define LRF_ENC_BODIES 5
// One image as the entry point hands it over, every field validated there.  sign_off: -1 = the default signs
struct EncRaggedImage {
    long H, W;
    int R[3];
    long rgb_off, u_off, v_off, sign_off;
    bool aligned8; // rgb + rgb_off is a multiple of 8
};
struct EncRaggedLaunch {
    int body;
    long block0, nblocks; // its workgroups: entries block0 .. block0 + nblocks - 1 of the workgroup table
    int xcd_chunk;        // strip bodies: ceil(nblocks / 8), the grid is 8 * xcd_chunk (k_planes_strip_ragged); ENC_TILE16: 0
};
struct EncRaggedPlane { int image, ch; };
struct EncRaggedPlan {
    std::vector<EncRaggedDesc> descs;      // per image; x_off = the running sum of img_floats
    std::vector<EncRaggedLaunch> launches; // by body, ENC_TILE16 first: at most LRF_ENC_BODIES
    std::vector<RaggedBlock> blocks;       // per launch the images in call order, an image's units ascending
    Tables t;                              // the plane / block tables plan_bcd and run_init / run_bcd take
    std::vector<EncRaggedPlane> order;     // which (image, channel) plane i of the table is
    bool split = false;                    // plan_splits of the whole call: the table is ordered by kernel family
    long x_floats = 0;                     // the X workspace
    long too_many = 0;                     // != 0: the call has this many (>= 2^31) BCD blocks or planes workgroups; nothing is built
};
// Plane order: by kernel family when the call splits (plan_bcd then finds at most three runs), inside a family — or in the
// whole table of a call that does not split — luma before Cb before Cr, images in call order.  Every plane computes its own
// initialisation, so each run's leading planes are its self-initialising ones, as plan_bcd assumes.
EncRaggedPlan plan_encode_ragged(const std::vector<EncRaggedImage>& images, const PlanSettings& s);

// ---- encode: the tables of a ragged sweep (lrf_qmf_encode_ragged_sweep_rgb_u8): images of differing sizes, each at a list of
// candidate rank triples of its own.  One image as the entry point hands it over, every field validated there
struct EncSweepImage {
    long H, W;
    long rgb_off, sign_off; // sign_off: -1 = the default signs, else where its [Rmax_Y + Rmax_Cb + Rmax_Cr] signs start
    bool aligned8;          // rgb + rgb_off is a multiple of 8
};
struct EncSweepCand {
    int image;
    int R[3];
    long u_off, v_off;
};
struct EncSweepPlane { int cand, ch; };
struct EncRaggedSweepPlan {
    std::vector<EncRaggedDesc> descs;      // per image, launches and blocks of the planes stage: plan_encode_ragged's for the list
    std::vector<EncRaggedLaunch> launches;
    std::vector<RaggedBlock> blocks;
    Tables t;                              // one plane per (candidate, channel); init_src: the plane of the same image and channel
                                           // with the image's largest rank for that channel (the first of equal ranks)
    std::vector<EncSweepPlane> order;      // which (candidate, channel) plane i of the table is
    std::vector<int> rmax;                 // [3 n]: the largest rank per (image, channel) over the image's candidates
    bool split = false;                    // plan_splits of the whole call
    long x_floats = 0;                     // the X workspace: the sum over IMAGES
    long too_many = 0;                     // != 0: this many (>= 2^31) BCD blocks or planes workgroups; nothing is built
};
// Plane order, the uniform sweep's: by kernel family when the call splits, inside a family the self-initialising planes first,
// then luma before Cb before Cr, candidates in call order.  With one candidate per image, in image order, the table is
// plan_encode_ragged's.  Every image must have a candidate (the entry point checks).
EncRaggedSweepPlan plan_encode_ragged_sweep(const std::vector<EncSweepImage>& images, const std::vector<EncSweepCand>& cands, const PlanSettings& s);

// ---- encode: the tables of a ragged gray sweep (lrf_qmf_encode_gray_ragged_sweep_u8; the plain ragged gray encode is the sweep
// with one candidate per image).  A gray image is one matrix [M][64]: one plane per candidate.
// the planes body that serves an image: k_gray_planes16's when W % 16 == 0 and its bytes start at a multiple of 16, else
// k_gray_planes' (lrf_channels_kernel.hip)
enum { ENC_GRAY16 = 0, ENC_GRAY_ANY = 1 };
// The list as the caller hands it over, checked and described (describe_gray_encode).  Checks, in this order: n in [1,65535],
// m in [n,2^20]; per image: the size (sides in [1,2^20]), the reflect padding of lrf_chan_dims(H, W, 1, 8, 8), fewer than 2^31
// pixels, negative offsets, the pixels against gray_len; K, the bounds; per candidate: the image index, the rank (>= 1, then
// <= LRF_BIG_TO_ANY_RANK), negative offsets, the U and the V extent against u_len / v_len; per image: a candidate, its [Rmax]
// signs against sign_len; then overlapping U and V ranges.  Every term is checked against the length before it is added to an
// offset: no sum can wrap.
enum { GENC_OK = 0, GENC_N, GENC_M, GENC_SIZE, GENC_GEOM, GENC_PIXELS, GENC_NEGATIVE, GENC_GRAY, GENC_K, GENC_BOUNDS, GENC_IMAGE, GENC_RANK_LOW,
       GENC_RANK_BIG, GENC_U, GENC_V, GENC_NO_CAND, GENC_SIGN, GENC_OVERLAP_U, GENC_OVERLAP_V };
struct GrayEncRefusal {
    int check = GENC_OK;
    int candidate = 0;               // 1: `index` counts candidates, 0: images
    int64_t index = 0, a = 0, b = 0; // GENC_SIZE, GENC_GEOM: H, W; GENC_IMAGE, GENC_RANK_*: the value; GENC_GRAY, GENC_U, GENC_V, GENC_SIGN: the
                                     // buffer's length; GENC_OVERLAP_*: the element where two ranges meet
};
struct EncGrayImage {
    long H, W;
    long gray_off, sign_off; // sign_off: -1 = the default signs, else where its [Rmax] signs start
    bool aligned16;          // gray + gray_off is a multiple of 16
};
struct EncGrayCand {
    int image, R;
    long u_off, v_off;
};
struct GrayEncCall {
    int64_t gray_len, sign_len, u_len, v_len; // sign_len: 0 = no sign buffer (every sign_off counts as -1)
    uintptr_t gray_base;                      // the address of `gray`: decides aligned16
    int K, lo, hi;
};
// ims, cs: filled only when the whole list is accepted — a refused list builds nothing (both stay empty)
GrayEncRefusal describe_gray_encode(int64_t n, const lrf_gray_sweep_image* images, int64_t m, const lrf_gray_sweep_candidate* cands,
                                    const GrayEncCall& k, std::vector<EncGrayImage>& ims, std::vector<EncGrayCand>& cs);
struct EncGrayLaunch {
    int body;
    long block0, nblocks; // its workgroups: entries block0 .. block0 + nblocks - 1 of the workgroup table
};
struct EncGraySweepPlan {
    std::vector<EncGrayDesc> descs;      // per image; x_off = the running sum of 64 M
    std::vector<EncGrayLaunch> launches; // by body, ENC_GRAY16 first: at most two
    std::vector<RaggedBlock> blocks;     // per launch the images in call order, an image's groups of 256 items ascending
    Tables t;                            // one plane per candidate; init_src: the plane of the image's first candidate of largest rank
    std::vector<int> order;              // which candidate plane i of the table is
    std::vector<int> rmax;               // [n]: the largest rank over the image's candidates
    bool split = false;                  // plan_splits of the whole call: the table is ordered by kernel family
    long x_floats = 0;                   // the X workspace: the sum over IMAGES
    long too_many = 0;                   // != 0: this many (>= 2^31) BCD blocks or planes workgroups; nothing is built
};
// Plane order, plan_encode_ragged_sweep's: by kernel family when the call splits, inside a family — or in the whole table of a
// call that does not split — the self-initialising planes first, candidates in call order.  images, cands: describe_gray_encode's
EncGraySweepPlan plan_encode_gray_ragged_sweep(const std::vector<EncGrayImage>& images, const std::vector<EncGrayCand>& cands, const PlanSettings& s);

// ---- the any-shape path (lrf_anyshape_host.inc executes these; tests/test_any_plan.py reads them on the CPU) ----------------
#define LRF_ANY_GS_MAX_LDS (160 * 1024) // dynamic LDS of k_any_gs<float, .>
#define LRF_ANY_NATIVE_BELOW 400        // products of fewer multiply-adds take ATen's small-product order
#define LRF_ANY_INIT_WORK_BYTES ((size_t)2 << 30) // Gram matrices and eigen-solver work space of one chunk of any_run_init
// One product C [B][I][R] = A' Bm over a contraction of length D (any_prod).  THIN_LONG: k_any_prod_thin_long; THIN_SHORT4 /
// 8 / 16: k_any_prod_thin_short<4 | 8 | 16>; BIG: k_any_prod_big; TILED: k_any_prod
enum AnyProdKernel { ANY_PROD_THIN_LONG, ANY_PROD_THIN_SHORT4, ANY_PROD_THIN_SHORT8, ANY_PROD_THIN_SHORT16, ANY_PROD_BIG, ANY_PROD_TILED };
struct AnyProdPlan {
    AnyProdKernel k;
    int nblk;            // blocks of LRF_KC of the contraction; above one the kernel writes partial sums ...
    bool fold;           // ... and k_any_fold, grid (fold_gx, B) of 256 threads, adds them in block order
    int tpw, tiles;      // 16-row tiles per wave (THIN_SHORT*) / 64-row tiles per workgroup (TILED); 1 for the others
    unsigned gx, gy, gz; // the product kernel's grid ...
    int threads;         // ... and workgroup size
    unsigned fold_gx;
    bool native;         // TILED in ATen's order (the caller's flag, where the product stays on k_any_prod)
    bool refused;        // the contraction's blocks times the rank's column tiles exceed the launch grid: no launch
};
AnyProdPlan plan_any_prod(int I, int D, int R, int B, long sai, long sak, bool native, bool prod_small);
// The Gauss-Seidel sweep over the rows of a factor (any_update).  GS_I8: k_any_gs<int8_t, true>; GS_F32_LDS: k_any_gs<float, true>;
// GS_F32_NOLDS: k_any_gs<float, false> (the diagonal no longer fits next to the rows)
enum AnyGsKernel { ANY_GS_I8, ANY_GS_F32_LDS, ANY_GS_F32_NOLDS };
struct AnyGsPlan {
    AnyGsKernel k;
    unsigned gx, gy; // 64 threads
    size_t lds;
    int native_gs;   // (R - 1) rows < LRF_ANY_NATIVE_BELOW
};
AnyGsPlan plan_any_gs(int rows, int R, int B, bool int_rows, bool gs_f32);
// One factor update of B matrices [M][N] at rank R (any_update; trans: the V update): a = x @ v (or x.mT @ u), b = v.mT @ v, the sweep
struct AnyUpdatePlan { AnyProdPlan a, b; AnyGsPlan gs; };
AnyUpdatePlan plan_any_update(int B, int M, int N, int R, bool trans, bool int_rows, bool prod_small, bool gs_f32);
// matrices per chunk of any_run_init: n = min(M, N), Rc = min(R, n)
long plan_any_init_chunk(int n, int Rc, long B);
#endif
