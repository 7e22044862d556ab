// Test-only C entries to plan_decode_resized (lrf_amd/csrc/lrf_plan.cpp) and to the functions of lrf_plan.h that say which level
// a box is sampled from, which level pixels an output pixel reads and which output pixels a thread answers for, for
// tests/test_decode_resized_plan.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

extern "C" int lrf_test_resized_level(int hb, int wb, int oh, int ow) { return resized_level(hb, wb, oh, ow); }
extern "C" void lrf_test_resized_tap(int r, int n_out, int b0, int nb, int f, int n_lvl, int* out)
{
    const ResizedTap t = resized_tap(r, n_out, b0, nb, f, n_lvl);
    out[0] = t.i0; out[1] = t.i1; out[2] = t.t;
}
extern "C" int lrf_test_resized_staged(int hb, int wb, int oh, int ow, int f) { return resized_staged(hb, wb, oh, ow, f) ? 1 : 0; }
extern "C" long lrf_test_resized_span_bound(int tile, int n_out, int nb, int f) { return resized_span_bound(tile, n_out, nb, f); }
extern "C" long lrf_test_resized_wgs(int direct, int oh, int ow) { return direct ? resized_direct_wgs(oh, ow) : resized_staged_wgs(oh, ow); }
// the LDS tile and the output tile of the staged path: (FH, FW, TH, TW)
extern "C" void lrf_test_resized_tile_dims(int* out) { out[0] = LRF_RS_FH; out[1] = LRF_RS_FW; out[2] = LRF_RS_TH; out[3] = LRF_RS_TW; }

// Adds one to count[y * ow + x] for every output pixel (at the place it is written: after the flip) the threads of the `wgs`
// workgroups of one box keep.  Returns the number of pixels outside the output, or outside their workgroup's tile: 0 when all is well.
extern "C" long lrf_test_resized_cover(int direct, int oh, int ow, int flip, long wgs, int* count)
{
    long bad = 0;
    for (long wg = 0; wg < wgs; wg++)
        for (int tid = 0; tid < 256; tid++) {
            if (direct) {
                const CropSpan s = scaled_pixel_of(0, 0, oh, ow, wg, tid);
                if (s.ny == 0) continue;
                const int x = resized_out_col(s.x, ow, flip);
                if (s.y < 0 || s.y >= oh || x < 0 || x >= ow) bad++;
                else count[(long)s.y * ow + x]++;
            } else {
                const ResizedTile t = resized_tile_of(oh, ow, (int)wg);
                const ResizedPx p = resized_thread_of(t, tid);
                for (int j = 0; j < p.n; j++) {
                    const int x = resized_out_col(p.c + j, ow, flip);
                    if (p.r < t.r0 || p.r >= t.r0 + t.nr || p.c + j < t.c0 || p.c + j >= t.c0 + t.nc) bad++;
                    if (p.r < 0 || p.r >= oh || x < 0 || x >= ow) bad++;
                    else count[(long)p.r * ow + x]++;
                }
            }
        }
    return bad;
}

// The footprint of every tile of a box (y0, x0, hb, wb) of an H x W image at its level: returns the number of output pixels one
// of whose taps lies outside its tile's footprint (resized_span over the tile's rows and columns), and in *max_h / *max_w the
// largest footprint met.
extern "C" long lrf_test_resized_footprint(int H, int W, int y0, int x0, int hb, int wb, int oh, int ow, int* max_h, int* max_w)
{
    const int f = resized_level(hb, wb, oh, ow);
    const int Hs = (int)scaled_dim(H, f == 1 ? 1 : f), Ws = (int)scaled_dim(W, f == 1 ? 1 : f);
    long bad = 0;
    *max_h = *max_w = 0;
    for (long wg = 0; wg < resized_staged_wgs(oh, ow); wg++) {
        const ResizedTile t = resized_tile_of(oh, ow, (int)wg);
        const ResizedSpan sy = resized_span(t.r0, t.r0 + t.nr - 1, oh, y0, hb, f, Hs), sx = resized_span(t.c0, t.c0 + t.nc - 1, ow, x0, wb, f, Ws);
        if (sy.n > *max_h) *max_h = sy.n;
        if (sx.n > *max_w) *max_w = sx.n;
        if (sy.lo < 0 || sy.lo + sy.n > Hs || sx.lo < 0 || sx.lo + sx.n > Ws) bad++;
        for (int r = t.r0; r < t.r0 + t.nr; r++) {
            const ResizedTap a = resized_tap(r, oh, y0, hb, f, Hs);
            if (a.i0 < sy.lo || a.i1 >= sy.lo + sy.n) bad++;
        }
        for (int c = t.c0; c < t.c0 + t.nc; c++) {
            const ResizedTap a = resized_tap(c, ow, x0, wb, f, Ws);
            if (a.i0 < sx.lo || a.i1 >= sx.lo + sx.n) bad++;
        }
    }
    return bad;
}

enum { RS_LAUNCH_INTS = 6, RS_ITEM_INTS = 8 };

// r8: per image; crops: (image, y0, x0, hb, wb, flip) per box.  launches: (direct, f, r8, item0, nitems, wgs) per launch, at most
// max_launches; table: (image, f, y0, x0, hb, wb, flip, place) per box.  Returns the number of launches, or -1 when they do not fit.
extern "C" int lrf_test_plan_decode_resized(int n_images, const int* r8, long n_crops, const int* crops, int oh, int ow, long* launches, int max_launches,
                                            long* table, long* too_many)
{
    std::vector<int> im(r8, r8 + n_images);
    std::vector<ResizedItem> it((size_t)n_crops);
    for (long j = 0; j < n_crops; j++) {
        const int* e = crops + 6 * j;
        it[(size_t)j] = ResizedItem{e[0], -1, e[1], e[2], e[3], e[4], e[5], -1};
    }
    const ResizedPlan p = plan_decode_resized(im, it, oh, ow);
    *too_many = p.too_many;
    if ((int)p.launches.size() > max_launches) return -1;
    for (size_t j = 0; j < p.launches.size(); j++) {
        const ResizedLaunch& l = p.launches[j];
        const long v[RS_LAUNCH_INTS] = {l.direct, l.f, l.r8, l.item0, l.nitems, l.wgs};
        for (int i = 0; i < RS_LAUNCH_INTS; i++) launches[j * RS_LAUNCH_INTS + i] = v[i];
    }
    for (size_t j = 0; j < p.table.size(); j++) {
        const ResizedItem& e = p.table[j];
        const long v[RS_ITEM_INTS] = {e.image, e.f, e.y0, e.x0, e.hb, e.wb, e.flip, e.place};
        for (int i = 0; i < RS_ITEM_INTS; i++) table[j * RS_ITEM_INTS + i] = v[i];
    }
    return (int)p.launches.size();
}
