// Test-only C entries to describe_gray_images, plan_gray_windows and plan_gray_resized (lrf_amd/csrc/lrf_plan.cpp) and to the
// functions of lrf_plan.h that say which pixels a thread of the gray loader's window kernels answers for, for
// tests/test_gray_loader_plan.py: built with the host compiler, no device.
#include <algorithm>

#include "../lrf_amd/csrc/lrf_plan.h"

// images: (H, W, R, u_off, v_off, out_off) per image.  Returns the check that refused (GDESC_*; 0: none) with the offender in
// *image; descs: (u_off, v_off, H, W, R, top, left, nw) per image when nothing is refused.
extern "C" int lrf_test_describe_gray(long n, const long* images, long u_len, long v_len, int scale, long out_len, long* image, long* descs)
{
    std::vector<lrf_gray_image> im((size_t)n);
    for (long i = 0; i < n; i++) {
        const long* e = images + 6 * i;
        im[(size_t)i] = lrf_gray_image{e[0], e[1], (int)e[2], e[3], e[4], e[5]};
    }
    std::vector<GrayDesc> d;
    const GrayRefusal r = describe_gray_images(n, im.data(), u_len, v_len, scale, out_len, d);
    *image = r.image;
    if (r.check != GDESC_OK) return r.check;
    for (long i = 0; i < n; i++) {
        const GrayDesc& g = d[(size_t)i];
        const long v[8] = {g.u_off, g.v_off, g.H, g.W, g.R, g.top, g.left, g.nw};
        for (int k = 0; k < 8; k++) descs[8 * i + k] = v[k];
    }
    return 0;
}

// Every window of size (h, w) of level f of an H x W image, at every origin: the pixels the threads of its workgroups keep
// (f = 1: gray_tile_of over gray_tile_wgs workgroups, as k_gray_window1 stores them; f = 2, 4, 8: crop_quad_of over crop_quad_wgs,
// as k_gray_windowf does) must be the window exactly.  Returns the number of origins checked, or -(1 + the index of the first
// origin, row-major, at which a pixel is kept twice, kept outside the window or not kept).
extern "C" long lrf_test_gray_window_cover(int H, int W, int f, int h, int w)
{
    const int Hs = (int)scaled_dim(H, f), Ws = (int)scaled_dim(W, f);
    const int top = ((8 - H % 8) % 8) / 2, left = ((8 - W % 8) % 8) / 2;
    if (h > Hs || w > Ws) return 0;
    std::vector<int> count((size_t)h * w);
    long origins = 0;
    for (int y0 = 0; y0 + h <= Hs; y0++)
        for (int x0 = 0; x0 + w <= Ws; x0++, origins++) {
            std::fill(count.begin(), count.end(), 0);
            bool bad = false;
            auto keep = [&](int y, int x) {
                if (y < y0 || y >= y0 + h || x < x0 || x >= x0 + w) bad = true;
                else count[(size_t)(y - y0) * w + (x - x0)]++;
            };
            const long wgs = f == 1 ? gray_tile_wgs(top, left, y0, x0, h, w) : crop_quad_wgs(h, w);
            for (long wg = 0; wg < wgs; wg++)
                for (int tid = 0; tid < 256; tid++) {
                    if (f == 1) {
                        const GrayTile t = gray_tile_of(top, left, y0, x0, h, w, wg, tid);
                        if (t.px.ny == 0 || t.px.nx == 0) continue;
                        // the rows and columns must be the thread's own: two rows of its patch
                        if (t.px.y < 8 * t.pr + 2 * t.ap - top || t.px.y + t.px.ny > 8 * t.pr + 2 * t.ap + 2 - top) bad = true;
                        if (t.px.x < 8 * t.pc - left || t.px.x + t.px.nx > 8 * t.pc + 8 - left) bad = true;
                        for (int y = t.px.y; y < t.px.y + t.px.ny; y++)
                            for (int x = t.px.x; x < t.px.x + t.px.nx; x++) keep(y, x);
                    } else {
                        const CropSpan q = crop_quad_of(y0, x0, h, w, (int)wg, tid);
                        for (int k = 0; k < q.nx * q.ny; k++) keep(q.y, q.x + k);
                    }
                }
            for (int c : count)
                if (c != 1) bad = true;
            if (bad) return -(1 + origins);
        }
    return origins;
}

static void put_plan(const GrayPlan& p, long* launches, long* table)
{
    for (size_t j = 0; j < p.launches.size(); j++) {
        const GrayLaunch& l = p.launches[j];
        const long v[5] = {l.f, l.direct, l.item0, l.nitems, l.wgs};
        for (int i = 0; i < 5; i++) launches[j * 5 + i] = v[i];
    }
    for (size_t j = 0; j < p.table.size(); j++) {
        const GrayItem& e = p.table[j];
        const long v[10] = {e.image, e.f, e.y0, e.x0, e.h, e.w, e.flip, e.place, e.out_off, e.pitch};
        for (int i = 0; i < 10; i++) table[j * 10 + i] = v[i];
    }
}

// sizes: (H, W) per image; items: (image, f, y0, x0, h, w, out_off, pitch) per window.  launches: (f, direct, item0, nitems, wgs)
// per launch, at most max_launches; table: (image, f, y0, x0, h, w, flip, place, out_off, pitch) per item.  Returns the number
// of launches, or -1 when they do not fit.
extern "C" int lrf_test_plan_gray_windows(int n_images, const long* sizes, long n_items, const long* items, long* launches, int max_launches, long* table,
                                          long* too_many)
{
    std::vector<GrayDesc> d((size_t)n_images);
    for (int i = 0; i < n_images; i++) {
        const int H = (int)sizes[2 * i], W = (int)sizes[2 * i + 1];
        d[(size_t)i] = GrayDesc{0, 0, H, W, 1, ((8 - H % 8) % 8) / 2, ((8 - W % 8) % 8) / 2, (W + 7) / 8};
    }
    std::vector<GrayItem> it((size_t)n_items);
    for (long j = 0; j < n_items; j++) {
        const long* e = items + 8 * j;
        it[(size_t)j] = GrayItem{(int)e[0], (int)e[1], (int)e[2], (int)e[3], (int)e[4], (int)e[5], 0, -1, e[6], e[7]};
    }
    const GrayPlan p = plan_gray_windows(d, it);
    *too_many = p.too_many;
    if ((int)p.launches.size() > max_launches) return -1;
    put_plan(p, launches, table);
    return (int)p.launches.size();
}

// boxes: (image, y0, x0, h, w, flip) per box
extern "C" int lrf_test_plan_gray_resized(long n_boxes, const long* boxes, int oh, int ow, long* launches, int max_launches, long* table, long* too_many)
{
    std::vector<GrayItem> it((size_t)n_boxes);
    for (long j = 0; j < n_boxes; j++) {
        const long* e = boxes + 6 * j;
        it[(size_t)j] = GrayItem{(int)e[0], -1, (int)e[1], (int)e[2], (int)e[3], (int)e[4], (int)e[5], -1, -1, -1};
    }
    const GrayPlan p = plan_gray_resized(it, oh, ow);
    *too_many = p.too_many;
    if ((int)p.launches.size() > max_launches) return -1;
    put_plan(p, launches, table);
    return (int)p.launches.size();
}

extern "C" long lrf_test_gray_window_wgs(int H, int W, int f, int y0, int x0, int h, int w)
{
    return f == 1 ? gray_tile_wgs(((8 - H % 8) % 8) / 2, ((8 - W % 8) % 8) / 2, y0, x0, h, w) : crop_quad_wgs(h, w);
}
