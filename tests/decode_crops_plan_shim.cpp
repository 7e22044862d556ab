// Test-only C entries to plan_decode_crops (lrf_amd/csrc/lrf_plan.cpp) and to the functions of lrf_plan.h that say which pixels a
// thread of a crop kernel answers for, for tests/test_decode_crops_plan.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

enum { LAUNCH_INTS = 5 };

// kind / cls: one entry per image; crops: (image, y0, x0) per crop.  launches: (kind, cls, crop0, ncrops, wgs) per launch, at
// most max_launches; table: (image, y0, x0, out) per crop.  Returns the number of launches, or -1 when they do not fit.
extern "C" int lrf_test_plan_decode_crops(int n_images, const int* kind, const int* cls, long n_crops, const int* crops, int h, int w, long* launches,
                                          int max_launches, int* table, long* too_many)
{
    std::vector<RaggedWork> im((size_t)n_images);
    for (int i = 0; i < n_images; i++) im[(size_t)i] = RaggedWork{kind[i], cls[i], 0};
    std::vector<CropEntry> cr((size_t)n_crops);
    for (long j = 0; j < n_crops; j++) cr[(size_t)j] = CropEntry{crops[3 * j], crops[3 * j + 1], crops[3 * j + 2], (int)j};
    const CropPlan p = plan_decode_crops(im, cr, h, w);
    *too_many = p.too_many;
    if ((int)p.launches.size() > max_launches) return -1;
    for (size_t j = 0; j < p.launches.size(); j++) {
        const CropLaunch& l = p.launches[j];
        const long v[LAUNCH_INTS] = {l.kind, l.cls, l.crop0, l.ncrops, l.wgs};
        for (int i = 0; i < LAUNCH_INTS; i++) launches[j * LAUNCH_INTS + i] = v[i];
    }
    for (size_t j = 0; j < p.table.size(); j++) {
        table[4 * j] = p.table[j].image;
        table[4 * j + 1] = p.table[j].y0;
        table[4 * j + 2] = p.table[j].x0;
        table[4 * j + 3] = p.table[j].out;
    }
    return (int)p.launches.size();
}

extern "C" long lrf_test_crop_wgs(int tiled, int h, int w) { return tiled ? crop_tiled_wgs(h, w) : crop_quad_wgs(h, w); }

// Adds one to count[y * W + x] for every pixel the threads of the `wgs` workgroups of one window keep (the H x W image's luma
// padding: top, left).  Returns the number of pixels outside the image, of spans kept by a workgroup crop_tile_wg_live calls
// dead, or of tiled threads whose rows / columns are not those of their (strip, ww, rp): 0 when all is well.
extern "C" long lrf_test_crop_cover(int tiled, int H, int W, int top, int left, int y0, int x0, int h, int w, long wgs, int* count)
{
    long bad = 0;
    for (long wg = 0; wg < wgs; wg++)
        for (int tid = 0; tid < 256; tid++) {
            CropSpan s;
            if (tiled) {
                const CropTile t = crop_tile_of(top, left, y0, x0, h, w, (int)wg, tid);
                s = t.px;
                if (s.ny > 0 && s.nx > 0) {
                    if (!crop_tile_wg_live(top, left, y0, x0, h, w, (int)wg)) bad++;
                    // the span lies in the thread's two padded rows and eight padded columns
                    if (s.y + top < 16 * t.strip + 2 * t.rp || s.y + s.ny + top > 16 * t.strip + 2 * t.rp + 2) bad++;
                    if (s.x + left < 8 * t.ww || s.x + s.nx + left > 8 * t.ww + 8) bad++;
                }
            } else
                s = crop_quad_of(y0, x0, h, w, (int)wg, tid);
            if (s.ny <= 0 || s.nx <= 0) continue;
            for (int y = s.y; y < s.y + s.ny; y++)
                for (int x = s.x; x < s.x + s.nx; x++) {
                    if (y < 0 || y >= H || x < 0 || x >= W) bad++;
                    else count[(long)y * W + x]++;
                }
        }
    return bad;
}
