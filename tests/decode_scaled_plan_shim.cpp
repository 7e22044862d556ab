// Test-only C entries to plan_decode_scaled (lrf_amd/csrc/lrf_plan.cpp) and to the functions of lrf_plan.h that say which image
// pixels an output pixel of a scaled decode covers and which output pixels a thread answers for, for
// tests/test_decode_scaled_plan.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

extern "C" int lrf_test_scaled_f_ok(int f) { return scaled_f_ok(f) ? 1 : 0; }
extern "C" long lrf_test_scaled_dim(long n, int f) { return scaled_dim(n, f); }

// Output index i of a side of n image pixels at scale f, the chroma plane having nc: span = (lo, hi) of the image rows it
// covers; rows / mult: its chroma rows and how many of the covered image rows lie over each, in order (at most 8).  Returns
// the number of runs.
extern "C" int lrf_test_scaled_footprint(int i, int f, int n, int nc, int* span, int* rows, int* mult)
{
    span[0] = scaled_lo(i, f);
    span[1] = scaled_hi(i, f, n);
    int k = 0;
    for (int y = span[0]; y < span[1];) {
        int q;
        const int m = scaled_chroma_run(y, span[1], n, nc, &q);
        if (k < 8) {
            rows[k] = q;
            mult[k] = m;
        }
        k++;
        y += m;
    }
    return k;
}

extern "C" long lrf_test_scaled_wgs(int tiled, int f, int y0, int x0, int h, int w) { return tiled ? scaled_tiled_wgs(f, y0, x0, h, w) : scaled_any_wgs(h, w); }

// Adds one to count[y * Ws + x] for every output pixel the threads of the `wgs` workgroups of one window keep (Hs x Ws: the
// scaled image).  Returns the number of pixels outside the scaled image, or of tiled threads whose pixels are not those of
// their chroma patch: 0 when all is well.
extern "C" long lrf_test_scaled_cover(int tiled, int f, int Hs, int Ws, int y0, int x0, int h, int w, long wgs, int* count)
{
    long bad = 0;
    const int nc = 16 / f;
    for (long wg = 0; wg < wgs; wg++)
        for (int tid = 0; tid < 256; tid++) {
            CropSpan s;
            if (tiled) {
                const ScaledTile t = scaled_tile_of(f, y0, x0, h, w, wg, tid);
                s = t.px;
                if (s.ny > 0 && s.nx > 0) {
                    if (s.y < t.pr * nc || s.y + s.ny > t.pr * nc + nc) bad++;
                    if (s.x < t.pc * nc || s.x + s.nx > t.pc * nc + nc) bad++;
                }
                if (t.pr < 0 || t.pc < 0 || t.pr * nc >= Hs || t.pc * nc >= Ws) bad++; // (the u rows a dead thread loads exist too)
            } else
                s = scaled_pixel_of(y0, x0, h, w, wg, tid);
            if (s.ny <= 0 || s.nx <= 0) continue;
            for (int y = s.y; y < s.y + s.ny; y++)
                for (int x = s.x; x < s.x + s.nx; x++) {
                    if (y < 0 || y >= Hs || x < 0 || x >= Ws) bad++;
                    else count[(long)y * Ws + x]++;
                }
        }
    return bad;
}

enum { LAUNCH_INTS = 6, ITEM_INTS = 9, JOB_INTS = 3 };

// images: (tiled, cls, R_Y, R_Cb, R_Cr) per image; items: (image, f, y0, x0, h, w) per item.  launches: (tiled, f, cls, item0,
// nitems, wgs) per launch, at most max_launches; table: (image, f, y0, x0, h, w, place, out_off, pool_off) per item, out_off
// being the item's place times 1000 on the way in; jobs: (image, f, pool_off), at most max_jobs.  Returns the number of
// launches, or -1 when launches or jobs do not fit.
extern "C" int lrf_test_plan_decode_scaled(int n_images, const int* images, long n_items, const int* items, long* launches, int max_launches, long* table,
                                           long* jobs, long max_jobs, long* n_jobs, long* pool_elems, long* too_many)
{
    std::vector<ScaledImage> im((size_t)n_images);
    for (int i = 0; i < n_images; i++) im[(size_t)i] = ScaledImage{images[5 * i], images[5 * i + 1], {images[5 * i + 2], images[5 * i + 3], images[5 * i + 4]}};
    std::vector<ScaledItem> it((size_t)n_items);
    for (long j = 0; j < n_items; j++) {
        const int* e = items + 6 * j;
        it[(size_t)j] = ScaledItem{e[0], e[1], e[2], e[3], e[4], e[5], -1, -1, 1000 * j, -1};
    }
    const ScaledPlan p = plan_decode_scaled(im, it);
    *too_many = p.too_many;
    *pool_elems = p.pool_elems;
    *n_jobs = (long)p.jobs.size();
    if ((int)p.launches.size() > max_launches || (long)p.jobs.size() > max_jobs) return -1;
    for (size_t j = 0; j < p.launches.size(); j++) {
        const ScaledLaunch& l = p.launches[j];
        const long v[LAUNCH_INTS] = {l.tiled, l.f, l.cls, l.item0, l.nitems, l.wgs};
        for (int i = 0; i < LAUNCH_INTS; i++) launches[j * LAUNCH_INTS + i] = v[i];
    }
    for (size_t j = 0; j < p.table.size(); j++) {
        const ScaledItem& e = p.table[j];
        const long v[ITEM_INTS] = {e.image, e.f, e.y0, e.x0, e.h, e.w, e.place, e.out_off, e.pool_off};
        for (int i = 0; i < ITEM_INTS; i++) table[j * ITEM_INTS + i] = v[i];
    }
    for (size_t j = 0; j < p.jobs.size(); j++) {
        jobs[j * JOB_INTS] = p.jobs[j].image;
        jobs[j * JOB_INTS + 1] = p.jobs[j].f;
        jobs[j * JOB_INTS + 2] = p.jobs[j].pool_off;
    }
    return (int)p.launches.size();
}
