// Test-only C entry to check_window_call and check_windows (lrf_amd/csrc/lrf_plan.cpp) for tests/test_decode_windows_host.py: built
// with the host compiler, no device.
#include <string.h>

#include "../lrf_amd/csrc/lrf_plan.h"

namespace {
// an item of any of the four types as (image, f, y0, x0, h, w, flip, place, out_off, pitch); -1: the type has no such field
void put(long* o, const CropEntry& e) { const long v[10] = {e.image, -1, e.y0, e.x0, -1, -1, -1, e.out, -1, -1}; memcpy(o, v, sizeof v); }
void put(long* o, const ScaledItem& e) { const long v[10] = {e.image, e.f, e.y0, e.x0, e.h, e.w, -1, e.place, e.out_off, e.pool_off}; memcpy(o, v, sizeof v); }
void put(long* o, const ResizedItem& e) { const long v[10] = {e.image, e.f, e.y0, e.x0, e.hb, e.wb, e.flip, e.place, -1, -1}; memcpy(o, v, sizeof v); }
void put(long* o, const GrayItem& e) { const long v[10] = {e.image, e.f, e.y0, e.x0, e.h, e.w, e.flip, e.place, e.out_off, e.pitch}; memcpy(o, v, sizeof v); }

template <class Desc, class Crop, class Item>
WindowRefusal run(const WindowCall& k, const long* sizes, const void* crops, long* items)
{
    std::vector<Desc> descs((size_t)k.n_images);
    memset((void*)descs.data(), 0, descs.size() * sizeof(Desc));
    for (int64_t i = 0; i < k.n_images; i++) { // (the check reads H and W of a descriptor, nothing else)
        descs[(size_t)i].H = (int)sizes[2 * i];
        descs[(size_t)i].W = (int)sizes[2 * i + 1];
    }
    std::vector<Item> list;
    const WindowRefusal r = check_windows(k, descs, (const Crop*)crops, list);
    if (r.check != WIN_OK) return r;
    if ((int64_t)list.size() != k.n_crops) return WindowRefusal{-1};
    for (int64_t j = 0; items && j < k.n_crops; j++) put(items + 10 * j, list[(size_t)j]);
    return r;
}
}

// As a crop entry runs them: check_window_call, then check_windows.  shape: 0 lrf_crop, 1 lrf_scaled_crop, 2 lrf_resized_crop;
// gray: the gray loader's descriptors and items; sizes: [n_images][2] (H, W).  refusal: (check, crop, image, scale, y0, x0, h, w,
// H, W); items: null, or room for ten numbers per crop (put above), written when the list is accepted.  Returns the check.
extern "C" int lrf_test_check_windows(int shape, int gray, long n_images, const long* sizes, long n_crops, const void* crops, long h, long w,
                                      unsigned scales, int channels, long out_len, long* refusal, long* items)
{
    const WindowCall k = {n_images, n_crops, h, w, shape == 2, scales, channels, out_len};
    WindowRefusal r = check_window_call(k);
    if (r.check == WIN_OK) {
        if (!gray && shape == 0) r = run<RaggedDesc, lrf_crop, CropEntry>(k, sizes, crops, items);
        else if (!gray && shape == 1) r = run<RaggedDesc, lrf_scaled_crop, ScaledItem>(k, sizes, crops, items);
        else if (!gray) r = run<RaggedDesc, lrf_resized_crop, ResizedItem>(k, sizes, crops, items);
        else if (shape == 1) r = run<GrayDesc, lrf_scaled_crop, GrayItem>(k, sizes, crops, items);
        else r = run<GrayDesc, lrf_resized_crop, GrayItem>(k, sizes, crops, items);
    }
    const long v[10] = {r.check, (long)r.crop, r.image, r.scale, r.y0, r.x0, (long)r.h, (long)r.w, (long)r.H, (long)r.W};
    memcpy(refusal, v, sizeof v);
    return r.check;
}
