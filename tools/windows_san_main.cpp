// The window check of the entries that decode crops (check_window_call, check_windows: lrf_amd/csrc/lrf_plan.cpp) under ASan and
// UBSan, as a program of its own — nothing is loaded into Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o windows_san tools/windows_san_main.cpp
//       tests/decode_windows_host_shim.cpp lrf_amd/csrc/lrf_plan.cpp && ./windows_san
// Every crop shape and both scale sets: each field of a crop at every extreme of int32 (alone and all at once) against exactly
// sized tables, sizes and output lengths at the extremes of int64, and a list of 2^20 crops accepted, refused for one element
// of output, and refused at its last crop.  tests/test_decode_windows_host.py builds and runs it.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "../lrf_amd/csrc/lrf_plan.h"

extern "C" int lrf_test_check_windows(int shape, int gray, long n_images, const long* sizes, long n_crops, const void* crops, long h, long w,
                                      unsigned scales, int channels, long out_len, long* refusal, long* items);

static int failures = 0;
static void expect(int got, int want, const char* what, int kind, long a, long b)
{
    if (got == want) return;
    failures++;
    printf("kind %d: %s (%ld, %ld): check %d, expected %d\n", kind, what, a, b, got, want);
}

int main()
{
    struct Kind { int shape, gray; unsigned scales; int channels, cols; };
    const Kind kinds[5] = {{0, 0, 0, 3, 3}, {1, 0, LRF_WIN_SCALES_COLOUR, 3, 4}, {2, 0, 0, 3, 6}, {1, 1, LRF_WIN_SCALES_GRAY, 1, 4}, {2, 1, 0, 1, 6}};
    const long sizes[6] = {24, 48, 45, 61, 16, 16}; // (the calls name the first two; n_images = 3 below the third)
    const int extremes[9] = {INT_MIN, INT_MIN + 1, -1, 0, 1, 2, 3, INT_MAX - 1, INT_MAX};
    long refusal[10], calls = 0;
    for (int ki = 0; ki < 5; ki++) {
        const Kind& k = kinds[ki];
        const int f = k.shape == 1 ? 2 : 1;
        // a good crop: (image 1, [scale f,] y0 3, x0 5[, h 8, w 12, flip 1]), the call's windows 8 x 12
        std::vector<int> good = k.shape == 0 ? std::vector<int>{1, 3, 5} : k.shape == 1 ? std::vector<int>{1, f, 3, 5} : std::vector<int>{1, 3, 5, 8, 12, 1};
        std::vector<long> item(10);
        expect(lrf_test_check_windows(k.shape, k.gray, 2, sizes, 1, good.data(), 8, 12, k.scales, k.channels, k.channels * 96L, refusal, item.data()), WIN_OK,
               "the good crop", ki, 0, 0);
        // one field at an extreme, then every field
        for (int col = 0; col <= k.cols; col++)
            for (int e = 0; e < 9; e++) {
                std::vector<int> list(3 * (size_t)k.cols); // exactly three crops: reading a fourth is an error ASan reports
                for (int j = 0; j < 3; j++)
                    for (int c = 0; c < k.cols; c++) list[(size_t)(j * k.cols + c)] = j == 1 && (c == col || col == k.cols) ? extremes[e] : good[(size_t)c];
                std::vector<long> items(30);
                const int rc = lrf_test_check_windows(k.shape, k.gray, 2, sizes, 3, list.data(), 8, 12, k.scales, k.channels, k.channels * 288L, refusal, items.data());
                calls++;
                if (rc != WIN_OK && (rc < WIN_IMAGE || rc > WIN_BOX || refusal[1] != 1)) expect(rc, WIN_BOX, "a crop refusal at crop 1", ki, col, extremes[e]);
                if (col == k.cols && extremes[e] != 0 && extremes[e] != 1) expect(rc != WIN_OK, 1, "every field at an extreme", ki, col, extremes[e]);
            }
        // the call's numbers at the extremes of int64, the list never read beyond its one crop
        const long far[8] = {LONG_MIN, -1, 0, 1, 3, 16385, (long)INT_MAX + 1, LONG_MAX};
        for (int a = 0; a < 8; a++)
            for (int b = 0; b < 8; b++)
                for (int c = 0; c < 8; c++) {
                    lrf_test_check_windows(k.shape, k.gray, 2, sizes, 1, good.data(), far[a], far[b], k.scales, k.channels, far[c], refusal, nullptr);
                    calls++;
                }
        const long bad_n[6] = {LONG_MIN, -1, 0, LRF_WIN_MAX_CROPS + 1, (long)INT_MAX + 1, LONG_MAX}; // (65536 images are too many as well)
        for (int a = 0; a < 6; a++) {
            expect(lrf_test_check_windows(k.shape, k.gray, bad_n[a], sizes, 1, good.data(), 8, 12, k.scales, k.channels, LONG_MAX, refusal, nullptr), WIN_N_IMAGES,
                   "n_images", ki, bad_n[a], 0);
            expect(lrf_test_check_windows(k.shape, k.gray, 2, sizes, bad_n[a], good.data(), 8, 12, k.scales, k.channels, LONG_MAX, refusal, nullptr), WIN_N_CROPS,
                   "n_crops", ki, bad_n[a], 0);
        }
        expect(lrf_test_check_windows(k.shape, k.gray, 1, sizes, 1, good.data(), 8, 12, k.scales, k.channels, LONG_MAX, refusal, nullptr), WIN_IMAGE, "one image", ki, 0, 0);
        expect(lrf_test_check_windows(k.shape, k.gray, 3, sizes, 1, good.data(), 8, 12, k.scales, k.channels, LONG_MAX, refusal, nullptr), WIN_OK, "three images", ki, 0, 0);
        calls += 14;
        // 2^20 crops
        const long n = LRF_WIN_MAX_CROPS, fit = k.channels * 8L * 12L * n;
        std::vector<int> list((size_t)(n * k.cols));
        for (long j = 0; j < n; j++)
            for (int c = 0; c < k.cols; c++) list[(size_t)(j * k.cols + c)] = good[(size_t)c];
        std::vector<long> items((size_t)(10 * n));
        expect(lrf_test_check_windows(k.shape, k.gray, 2, sizes, n, list.data(), 8, 12, k.scales, k.channels, LONG_MAX, refusal, items.data()), WIN_OK,
               "2^20 crops into INT64_MAX elements", ki, 0, 0);
        expect(lrf_test_check_windows(k.shape, k.gray, 2, sizes, n, list.data(), 8, 12, k.scales, k.channels, fit, refusal, items.data()), WIN_OK,
               "2^20 crops into the exact fit", ki, 0, 0);
        expect((int)items[(size_t)(10 * (n - 1) + 7)], (int)(n - 1), "the last item's place", ki, 0, 0);
        expect(lrf_test_check_windows(k.shape, k.gray, 2, sizes, n, list.data(), 8, 12, k.scales, k.channels, fit - 1, refusal, nullptr), WIN_CAPACITY,
               "2^20 crops, one element short", ki, 0, 0);
        list[(size_t)((n - 1) * k.cols)] = 2;
        expect(lrf_test_check_windows(k.shape, k.gray, 2, sizes, n, list.data(), 8, 12, k.scales, k.channels, fit, refusal, nullptr), WIN_IMAGE,
               "2^20 crops, the last one bad", ki, 0, 0);
        expect((int)refusal[1], (int)(n - 1), "... named", ki, 0, 0);
        calls += 5;
    }
    printf("%ld calls, %d failures\n", calls, failures);
    return failures != 0;
}
