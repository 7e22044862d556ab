// Test-only C entry to plan_inflate (lrf_amd/csrc/lrf_plan.cpp) for tests/test_inflate_plan.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

// rows / cols: one entry per matrix.  slots: (matrix, column) per slot, `max_slots` pairs of room.  Returns the number of slots, or -1.
extern "C" long lrf_test_plan_inflate(int n, const long* rows, const int* cols, int* slots, long max_slots)
{
    std::vector<InflateMatDim> m((size_t)n);
    for (int i = 0; i < n; i++) m[(size_t)i] = InflateMatDim{rows[i], cols[i]};
    const std::vector<InflateSlot> s = plan_inflate(m);
    if ((long)s.size() > max_slots) return -1;
    for (size_t k = 0; k < s.size(); k++) {
        slots[2 * k] = s[k].mat;
        slots[2 * k + 1] = s[k].col;
    }
    return (long)s.size();
}
