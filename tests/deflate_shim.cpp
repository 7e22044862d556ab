// Test-only C entry to the shared definition of the deflate coder (lrf_amd/csrc/lrf_deflate_shared.h) for
// tests/test_deflate_host.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_deflate_shared.h"

extern "C" {

int shim_tile(void) { return LRFD_T; }

// code lengths of n <= 512 symbols with counts freq[] under `limit` bits
int shim_code_lengths(const uint32_t* freq, int n, int limit, uint8_t* len)
{
    uint16_t sym[512];
    uint32_t w[512];
    if (n < 1 || n > 512 || limit < 1 || limit > 15) return -1;
    lrfd_code_lengths(freq, n, limit, len, sym, w);
    return 0;
}
}
