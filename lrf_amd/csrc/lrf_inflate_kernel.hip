// lrf_inflate_kernel.hip — k_inflate_columns: one LANE owns one zlib stream from its header to its Adler-32 and runs the serial
// decoder of lrf_inflate_shared.h on it; a workgroup is one wave, its 64 lanes the 64 consecutive slots plan_inflate gave it
// (adjacent columns of one matrix wherever possible).  The lanes share nothing: no barrier (they diverge from the first code
// on), no atomics, no hand-off.
//   tables  each lane's LRFI_TAB_N 16-bit entries in LDS, entry i of lane l at [i * 64 + l]: whatever entries the lanes of a wave
//           ask for, lane l's lie in bank (l / 2) mod 32 of its own — two lanes to a bank, the two halves of one dword when
//           both are at the same entry.  64 * 480 * 2 = 61,440 bytes per wave: two waves per CU.
//   input   byte loads from the lane's own stream into a 64-bit bit buffer
//   output  byte stores to dst[i * stride]: adjacent columns at the same row are adjacent bytes.  A match reads the lane's own
//           earlier stores back from global memory (program order of one lane; nobody else writes the column).
#define INF_LANES 64

struct InflateCol { // one slot of the launch, in plan_inflate's order
    int64_t src_off, dst_off; // the stream's first byte; the column's first element
    int32_t src_len, rows, stride, k; // k: the stream's index (its entry of `status`)
};
static_assert(sizeof(InflateCol) == 32, "the column table is copied as bytes");

__global__ __launch_bounds__(INF_LANES) void k_inflate_columns(const uint8_t* __restrict__ src, const InflateCol* __restrict__ cols, int ncols,
                                                               int8_t* dst, int32_t* __restrict__ status)
{
    __shared__ uint16_t tab[LRFI_TAB_N * INF_LANES];
    const int slot = (int)blockIdx.x * INF_LANES + (int)threadIdx.x;
    if (slot >= ncols) return;
    const InflateCol c = cols[slot];
    const lrfi_tab t = {tab + threadIdx.x, INF_LANES};
    status[c.k] = lrfi_inflate(src + c.src_off, c.src_len, dst + c.dst_off, c.rows, c.stride, t, nullptr);
}
