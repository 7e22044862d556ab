// lrf_inflate.hip — lrf_inflate_columns_i8 (include/lrf_hip.h): zlib streams of factor columns, inflated on the device.  The
// decoder lives in lrf_inflate_shared.h, the kernel in lrf_inflate_kernel.hip, the lane order in lrf_plan.cpp (plan_inflate);
// this file checks a call's every range before the launch and sends the column table to the device stream-ordered.
#include "lrf_host.h"
#include "lrf_inflate_shared.h"
#include "lrf_inflate_kernel.hip"

// The column table of one call on its way to the device: stream-ordered, no wait for the stream (as the table of
// lrf_deflate_columns_i8 travels).  The pinned staging slots take turns; a slot is written again only after the event recorded
// behind its last copy says that copy has run, and grows when a table is larger than it.
static int stage_inflate_table(lrf_ctx* c, const std::vector<InflateCol>& table)
{
    const size_t bytes = table.size() * sizeof(InflateCol);
    int rc = ensure(c, c->inflate_tab, bytes);
    if (rc) return rc;
    lrf_ctx::CropSlot& s = c->inflate_slot[c->inflate_next];
    c->inflate_next = (c->inflate_next + 1) % LRF_CROP_SLOTS;
    if (!s.copied) HIP_TRY(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    else if (s.in_flight) HIP_TRY(hipEventSynchronize(s.copied));
    s.in_flight = false;
    if (bytes > s.cap) {
        if (s.h) HIP_TRY(hipHostFree(s.h));
        s.h = nullptr;
        s.cap = 0;
        HIP_TRY(hipHostMalloc(&s.h, bytes + bytes / 2, hipHostMallocDefault));
        s.cap = bytes + bytes / 2;
    }
    memcpy(s.h, table.data(), bytes);
    HIP_TRY(hipMemcpyAsync(c->inflate_tab.p, s.h, bytes, hipMemcpyHostToDevice, c->stream));
    s.in_flight = true;
    HIP_TRY(hipEventRecord(s.copied, c->stream));
    return LRF_OK;
}

extern "C" {

int lrf_inflate_columns_i8(lrf_ctx* c, const uint8_t* src, int64_t src_len, int64_t n, const lrf_inflate_matrix* mats, const int64_t* col_off,
                           const int32_t* col_len, int64_t ncols, int8_t* dst, int64_t dst_len, int32_t* status)
{
    if (!c || !src || !mats || !col_off || !col_len || !dst || !status) return set_err(LRF_EINVAL, "NULL argument");
    if (n < 1 || n > (1 << 20)) return set_err(LRF_EINVAL, "n=%ld out of range [1,2^20]", (long)n);
    if (src_len < 1 || dst_len < 1) return set_err(LRF_EINVAL, "a buffer length below 1");
    if (ncols < 1 || ncols > INT32_MAX - 64) return set_err(LRF_EINVAL, "ncols=%ld out of range", (long)ncols);
    struct Range {
        int64_t off, len;
    };
    std::vector<Range> dr((size_t)n), sr((size_t)n);
    std::vector<InflateMatDim> dims((size_t)n);
    int64_t sum = 0;
    for (int64_t i = 0; i < n; i++) {
        const lrf_inflate_matrix& m = mats[i];
        if (m.rows < 1 || m.rows > LRFI_MAX_ROWS) return set_err(LRF_EINVAL, "matrix %ld: rows=%ld out of range [1,2^30]", (long)i, (long)m.rows);
        if (m.cols < 1 || m.cols > 4096) return set_err(LRF_EINVAL, "matrix %ld: cols=%ld out of range [1,4096]", (long)i, (long)m.cols);
        if (m.dst_off < 0 || m.first < 0) return set_err(LRF_EINVAL, "matrix %ld: negative offset", (long)i);
        // (every term is checked against the length before it is added to an offset: no sum can wrap; rows cols < 2^42)
        const int64_t bytes = m.rows * m.cols;
        if (bytes > dst_len || m.dst_off > dst_len - bytes) return set_err(LRF_EINVAL, "matrix %ld: its %ld bytes at %ld leave the buffer of %ld bytes", (long)i, (long)bytes, (long)m.dst_off, (long)dst_len);
        if (m.cols > ncols || m.first > ncols - m.cols) return set_err(LRF_EINVAL, "matrix %ld: its %ld streams from %ld leave the %ld streams of the call", (long)i, (long)m.cols, (long)m.first, (long)ncols);
        dr[(size_t)i] = Range{m.dst_off, bytes};
        sr[(size_t)i] = Range{m.first, m.cols};
        dims[(size_t)i] = InflateMatDim{(long)m.rows, (int)m.cols};
        sum += m.cols;
    }
    if (sum != ncols) return set_err(LRF_EINVAL, "ncols=%ld, the matrices have %ld columns", (long)ncols, (long)sum);
    for (std::vector<Range>* r : {&dr, &sr}) { // no two matrices may share output bytes or streams
        std::sort(r->begin(), r->end(), [](const Range& a, const Range& b) { return a.off < b.off; });
        for (size_t i = 1; i < r->size(); i++)
            if ((*r)[i].off - (*r)[i - 1].off < (*r)[i - 1].len) return set_err(LRF_EINVAL, "the %s of two matrices overlap (at %ld)", r == &dr ? "bytes" : "streams", (long)(*r)[i].off);
    }
    for (int64_t k = 0; k < ncols; k++) {
        if (col_len[k] < 8) return set_err(LRF_EINVAL, "stream %ld: %d bytes (a zlib stream has at least 8)", (long)k, (int)col_len[k]);
        if (col_off[k] < 0 || col_len[k] > src_len || col_off[k] > src_len - col_len[k]) return set_err(LRF_EINVAL, "stream %ld: its %d bytes at %ld leave the buffer of %ld bytes", (long)k, (int)col_len[k], (long)col_off[k], (long)src_len);
    }
    const std::vector<InflateSlot> slots = plan_inflate(dims);
    std::vector<InflateCol> table(slots.size());
    for (size_t s = 0; s < slots.size(); s++) {
        const lrf_inflate_matrix& m = mats[slots[s].mat];
        const int64_t k = m.first + slots[s].col;
        table[s] = InflateCol{col_off[k], m.dst_off + slots[s].col, col_len[k], (int32_t)m.rows, (int32_t)m.cols, (int32_t)k};
    }
    LRF_ON_DEVICE(c);
    int rc = stage_inflate_table(c, table);
    if (rc) return rc;
    {
        Prof p(c, LRF_K_INFLATE);
        hipLaunchKernelGGL(k_inflate_columns, dim3((unsigned)((ncols + INF_LANES - 1) / INF_LANES)), dim3(INF_LANES), 0, c->stream, src,
                           (const InflateCol*)c->inflate_tab.p, (int)ncols, dst, status);
    }
    LAUNCH_CHECK();
    return LRF_OK;
}

} // extern "C"
