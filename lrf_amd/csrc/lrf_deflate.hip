// lrf_deflate.hip — lrf_deflate_columns_i8 (include/lrf_hip.h): the zlib streams of factor columns, written on the device, and
// lrf_deflate_sizes_i8: their lengths alone.  The format lives in lrf_deflate_shared.h, the kernels in lrf_deflate_kernel.hip and
// lrf_deflate_sizes_kernel.hip; this file checks a call's every range before the launch and sends the matrix table to the device
// stream-ordered.
#include "lrf_host.h"
#include "lrf_deflate_shared.h"
#include "lrf_deflate_kernel.hip"
#include "lrf_deflate_sizes_kernel.hip"

// The matrix table of one call on its way to the device: stream-ordered, no wait for the stream (as the crop table of
// lrf_qmf_decode_crops_rgb_u8 travels).  The pinned staging slots take turns; a slot is written again only after the event
// recorded behind its last copy says that copy has run.  The device table is one buffer: the copy of a call is ordered behind
// the kernel of the call before it on the same stream.
static int stage_deflate_table(lrf_ctx* c, const std::vector<DeflateMat>& table)
{
    const size_t bytes = table.size() * sizeof(DeflateMat);
    int rc = ensure(c, c->deflate_tab, bytes);
    if (rc) return rc;
    lrf_ctx::CropSlot& s = c->deflate_slot[c->deflate_next];
    c->deflate_next = (c->deflate_next + 1) % LRF_CROP_SLOTS;
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
    HIP_TRY(hipMemcpyAsync(c->deflate_tab.p, s.h, bytes, hipMemcpyHostToDevice, c->stream));
    s.in_flight = true;
    HIP_TRY(hipEventRecord(s.copied, c->stream));
    return LRF_OK;
}

// The host checks both entry points make before a launch, and the device table: every matrix's ranges against src_len, dst_len
// (dst_len < 0: the call writes no slots and dst_off is ignored) and out_len_count, no two matrices sharing slot bytes or length
// entries.  A workgroup owns `per` consecutive columns of a matrix; table[i].col0 counts the workgroups in front of matrix i and
// *grid all of them.
static int deflate_table_checked(int64_t src_len, int64_t n, const lrf_deflate_matrix* mats, int64_t dst_len, int64_t out_len_count, int64_t per,
                                 std::vector<DeflateMat>& table, int64_t* grid)
{
    const bool slotted = dst_len >= 0;
    if (n < 1 || n > (1 << 20)) return set_err(LRF_EINVAL, "n=%ld out of range [1,2^20]", (long)n);
    if (src_len < 1 || (slotted && dst_len < 1) || out_len_count < 1) return set_err(LRF_EINVAL, "a buffer length below 1");
    struct Range {
        int64_t off, len;
    };
    table.resize((size_t)n);
    std::vector<Range> dr, lr((size_t)n);
    if (slotted) dr.resize((size_t)n);
    int64_t col0 = 0;
    for (int64_t i = 0; i < n; i++) {
        const lrf_deflate_matrix& m = mats[i];
        if (m.rows < 1 || m.rows > LRFD_MAX_ROWS) return set_err(LRF_EINVAL, "matrix %ld: rows=%ld out of range [1,2^30]", (long)i, (long)m.rows);
        if (m.cols < 1 || m.cols > 4096) return set_err(LRF_EINVAL, "matrix %ld: cols=%ld out of range [1,4096]", (long)i, (long)m.cols);
        if (m.src_off < 0 || (slotted && m.dst_off < 0) || m.len_off < 0) return set_err(LRF_EINVAL, "matrix %ld: negative offset", (long)i);
        // (every term is checked against the length before it is added to an offset: no sum can wrap; rows cols < 2^42)
        const int64_t bytes = m.rows * m.cols, slots = m.cols * lrfd_bound(m.rows);
        if (bytes > src_len || m.src_off > src_len - bytes) return set_err(LRF_EINVAL, "matrix %ld: its %ld bytes at %ld leave the buffer of %ld bytes", (long)i, (long)bytes, (long)m.src_off, (long)src_len);
        if (slotted && (slots > dst_len || m.dst_off > dst_len - slots)) return set_err(LRF_EINVAL, "matrix %ld: its slots (%ld bytes at %ld) leave the buffer of %ld bytes", (long)i, (long)slots, (long)m.dst_off, (long)dst_len);
        if (m.cols > out_len_count || m.len_off > out_len_count - m.cols) return set_err(LRF_EINVAL, "matrix %ld: its %ld lengths at %ld leave the buffer of %ld entries", (long)i, (long)m.cols, (long)m.len_off, (long)out_len_count);
        table[(size_t)i] = DeflateMat{m.src_off, m.rows, m.cols, slotted ? m.dst_off : 0, m.len_off, col0};
        if (slotted) dr[(size_t)i] = Range{m.dst_off, slots};
        lr[(size_t)i] = Range{m.len_off, m.cols};
        col0 += (m.cols + per - 1) / per;
    }
    if (col0 > INT32_MAX) return set_err(LRF_ENOTSUP, "%ld workgroups in one call: split the list", (long)col0);
    for (std::vector<Range>* r : {&dr, &lr}) { // no two matrices may share output bytes or length entries
        std::sort(r->begin(), r->end(), [](const Range& a, const Range& b) { return a.off < b.off; });
        for (size_t i = 1; i < r->size(); i++)
            if ((*r)[i].off - (*r)[i - 1].off < (*r)[i - 1].len) return set_err(LRF_EINVAL, "the %s of two matrices overlap (at %ld)", r == &dr ? "slots" : "length entries", (long)(*r)[i].off);
    }
    *grid = col0;
    return LRF_OK;
}

extern "C" {

int64_t lrf_deflate_bound(int64_t len) { return len < 1 ? -1 : lrfd_bound(len); }

int lrf_deflate_columns_i8(lrf_ctx* c, const int8_t* src, int64_t src_len, int64_t n, const lrf_deflate_matrix* mats, uint8_t* dst, int64_t dst_len,
                           int32_t* out_len, int64_t out_len_count)
{
    if (!c || !src || !mats || !dst || !out_len) return set_err(LRF_EINVAL, "NULL argument");
    if (dst_len < 1) return set_err(LRF_EINVAL, "a buffer length below 1");
    std::vector<DeflateMat> table;
    int64_t grid = 0;
    int rc = deflate_table_checked(src_len, n, mats, dst_len, out_len_count, 1, table, &grid);
    if (rc) return rc;
    LRF_ON_DEVICE(c);
    rc = stage_deflate_table(c, table);
    if (rc) return rc;
    hipLaunchKernelGGL(k_deflate_columns, dim3((unsigned)grid), dim3(DFL_THREADS), 0, c->stream, src, (const DeflateMat*)c->deflate_tab.p, (int)n, dst, out_len);
    LAUNCH_CHECK();
    return LRF_OK;
}

int lrf_deflate_sizes_i8(lrf_ctx* c, const int8_t* src, int64_t src_len, int64_t n, const lrf_deflate_matrix* mats, int32_t* out_len, int64_t out_len_count)
{
    if (!c || !src || !mats || !out_len) return set_err(LRF_EINVAL, "NULL argument");
    std::vector<DeflateMat> table;
    int64_t grid = 0;
    int rc = deflate_table_checked(src_len, n, mats, -1, out_len_count, DFS_CG, table, &grid);
    if (rc) return rc;
    LRF_ON_DEVICE(c);
    rc = stage_deflate_table(c, table);
    if (rc) return rc;
    hipLaunchKernelGGL(k_deflate_sizes, dim3((unsigned)grid), dim3(DFS_THREADS), 0, c->stream, src, (const DeflateMat*)c->deflate_tab.p, (int)n, out_len);
    LAUNCH_CHECK();
    return LRF_OK;
}

} // extern "C"
