// lrf_deflate_sizes_kernel.hip — k_deflate_sizes: the length of every column's stream without the stream.  One workgroup of 256
// lanes owns DFS_CG consecutive columns of one matrix (no hand-off between workgroups, no global atomics).  Everything that
// decides a length is lrfd_measure of lrf_deflate_shared.h; this file only spreads the work over the lanes:
//   count    the workgroup streams the matrix's rows * cols contiguous bytes ONCE, with 16-byte loads (the unaligned head and
//            tail byte by byte); a byte whose column is one of the group's goes into that column's histogram in LDS (LDS
//            atomics on 32-bit counts).  A byte's column follows from its flat index: a lane works out the column of its
//            first byte once, steps it per byte inside a vector and by (16 * 256) mod cols from one vector to its next — no
//            division per byte or per vector.  Nothing is staged in LDS and no Adler sum is taken (neither changes a length).
//   measure  one lane per column, the lanes 32 apart (two per wave, in different halves of it), each runs lrfd_measure on
//            its own lrfd_count in LDS and stores its column's length.  The structs lie an odd number of dwords apart, so the
//            lanes' equal-index accesses fall into different banks.
// A matrix is read ceil(cols / DFS_CG) times, not cols times; a slot is never written.
#define DFS_THREADS 256
#define DFS_CG LRF_DEFLATE_CG
#define DFS_LANE_STEP (DFS_THREADS / DFS_CG)        // lane k * DFS_LANE_STEP measures column k of the group
#define DFS_STRIDE_W ((sizeof(lrfd_count) / 4) | 1) // dwords from one column's lrfd_count to the next: odd
static_assert(sizeof(lrfd_count) % 4 == 0 && DFS_THREADS % DFS_CG == 0 && DFS_CG >= 8, "k_deflate_sizes: layout of the group's work structs");

// the counts of the 16 bytes of x, the first of them in column c of `cols`; columns [j0, j0 + ncg) are the group's
__device__ static inline void dfs_count_vec(uint32_t* wk, const uint4 x, int c, int cols, int j0, int ncg)
{
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t k = (uint32_t)(c - j0);
        if (k < (uint32_t)ncg) atomicAdd(&wk[k * DFS_STRIDE_W + ((w[e >> 2] >> (8 * (e & 3))) & 0xffu)], 1u);
        c = c + 1 == cols ? 0 : c + 1;
    }
}

// mats[i].col0 counts the column GROUPS in the matrices before matrix i here: workgroup col0 + g owns columns
// [g * DFS_CG, min(cols, (g + 1) * DFS_CG)); dst_off is not read
__global__ __launch_bounds__(DFS_THREADS) void k_deflate_sizes(const int8_t* __restrict__ src, const DeflateMat* __restrict__ mats, int nmats,
                                                               int32_t* __restrict__ out_len)
{
    __shared__ uint32_t wk[DFS_CG * DFS_STRIDE_W];
    const int tid = threadIdx.x;
    // the matrix of this workgroup: the last one whose first group is <= blockIdx.x
    int lo = 0, hi = nmats - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (mats[mid].col0 <= (int64_t)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const DeflateMat m = mats[lo];
    const int cols = (int)m.cols, j0 = (int)((int64_t)blockIdx.x - m.col0) * DFS_CG;
    const int ncg = cols - j0 < DFS_CG ? cols - j0 : DFS_CG;
    const int8_t* mat = src + m.src_off;
    const int64_t nbytes = m.rows * m.cols;

    for (int i = tid; i < DFS_CG * LRFD_NLIT; i += DFS_THREADS) wk[(i / LRFD_NLIT) * DFS_STRIDE_W + i % LRFD_NLIT] = 0;
    __syncthreads();

    // ---- count: head, whole 16-byte vectors, tail
    const int o = (int)(reinterpret_cast<uintptr_t>(mat) & 15);
    const int head = (int)((16 - o) & 15) < nbytes ? (16 - o) & 15 : (int)nbytes;
    const int64_t nvec = (nbytes - head) / 16, tail0 = head + 16 * nvec;
    const uint4* gv = (const uint4*)(mat + head);
    {
        const int step = (16 * DFS_THREADS) % cols;
        int c = (head + 16 * tid) % cols;
        for (int64_t v = tid; v < nvec; v += DFS_THREADS) {
            dfs_count_vec(wk, gv[v], c, cols, j0, ncg);
            c = c + step >= cols ? c + step - cols : c + step;
        }
    }
    if (tid < head) {
        const uint32_t k = (uint32_t)(tid % cols - j0);
        if (k < (uint32_t)ncg) atomicAdd(&wk[k * DFS_STRIDE_W + (uint8_t)mat[tid]], 1u);
    }
    if (tid >= 32 && tid - 32 < nbytes - tail0) {
        const uint32_t k = (uint32_t)((int)((tail0 + tid - 32) % cols) - j0);
        if (k < (uint32_t)ncg) atomicAdd(&wk[k * DFS_STRIDE_W + (uint8_t)mat[tail0 + tid - 32]], 1u);
    }
    __syncthreads();

    // ---- measure: the group's plans side by side
    if (tid % DFS_LANE_STEP == 0 && tid / DFS_LANE_STEP < ncg) {
        const int k = tid / DFS_LANE_STEP;
        lrfd_count* w = reinterpret_cast<lrfd_count*>(wk + k * DFS_STRIDE_W);
        lrfd_measured r;
        w->freq[256] = 1;
        lrfd_measure(w->freq, w->w, w->sym, w->len, w->seq, m.rows, &r);
        out_len[m.len_off + j0 + k] = (int32_t)r.stream_len;
    }
}
