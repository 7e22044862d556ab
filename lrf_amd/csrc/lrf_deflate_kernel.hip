// lrf_deflate_kernel.hip — k_deflate_columns: one workgroup of 256 lanes owns one column of one matrix from its first byte to
// its Adler-32 (no hand-off between workgroups, no global atomics).  Everything that decides a byte is lrf_deflate_shared.h;
// this file only spreads the work over the lanes:
//   load    a tile of LRFD_T symbols of the column: row chunks of the matrix (all its columns: contiguous bytes) come in with
//           16-byte loads (the unaligned head and tail of a chunk byte by byte) into LDS, the column is picked out there
//   pass 1  histogram in LDS (LDS atomics) and the two Adler-32 sums, tile by tile
//   plan    lane 0 runs lrfd_plan: code lengths, codes, the form, the stream's exact length and the header bits
//   pass 2  per tile each lane adds up the bit lengths of its 8 consecutive symbols, a workgroup scan turns the sums into bit
//           offsets, the codes are OR-ed into a zeroed LDS staging buffer, its whole bytes go to the slot (lane k byte k) and
//           the bits of the last, partial byte open the next tile's staging.  STORED: the tile's bytes go to their places.
// A column of at most LRFD_T rows is loaded once and stays in LDS for both passes.
#define DFL_THREADS 256
#define DFL_PER_LANE (LRFD_T / DFL_THREADS) // 8 consecutive symbols per lane and tile
#define DFL_CHUNK 8192                      // bytes of a row chunk (at least two rows: cols <= 4096)
#define DFL_STAGE_WORDS ((LRFD_HDR_MAX + LRFD_T * LRFD_LIT_LIMIT / 8 + 16 + 3) / 4)
static_assert(DFL_PER_LANE == 8, "a lane reads its symbols of a tile as two words");

struct DeflateMat {
    int64_t src_off, rows, cols, dst_off, len_off;
    int64_t col0; // number of columns in the matrices before this one: workgroup col0 + j owns column j
};

// tile `t` of column j into colbuf (bytes [0, nr)); `chunk` is the row-chunk buffer
__device__ static void dfl_load_tile(const int8_t* __restrict__ mat, int64_t rows, int64_t cols, int64_t j, int64_t t, int nr, uint4* chunk,
                                     uint32_t* colbuf)
{
    const int tid = threadIdx.x;
    uint8_t* cbytes = (uint8_t*)chunk;
    uint8_t* col = (uint8_t*)colbuf;
    const int cr = (int)(DFL_CHUNK / cols); // rows per chunk
    for (int c0 = 0; c0 < nr; c0 += cr) {
        const int nrc = nr - c0 < cr ? nr - c0 : cr;
        const int8_t* g = mat + (t * LRFD_T + c0) * cols; // first byte of the chunk
        const int nbytes = (int)(nrc * cols);
        const int o = (int)(reinterpret_cast<uintptr_t>(g) & 15); // the chunk sits in LDS at the same offset from a 16-byte boundary
        int head = (16 - o) & 15;
        if (head > nbytes) head = nbytes;
        const int nvec = (nbytes - head) / 16, tail0 = head + 16 * nvec;
        const uint4* gv = (const uint4*)(g + head);
        for (int v = tid; v < nvec; v += DFL_THREADS) chunk[(o + head) / 16 + v] = gv[v];
        if (tid < head) cbytes[o + tid] = (uint8_t)g[tid];
        if (tid >= 32 && tid - 32 < nbytes - tail0) cbytes[o + tail0 + tid - 32] = (uint8_t)g[tail0 + tid - 32];
        __syncthreads();
        for (int r = tid; r < nrc; r += DFL_THREADS) col[c0 + r] = cbytes[o + r * cols + j];
        __syncthreads();
    }
}

__global__ __launch_bounds__(DFL_THREADS) void k_deflate_columns(const int8_t* __restrict__ src, const DeflateMat* __restrict__ mats, int nmats,
                                                                 uint8_t* __restrict__ dst, int32_t* __restrict__ out_len)
{
    __shared__ uint4 chunk[DFL_CHUNK / 16 + 2];
    __shared__ uint32_t colbuf[LRFD_T / 4];
    __shared__ uint32_t stage[DFL_STAGE_WORDS];
    __shared__ lrfd_work wk;
    __shared__ uint32_t red[2];
    __shared__ uint32_t wave_sum[DFL_THREADS / 64];
    const int tid = threadIdx.x;
    // the matrix of this workgroup: the last one whose first column is <= blockIdx.x
    int lo = 0, hi = nmats - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (mats[mid].col0 <= (int64_t)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const DeflateMat m = mats[lo];
    const int64_t j = (int64_t)blockIdx.x - m.col0, rows = m.rows, cols = m.cols;
    const int8_t* mat = src + m.src_off;
    uint8_t* slot = dst + m.dst_off + j * lrfd_bound(rows);
    const int64_t ntiles = (rows + LRFD_T - 1) / LRFD_T;

    for (int i = tid; i < LRFD_NLIT; i += DFL_THREADS) wk.freq[i] = 0;
    for (int i = tid; i < DFL_STAGE_WORDS; i += DFL_THREADS) stage[i] = 0;
    if (tid < 2) red[tid] = 0;
    __syncthreads();

    // ---- pass 1: histogram and Adler sums
    uint64_t a_acc = 0, b_acc = 0;
    for (int64_t t = 0; t < ntiles; t++) {
        const int nr = (int)(rows - t * LRFD_T < LRFD_T ? rows - t * LRFD_T : LRFD_T);
        dfl_load_tile(mat, rows, cols, j, t, nr, chunk, colbuf);
        const uint32_t w0 = colbuf[2 * tid], w1 = colbuf[2 * tid + 1];
        uint32_t a = 0, b = 0;
        // (rows - i) mod 65521 of the lane's first symbol; its next ones count down from it
        const int32_t wgt = (int32_t)((rows - (t * LRFD_T + DFL_PER_LANE * tid)) % (int64_t)LRFD_ADLER);
#pragma unroll
        for (int e = 0; e < DFL_PER_LANE; e++) {
            const int k = DFL_PER_LANE * tid + e;
            if (k < nr) {
                const uint32_t d = ((e < 4 ? w0 : w1) >> (8 * (e & 3))) & 0xffu;
                atomicAdd(&wk.freq[d], 1u);
                a += d;
                b += (uint32_t)(wgt - e < 0 ? wgt - e + (int32_t)LRFD_ADLER : wgt - e) * d;
            }
        }
        a_acc += a;
        b_acc += b;
        __syncthreads(); // (the next load overwrites colbuf)
    }
    atomicAdd(&red[0], (uint32_t)(a_acc % LRFD_ADLER));
    atomicAdd(&red[1], (uint32_t)(b_acc % LRFD_ADLER));
    __syncthreads();
    if (tid == 0) {
        wk.freq[256] = 1;
        lrfd_plan(&wk, rows, (uint8_t*)stage);
    }
    __syncthreads();
    const int form = wk.form;
    const int64_t stream_len = wk.stream_len;
    const uint8_t* sbytes = (const uint8_t*)stage;

    // ---- pass 2
    if (form == LRFD_STORED) {
        if (tid < 2) slot[tid] = sbytes[tid];
        const int64_t nblocks = (rows + LRFD_STORED_MAX - 1) / LRFD_STORED_MAX;
        for (int64_t blk = tid; blk < nblocks; blk += DFL_THREADS) {
            uint8_t h[5];
            lrfd_stored_block_header(rows, blk, h);
            for (int e = 0; e < 5; e++) slot[2 + blk * (LRFD_STORED_MAX + 5) + e] = h[e];
        }
        for (int64_t t = 0; t < ntiles; t++) {
            const int nr = (int)(rows - t * LRFD_T < LRFD_T ? rows - t * LRFD_T : LRFD_T);
            if (ntiles > 1) dfl_load_tile(mat, rows, cols, j, t, nr, chunk, colbuf);
            const uint8_t* col = (const uint8_t*)colbuf;
            for (int k = tid; k < nr; k += DFL_THREADS) slot[lrfd_stored_pos(t * LRFD_T + k)] = col[k];
            __syncthreads();
        }
    } else {
        uint32_t sbits = wk.hdr_bits; // bits now in the staging buffer
        int64_t flushed = 0;          // bytes of the stream already in the slot
        for (int64_t t = 0; t < ntiles; t++) {
            const int nr = (int)(rows - t * LRFD_T < LRFD_T ? rows - t * LRFD_T : LRFD_T);
            const bool last = t + 1 == ntiles;
            if (ntiles > 1) dfl_load_tile(mat, rows, cols, j, t, nr, chunk, colbuf);
            const uint32_t w0 = colbuf[2 * tid], w1 = colbuf[2 * tid + 1];
            uint32_t nbits = 0;
#pragma unroll
            for (int e = 0; e < DFL_PER_LANE; e++)
                if (DFL_PER_LANE * tid + e < nr) nbits += wk.len[((e < 4 ? w0 : w1) >> (8 * (e & 3))) & 0xffu];
            // exclusive scan over the workgroup
            uint32_t incl = nbits;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if ((tid & 63) >= d) incl += up;
            }
            if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (int w = 0; w < DFL_THREADS / 64; w++) {
                if (w < (tid >> 6)) before += wave_sum[w];
                total += wave_sum[w];
            }
            uint32_t pos = sbits + before + incl - nbits;
#pragma unroll
            for (int e = 0; e < DFL_PER_LANE; e++)
                if (DFL_PER_LANE * tid + e < nr) {
                    const uint32_t d = ((e < 4 ? w0 : w1) >> (8 * (e & 3))) & 0xffu;
                    const uint32_t c = wk.code[d], n = wk.len[d], sh = pos & 31;
                    atomicOr(&stage[pos >> 5], c << sh);
                    if (sh + n > 32) atomicOr(&stage[(pos >> 5) + 1], c >> (32 - sh));
                    pos += n;
                }
            uint32_t end = sbits + total;
            if (last) {
                if (tid == 0) {
                    const uint32_t c = wk.code[256], n = wk.len[256], sh = end & 31;
                    atomicOr(&stage[end >> 5], c << sh);
                    if (sh + n > 32) atomicOr(&stage[(end >> 5) + 1], c >> (32 - sh));
                }
                end += wk.len[256];
            }
            __syncthreads();
            const uint32_t nflush = last ? (end + 7) / 8 : end / 8;
            for (uint32_t k = tid; k < nflush; k += DFL_THREADS) slot[flushed + k] = sbytes[k];
            const uint32_t carry = sbytes[nflush < 4u * DFL_STAGE_WORDS ? nflush : 0]; // the partial byte (unused after the last tile)
            flushed += nflush;
            __syncthreads();
            if (!last) {
                for (int i = tid; i < DFL_STAGE_WORDS; i += DFL_THREADS) stage[i] = i == 0 ? carry : 0;
                sbits = end & 7;
                __syncthreads();
            }
        }
    }
    if (tid == 0) {
        uint8_t tr[4];
        lrfd_adler_bytes((1u + red[0]) % LRFD_ADLER, (uint32_t)((rows % LRFD_ADLER + red[1]) % LRFD_ADLER), tr);
        for (int e = 0; e < 4; e++) slot[stream_len - 4 + e] = tr[e];
        out_len[m.len_off + j] = (int32_t)stream_len;
    }
}
