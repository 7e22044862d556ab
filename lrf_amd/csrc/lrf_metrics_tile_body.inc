// lrf_metrics_tile_body.inc — one tile of one plane of the SSIM: everything behind "which plane, which tile, where a and b
// start, H, W, the data range": staging, row sums, column sums, the per-thread sums in row order, the workgroup's tree, the
// slot and the squared error.  Included in the body of k_ssim_tiles<V> (lrf_metrics_kernel.hip) and of k_ragged_ssim_tiles<V>
// (lrf_metrics_ragged_kernel.hip): the same statements, so a plane's tile has the same bits from either.  The including kernel
// declares the LDS (LRF_MT_TILE_LDS) and, under these names,
//   T, tid            the piece type MtVec<V>::T and threadIdx.x
//   a, b, plane       the images; the plane's [H][W] starts plane H W bytes into both (aligned to V, W % V == 0)
//   H, W, ntx, nty    the plane's size and its tiles; ty, tx: this workgroup's tile
//   mm, C             (max, 255 - min) of the pair's a image at mm[2 * (plane / C)]; sse + plane / C takes the squared error
//   slots             the tile's sum of S goes to slots[blockIdx.x]
    const int y0 = ty * LRF_MT_TH, x0 = tx * LRF_MT_TW;
    const long base = (long)plane * H * W;
    if (tid == 0) s_sse = 0;

    // ---- stage the pixels the tile's windows cover; rows and pieces outside the image are zeros (their windows are not counted)
    constexpr int NCH = ((LRF_MT_HC + 3) / 4 * 4 + V - 1) / V; // pieces of V bytes per row: the 72 bytes the next phase reads, or more
    const bool last_row = ty == nty - 1, last_col = tx == ntx - 1;
    unsigned my_sse = 0;
    for (int it = tid; it < LRF_MT_HR * NCH; it += 256) {
        const int r = it / NCH, col = (it - r * NCH) * V;
        const int y = y0 + r, x = x0 + col;
        const bool in = y < H && x + V <= W;
        T va = T(), vb = T();
        if (in) {
            const long off = base + (long)y * W + x;
            va = *reinterpret_cast<const T*>(a + off);
            vb = *reinterpret_cast<const T*>(b + off);
        }
        *reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(rawA) + r * LRF_MT_PITCH + col) = va;
        *reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(rawB) + r * LRF_MT_PITCH + col) = vb;
        // the squared error of a pixel is added by the tile whose 24 x 64 origin block holds it (the last tile row / column:
        // everything down to / right of it as well); V divides 64, so a piece is owned whole or not at all
        if (in && (r < LRF_MT_TH || last_row) && (col < LRF_MT_TW || last_col)) {
            if constexpr (V == 16) my_sse += mt_sse4(va.x, vb.x) + mt_sse4(va.y, vb.y) + mt_sse4(va.z, vb.z) + mt_sse4(va.w, vb.w);
            else my_sse += mt_sse4(va, vb);
        }
    }
    __syncthreads();
    if (my_sse) atomicAdd(&s_sse, my_sse); // <= 30 * 80 * 255^2 per tile: 32 bits

    // ---- sums of 7 along the rows: a thread per (row, 8 window columns) reads 14 + 2 pixels of a and b
    if (tid < LRF_MT_HR * (LRF_MT_TW / 8)) {
        const int r = tid >> 3, s = tid & 7;
        const uint2* pa = reinterpret_cast<const uint2*>(rawA + r * (LRF_MT_PITCH / 4) + 2 * s);
        const uint2* pb = reinterpret_cast<const uint2*>(rawB + r * (LRF_MT_PITCH / 4) + 2 * s);
        const uint2 a0 = pa[0], a1 = pa[1], b0 = pb[0], b1 = pb[1];
        const unsigned wa[4] = {a0.x, a0.y, a1.x, a1.y}, wb[4] = {b0.x, b0.y, b1.x, b1.y};
        unsigned p[14], q[14], xy[14];
#pragma unroll
        for (int k = 0; k < 14; k++) {
            const unsigned av = mt_byte(wa[k >> 2], k & 3), bv = mt_byte(wb[k >> 2], k & 3);
            p[k] = av | (bv << 16);
            q[k] = __umul24(av, av) + __umul24(bv, bv);
            xy[k] = __umul24(av, bv);
        }
        unsigned o1[8], o2[8], o3[8];
        unsigned s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) { s1 += p[k]; s2 += q[k]; s3 += xy[k]; }
        o1[0] = s1; o2[0] = s2; o3[0] = s3;
#pragma unroll
        for (int i = 1; i < 8; i++) {
            s1 += p[i + 6] - p[i - 1]; // (both halves stay within 16 bits: each is a sum of 7 bytes again)
            s2 += q[i + 6] - q[i - 1];
            s3 += xy[i + 6] - xy[i - 1];
            o1[i] = s1; o2[i] = s2; o3[i] = s3;
        }
        uint4* d1 = reinterpret_cast<uint4*>(h1 + r * LRF_MT_TW + 8 * s);
        uint4* d2 = reinterpret_cast<uint4*>(h2 + r * LRF_MT_TW + 8 * s);
        uint4* d3 = reinterpret_cast<uint4*>(h3 + r * LRF_MT_TW + 8 * s);
        d1[0] = make_uint4(o1[0], o1[1], o1[2], o1[3]); d1[1] = make_uint4(o1[4], o1[5], o1[6], o1[7]);
        d2[0] = make_uint4(o2[0], o2[1], o2[2], o2[3]); d2[1] = make_uint4(o2[4], o2[5], o2[6], o2[7]);
        d3[0] = make_uint4(o3[0], o3[1], o3[2], o3[3]); d3[1] = make_uint4(o3[4], o3[5], o3[6], o3[7]);
    }
    __syncthreads();

    // ---- sliding sum of 7 down a column: thread = (band of 6 rows, column); then S of each window, in float64
    const unsigned vmax = mm[2 * (plane / (unsigned)C)], vmin = 255u - mm[2 * (plane / (unsigned)C) + 1];
    const double L = (double)(vmax - vmin); // data_range of the first image: max - min
    const double c1 = (0.01 * L) * (0.01 * L), c2 = (0.03 * L) * (0.03 * L);
    const int band = tid >> 6, cx = tid & 63;
    const int r0 = band * (LRF_MT_TH / 4);
    const bool col_ok = x0 + cx < W - 6;
    unsigned v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        v1 += h1[(r0 + k) * LRF_MT_TW + cx];
        v2 += h2[(r0 + k) * LRF_MT_TW + cx];
        v3 += h3[(r0 + k) * LRF_MT_TW + cx];
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LRF_MT_TH / 4; j++) {
        v1 += h1[(r0 + j + 6) * LRF_MT_TW + cx];
        v2 += h2[(r0 + j + 6) * LRF_MT_TW + cx];
        v3 += h3[(r0 + j + 6) * LRF_MT_TW + cx];
        const int sx = (int)(v1 & 0xffffu), sy = (int)(v1 >> 16);
        const int P = __mul24(sx, sy), Q = __mul24(sx, sx) + __mul24(sy, sy);
        const int N1 = __mul24(49, (int)v3) - P;     // 49 Sxy - Sx Sy       (Sxy < 2^22)
        const int N2 = __mul24(49, (int)v2) - Q;     // 49 (Sxx + Syy) - Q   (Sxx + Syy < 2^23)
        const double A1 = (double)P * (2.0 / 2401.0) + c1, A2 = (double)N1 * (2.0 / 2352.0) + c2;
        const double B1 = (double)Q * (1.0 / 2401.0) + c1, B2 = (double)N2 * (1.0 / 2352.0) + c2;
        const double S = (A1 * A2) / (B1 * B2);
        acc += (col_ok && y0 + r0 + j < H - 6) ? S : 0.0;
        v1 -= h1[(r0 + j) * LRF_MT_TW + cx];
        v2 -= h2[(r0 + j) * LRF_MT_TW + cx];
        v3 -= h3[(r0 + j) * LRF_MT_TW + cx];
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        slots[blockIdx.x] = red[0];
        if (s_sse) atomicAdd(sse + plane / (unsigned)C, (unsigned long long)s_sse);
    }
