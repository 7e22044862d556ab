#pragma once
// lrf_bcdp_kernel.hip — k_bcd_p<F16, NP32, FIRST>: the iterations of a large call in ONE launch, for every rank family of the
// 64-column path (round 4: ranks <= 8, iterations 2..K; round 5: the planes of ranks 9..16 and 17..32 and their mixes — (16,8,8),
// (26,13,13), ... — too, and, FIRST, at ranks <= 16 the call's first iteration as well: all K in the launch).
// Included by lrf_bcd_persist.hip after the block bodies it repeats operation for operation — ranks <= 8: k_bcd_w<0>
// (lrf_bcdw_kernel.hip; restated here with sc1 accesses, bcdp_w_block), 9..16: w16_block (lrf_bcdw16_kernel.hip), 17..32:
// w32_block (lrf_bcdw32_kernel.hip) — so the outputs are bit-identical to the launch-per-iteration path.
//
// What it removes: per iteration two kernel boundaries per family, the V-update launches (latency chains per matrix that leave
// the chip idle, or — when the families of a call run on streams of their own — starve behind the other family's U update:
// k_vupdate<16> took 180 us per launch beside k_bcd_w32 at (26,13,13)) and the drain / refill of every U-update launch.  How:
//   * items (iteration, block) are pulled in iteration-major order from one device-scope counter by whatever waves are
//     resident (a plain grid; a wave that finds the queue empty leaves); a block runs the body of its plane's rank family;
//   * a block stores its partials of X^T u / u^T u, drains its stores, and takes a ticket of its matrix; the LAST arriver of
//     (matrix, iteration) performs that matrix's V update on its own wave (partial sums in block order, the 64-row
//     Gauss-Seidel lane = row, the b table of the new V: bcdp_vupdate / bcdp_vupdate16 / bcdp_vupdate32 restate k_vupdate<8>,
//     k_vupdate<16>, k_vupdate_mid) and publishes flag[matrix] = iteration + 1;
//   * a block of iteration i + 1 polls its matrix's flag before it loads V.  Queue order makes this deadlock-free without
//     any assumption on dispatch: an item of iteration i + 1 is pulled only after every item of iteration i has been pulled
//     by a running wave, and running waves of iteration i never wait for later items.  In steady state nobody spins: the
//     same matrix's next item comes a full round of the queue later.  Every poll loop is BOUNDED (LRF_BCDP_MAX_POLLS): on
//     expiry the wave sets the error word (host memory) and returns, so the grid always drains; the host refuses the result.
//   * visibility across CUs / XCDs (MI355X_MICROARCH.md, inter-workgroup visibility): everything one wave writes and another
//     reads inside the launch — int8 U rows, partials, V table, b table — is stored `sc1` (write-through) and loaded `sc1`
//     (L1 bypass; MemSc1, lrf_device.h), every storing wave drains (`s_waitcnt vmcnt(0)`) before its ticket / flag, tickets
//     and flags are agent-scope atomics.  X is read-only and loaded plainly.

#ifndef LRF_BCDP_MAX_POLLS
#define LRF_BCDP_MAX_POLLS (1 << 20) // x ~1 us per poll: a second, then the wave gives up (error word)
#endif

struct BcdpSync {
    int head;        // next item
    int done;        // waves that have left
    int err;         // a poll of some launch on this state has expired: later launches leave at once (the host clears it)
    int pad[29];     // (head on a line of its own)
    int cell[1];     // [nplanes] tickets, then [nplanes] flags
};
// The queue head, tickets and flags start at zero.  The buffer is zeroed when it is allocated (and after a failed launch);
// after that every launch leaves it zeroed: the last wave to leave (`done`) clears what the launch used — no clearing kernel
// and no copy of an error word per call (the error word lives in page-locked host memory the kernel writes to directly).
// A FAILED launch (a poll expired) writes its sequence number `seq` (>= 1, counted per context by the host) to that word and
// sets `err` in this state; launches queued behind it find `err` set and leave at once without touching anything, so the
// host word keeps the number of the FIRST failed launch: that call's results and those of every later one are invalid until
// the host has looked (lrf_ctx_check / lrf_ctx_synchronize / lrf_pipe_wait_next / the next call's entry) and cleared the state.

// the tables of one rank pitch: 16 (ranks <= 16: LRF_RP, gt pitch LRF_GT_LD) or 64 (ranks 17..32: LRF_RPB, LRF_GTB_LD)
struct BcdpTabs {
    float *vf, *bf, *pp, *qp;
    const float* wf; // the initialisation's W0 = V0 / sigma (k_bcd_p<.., .., true>: the first iteration's old U is X @ W0)
};

// (address-space-1 pointers: `global_` instructions, never `flat_`)
__device__ __forceinline__ float ld_sc1(const float* p) { return __hip_atomic_load((const LRF_GLOBAL float*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(float* p, float v)
{
#ifdef LRF_BCDP_PLAIN_PSTORE // timing experiment only
    *p = v;
#else
    __hip_atomic_store((LRF_GLOBAL float*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// 16-B sc1 load at byte offset `off` from a WAVE-UNIFORM base: buffer_load_dwordx4 ... sc1 (aux bit 4 = sc1 on gfx950; a
// compiler-tracked load, so its result is waited for where it is used).  The raw buffer is unbounded (DATA_FORMAT 32).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4 ld_sc1_x4u(const void* base, unsigned off)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, 0x7fffffff, 0x00020000);
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16));
}
__device__ __forceinline__ f32x4 ld_sc1_x4(const float* base, unsigned off) { return __builtin_bit_cast(f32x4, ld_sc1_x4u(base, off)); }
// sc1 stores of 16, 8, 4, 2, 1 bytes at a naturally aligned address (no result register: a hand-issued store is safe; the
// wave's `s_waitcnt vmcnt(0)` before its ticket covers them)
__device__ __forceinline__ void st_sc1_x4(void* p, u32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st_sc1_x2(void* p, u32x2 v) { asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st_sc1_b32(void* p, unsigned v) { asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st_sc1_b16(void* p, unsigned v) { asm volatile("global_store_short %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st_sc1_b8(void* p, unsigned v) { asm volatile("global_store_byte %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }

// ranks <= 8: a block's partial slot (bcdp_w_block -> bcdp_vupdate) is DENSE at the plane's rank: P^T as [R][64] (entry (r, n) =
// sum over the block's rows of u_r x_n), then b' = U^T U as [R][R]; 64 R + R R floats, stored as whole 16-B chunks (the slot
// stride stays 64 LRF_RP floats: the padding of the last chunk lies inside the slot)
__device__ __forceinline__ int bcdp_dense_chunks(int R) { return (64 * R + R * R + 3) >> 2; }
#define LRF_BCDP_USTAGE 544 // bytes per wave: a 64-row U span (<= 512 B) at its address's phase mod 16, plus a 16-B read past it

// ---- V updates on ONE wave (lane = row of V).  lds: the wave's own share (>= 17 KB) --------------------------------------------
// a' = ((P0 + P1) + P2) + ... per element, b' likewise, at rank pitch 16: element e of the [64][16] table = lane + 64 j
// (j < 16), of the [16][16] table = lane + 64 j (j < 4); four blocks' loads in flight at a time
__device__ __forceinline__ void bcdp_sum16(const PlaneDesc& pd, const float* __restrict__ Ppart, const float* __restrict__ Qpart, int lane,
                                           float (&acc)[16], float (&q)[4])
{
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = 0.f;
    const float* Pp = Ppart + (long)pd.blk0 * 64 * LRF_RP + lane;
    const float* Qp = Qpart + (long)pd.blk0 * LRF_RP * LRF_RP + lane;
    constexpr int NB = 4; // blocks in flight: 80 registers (the kernel must stay inside 256 for two waves per SIMD)
    for (int b0 = 0; b0 < pd.nblk; b0 += NB) {
        float pv[NB][16], qv[NB][4];
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const long blk = b0 + k < pd.nblk ? b0 + k : b0;
#pragma unroll
            for (int j = 0; j < 16; j++) pv[k][j] = ld_sc1(Pp + blk * 64 * LRF_RP + 64 * j);
#pragma unroll
            for (int j = 0; j < 4; j++) qv[k][j] = ld_sc1(Qp + blk * LRF_RP * LRF_RP + 64 * j);
        }
#pragma unroll
        for (int k = 0; k < NB; k++)
            if (b0 + k < pd.nblk) {
#pragma unroll
                for (int j = 0; j < 16; j++) acc[j] = (b0 + k == 0) ? pv[k][j] : acc[j] + pv[k][j];
#pragma unroll
                for (int j = 0; j < 4; j++) q[j] = (b0 + k == 0) ? qv[k][j] : q[j] + qv[k][j];
            }
    }
}
__device__ __forceinline__ void bcdp_wave_sync() // LDS written by some lanes is read by others of the same wave
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ranks <= 8: the dense slots of the plane's blocks summed per element in block order (((P0 + P1) + P2) + ..., as bcdp_sum16)
// into sum_s (LDS, 16-B aligned): chunk c = lane + 64 j (j < 3: 64 R + R R <= 576 floats) of every slot, four blocks' loads
// in flight at a time (48 registers)
__device__ __forceinline__ void bcdp_sum_dense(const PlaneDesc& pd, const float* __restrict__ Ppart, int lane, float* sum_s)
{
    const int nch = bcdp_dense_chunks(pd.R), nj = (nch + 63) >> 6;
    const float* base = Ppart + (long)pd.blk0 * 64 * LRF_RP;
    f32x4 acc[3];
#pragma unroll
    for (int j = 0; j < 3; j++) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int NB = 4;
    for (int b0 = 0; b0 < pd.nblk; b0 += NB) {
        f32x4 pv[NB][3];
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const unsigned blk = b0 + k < pd.nblk ? b0 + k : b0;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int c = lane + 64 * j < nch ? lane + 64 * j : nch - 1; // (inside the slot)
                if (j < nj) pv[k][j] = ld_sc1_x4(base, (blk * 64 * LRF_RP + 4 * c) * 4);
            }
        }
#pragma unroll
        for (int k = 0; k < NB; k++)
            if (b0 + k < pd.nblk) {
#pragma unroll
                for (int j = 0; j < 3; j++)
                    if (j < nj) acc[j] = (b0 + k == 0) ? pv[k][j] : acc[j] + pv[k][j];
            }
    }
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (lane + 64 * j < nch) *reinterpret_cast<f32x4*>(&sum_s[4 * (lane + 64 * j)]) = acc[j];
}

// ranks <= 8: k_vupdate<8> (a_s [64][16], v_s [64][16], gt_s; sum_s: the summed dense slot)
__device__ __forceinline__ void bcdp_vupdate(const PlaneDesc& pd, int pli, const float* __restrict__ Ppart, float* __restrict__ Vf,
                                             float* __restrict__ Bf, int8_t* __restrict__ V8, const GsParams gp, int write_i8, float* lds, int lane)
{
    float* a_s = lds;
    float* v_s = lds + 64 * LRF_RP;
    float* gt_s = lds + 2 * 64 * LRF_RP;
    float* sum_s = gt_s + LRF_GT_STRIDE; // [R][64] then [R][R] (16-B aligned)
    const int R = pd.R;
    bcdp_sum_dense(pd, Ppart, lane, sum_s);
    const float* Vg = Vf + (long)pli * 64 * LRF_RP;
#pragma unroll
    for (int j = 0; j < 4; j++) *reinterpret_cast<f32x4*>(&v_s[4 * (lane + 64 * j)]) = ld_sc1_x4(Vg, 16 * (lane + 64 * j));
    bcdp_wave_sync();
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int idx = lane + 64 * j, n = idx >> 4, r = idx & 15; // a' entry (n, r)
        a_s[idx] = r < R ? sum_s[r * 64 + n] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int idx = lane + 64 * j, jj = idx >> 4, r = idx & 15; // b' entry (jj, r)
        if (jj < R && r < R) {
            const float q = sum_s[64 * R + jj * R + r];
            if (jj == r) {
                const float den = (q + 0.f) + LRF_EPS;
                gt_s[r * LRF_GT_LD + LRF_GT_DEN] = den;
                gt_s[r * LRF_GT_LD + LRF_GT_RDEN] = 1.0f / den;
            } else {
                gt_s[r * LRF_GT_LD + (jj < r ? jj : jj - 1)] = q;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {
        const bool native = (long)(R - 1) * 64 < 400;
        const float no_tab[17] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        gs_dispatch<8, false>(R, &a_s[lane * LRF_RP], &v_s[lane * LRF_RP], nullptr, 0, gt_s, native, gp, no_tab);
        float* Vp = Vf + (long)pli * 64 * LRF_RP + lane * LRF_RP;
        for (int r = 0; r < R; r++) st_sc1(Vp + r, v_s[lane * LRF_RP + r]);
        if (write_i8) {
            int8_t* vo = V8 + pd.v_off + (long)lane * R;
            for (int r = 0; r < R; r++) vo[r] = (int8_t)v_s[lane * LRF_RP + r];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (!write_i8) {
        // the b table of the new V: into LDS (make_gtable's stores), then out with write-through stores
        float* gt_n = a_s; // a_s is free now
        make_gtable(v_s, 64, R, gt_n, lane, 64);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float* gt_g = Bf + (long)pli * LRF_GT_STRIDE;
        static_assert(LRF_GT_LD % 4 == 0, "the b table goes out in 16-B chunks");
        for (int i = 4 * lane; i < R * LRF_GT_LD; i += 256) st_sc1_x4(gt_g + i, *reinterpret_cast<const u32x4*>(&gt_n[i]));
    }
}


// ranks 9..16: k_vupdate<16>.  lds: a_s [64][16], v_s [64][16], the b' table in the layout mid_ordered_row reads (pitch
// LRF_GTB_LD; 12.5 KB in all).  The ordered chain of a row runs in registers (mid_ordered_row: MKL's single-column order with
// the IEEE division — what gs_row's speculative reciprocal provably reproduces); (R - 1) 64 >= 400: never ATen's native order.
__device__ __forceinline__ void bcdp_vupdate16(const PlaneDesc& pd, int pli, const float* __restrict__ Ppart, const float* __restrict__ Qpart,
                                               float* __restrict__ Vf, float* __restrict__ Bf, int8_t* __restrict__ V8, const GsParams gp,
                                               int write_i8, float* lds, int lane)
{
    float* a_s = lds;
    float* v_s = lds + 64 * LRF_RP;
    float* gt_b = lds + 2 * 64 * LRF_RP; // [R][LRF_GTB_LD]
    const int R = pd.R;
    {
        float acc[16], q[4];
        bcdp_sum16(pd, Ppart, Qpart, lane, acc, q);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            a_s[lane + 64 * j] = acc[j];
            v_s[lane + 64 * j] = ld_sc1(Vf + (long)pli * 64 * LRF_RP + lane + 64 * j);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int idx = lane + 64 * j, jj = idx >> 4, r = idx & 15; // b' entry (jj, r)
            if (jj < R && r < R) {
                if (jj == r) gt_b[r * LRF_GTB_LD + LRF_GTB_DEN] = (q[j] + 0.f) + LRF_EPS;
                else gt_b[r * LRF_GTB_LD + (jj < r ? jj : jj - 1)] = q[j];
            }
        }
    }
    bcdp_wave_sync();
    {
        float a[32], v[32];
#pragma unroll
        for (int j = 0; j < 16; j += 4) {
            const f32x4 va4 = *reinterpret_cast<const f32x4*>(&a_s[lane * LRF_RP + j]);
            const f32x4 vv4 = *reinterpret_cast<const f32x4*>(&v_s[lane * LRF_RP + j]);
#pragma unroll
            for (int i = 0; i < 4; i++) { a[j + i] = va4[i]; v[j + i] = vv4[i]; }
        }
#pragma unroll
        for (int j = 16; j < 32; j++) a[j] = v[j] = 0.f;
        mid_ordered_row(R, a, v, gt_b, gp.lo, gp.hi, std::make_integer_sequence<int, 16>{});
        float* Vp = Vf + (long)pli * 64 * LRF_RP + lane * LRF_RP;
        int8_t* vo = V8 + pd.v_off + (long)lane * R;
#pragma unroll
        for (int r = 0; r < 16; r++)
            if (r < R) {
                v_s[lane * LRF_RP + r] = v[r];
                st_sc1(Vp + r, v[r]);
                if (write_i8) vo[r] = (int8_t)v[r];
            }
    }
    bcdp_wave_sync();
    if (!write_i8) {
        float* gt_n = a_s; // a_s is free now
        make_gtable(v_s, 64, R, gt_n, lane, 64);
        bcdp_wave_sync();
        float* gt_g = Bf + (long)pli * LRF_GT_STRIDE;
        for (int i = lane; i < R * LRF_GT_LD; i += 64) st_sc1(gt_g + i, gt_n[i]);
    }
}

// ranks 17..32: k_vupdate_mid (rank pitch LRF_RPB; only the first 32 columns exist at these ranks).  lds: t_s [64][32] (a',
// then the old V, then the new V: a lane's row is contiguous there, the global tables are read and written element-wise, 128
// contiguous bytes per row pair) and the b' table [R][LRF_GTB_LD]: 16.9 KB.  Elements: lane + 64 m -> (row = e >> 5, col = e & 31).
__device__ __forceinline__ void bcdp_vupdate32(const PlaneDesc& pd, int pli, const float* __restrict__ Ppart, const float* __restrict__ Qpart,
                                               float* __restrict__ Vf, float* __restrict__ Bf, int8_t* __restrict__ V8, const GsParams gp,
                                               int write_i8, float* lds, int lane)
{
    float* t_s = lds;            // [64][32]
    float* gt_b = lds + 64 * 32; // [R][LRF_GTB_LD]
    const int R = pd.R;
    float a[32], v[32];
    {
        float acc[32], q[16];
#pragma unroll
        for (int m = 0; m < 32; m++) acc[m] = 0.f;
#pragma unroll
        for (int m = 0; m < 16; m++) q[m] = 0.f;
        const float* P0 = Ppart + (long)pd.blk0 * 64 * LRF_RPB + (lane >> 5) * LRF_RPB + (lane & 31);
        const float* Q0 = Qpart + (long)pd.blk0 * LRF_RPB * LRF_RPB + (lane >> 5) * LRF_RPB + (lane & 31);
        constexpr int NB = 2; // blocks in flight: 96 registers
        for (int b0 = 0; b0 < pd.nblk; b0 += NB) {
            float pv[NB][32], qv[NB][16];
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const long blk = b0 + k < pd.nblk ? b0 + k : b0;
#pragma unroll
                for (int m = 0; m < 32; m++) pv[k][m] = ld_sc1(P0 + blk * 64 * LRF_RPB + 2 * m * LRF_RPB); // rows 2 m, 2 m + 1
#pragma unroll
                for (int m = 0; m < 16; m++) qv[k][m] = ld_sc1(Q0 + blk * LRF_RPB * LRF_RPB + 2 * m * LRF_RPB);
            }
#pragma unroll
            for (int k = 0; k < NB; k++)
                if (b0 + k < pd.nblk) {
#pragma unroll
                    for (int m = 0; m < 32; m++) acc[m] = (b0 + k == 0) ? pv[k][m] : acc[m] + pv[k][m];
#pragma unroll
                    for (int m = 0; m < 16; m++) q[m] = (b0 + k == 0) ? qv[k][m] : q[m] + qv[k][m];
                }
        }
#pragma unroll
        for (int m = 0; m < 32; m++) t_s[lane + 64 * m] = acc[m];
#pragma unroll
        for (int m = 0; m < 16; m++) {
            const int j = 2 * m + (lane >> 5), r = lane & 31; // b' = U^T U entry (j, r)
            if (j < R && r < R) {
                if (j == r) gt_b[r * LRF_GTB_LD + LRF_GTB_DEN] = (q[m] + 0.f) + LRF_EPS;
                else gt_b[r * LRF_GTB_LD + (j < r ? j : j - 1)] = q[m];
            }
        }
    }
    bcdp_wave_sync();
#pragma unroll
    for (int j = 0; j < 32; j += 4) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(&t_s[lane * 32 + j]);
#pragma unroll
        for (int i = 0; i < 4; i++) a[j + i] = t4[i];
    }
    bcdp_wave_sync();
    {
        const float* Vg = Vf + (long)pli * 64 * LRF_RPB + (lane >> 5) * LRF_RPB + (lane & 31);
        float vv[32];
#pragma unroll
        for (int m = 0; m < 32; m++) vv[m] = ld_sc1(Vg + 2 * m * LRF_RPB);
#pragma unroll
        for (int m = 0; m < 32; m++) t_s[lane + 64 * m] = vv[m];
    }
    bcdp_wave_sync();
#pragma unroll
    for (int j = 0; j < 32; j += 4) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(&t_s[lane * 32 + j]);
#pragma unroll
        for (int i = 0; i < 4; i++) v[j + i] = t4[i];
    }
    mid_ordered_row(R, a, v, gt_b, gp.lo, gp.hi, std::make_integer_sequence<int, 32>{});
    bcdp_wave_sync(); // every lane has read its old row
    {
        int8_t* vo = V8 + pd.v_off + (long)lane * R;
#pragma unroll
        for (int r = 0; r < 32; r++) {
            t_s[lane * 32 + r] = r < R ? v[r] : 0.f;
            if (write_i8 && r < R) vo[r] = (int8_t)v[r];
        }
    }
    bcdp_wave_sync();
    {
        float* Vg = Vf + (long)pli * 64 * LRF_RPB + (lane >> 5) * LRF_RPB + (lane & 31);
        if ((lane & 31) < R) {
#pragma unroll
            for (int m = 0; m < 32; m++) st_sc1(Vg + 2 * m * LRF_RPB, t_s[lane + 64 * m]);
        }
    }
    if (!write_i8) {
        // the b table of the new V (make_gtable_big's arithmetic: one k-ordered fma chain per entry; 64 R R >= 400: never native)
        float* gt_g = Bf + (long)pli * LRF_GTB_STRIDE;
        for (int i = lane; i < R * R; i += 64) {
            const int j = i / R, r = i - j * R;
            float acc = 0.f;
#pragma unroll 8
            for (int k = 0; k < 64; k++) acc = fmaf(t_s[k * 32 + j], t_s[k * 32 + r], acc);
            if (j == r) st_sc1(gt_g + r * LRF_GTB_LD + LRF_GTB_DEN, (acc + 0.f) + LRF_EPS);
            else st_sc1(gt_g + r * LRF_GTB_LD + (j < r ? j : j - 1), acc);
        }
    }
}

// ---- ranks <= 8: both products of the block body on 4x4x1 MFMA blocks, by rank QUAD (ranks 4 q .. 4 q + 3; one quad at R <= 4,
// two at R = 5..8).  v_mfma_f32_4x4x1_16b_f32 is sixteen 4x4 outer products (block = lane >> 2; A: 4x1, i = lane & 3; B: 1x4,
// j = lane & 3; D: register v of lane l = D_block[v][l & 3]); with cbsz:4 abid:T every block takes its A from block T, so
// register v of lane l accumulates A[lane 4 T + v] * B[lane l]: the rank sits on the 4-side, the 64 lanes are 64 rows (x V) or
// 64 columns (X^T u), and every element stays ONE chain of single fmas in ascending k — the order of row_times_v and of the
// 16x16x4 tiles of k_bcd_w, without their padding of the rank to 16 or the 64 R DPP fmas.
template <int T>
__device__ __forceinline__ f32x4 mfma_quad(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, acc, 4, T, 0); }
// a quad operand of a [64][pitch] table held as four registers: op[s], lane l = tab[16 s + (l >> 2)][4 q + (l & 3)]
// acc[c][v] = fma(op[c][k >> 4] (lane 4 (k & 15) + v), x[lane][k], acc[c][v]) for k = 0..63 in order; the NC chains are
// interleaved step by step (two or more: no wait state between dependent MFMAs).  x: the lane's own row of the LDS tile.
// xv: the lane's own row, sixteen 16-B chunks in column order
template <int NC>
__device__ __forceinline__ void regs_times_quads(const f32x4 (&xv)[16], const float (&op)[4][4], f32x4 (&acc)[4])
{
    static_for<64>([&](auto kc) {
        constexpr int k = kc;
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = mfma_quad<(k & 15)>(op[c][k >> 4], xv[k >> 2][k & 3], acc[c]);
    });
}
template <int NC>
__device__ __forceinline__ void row_times_quads(const float* xrow_lds, int g16, const float (&op)[4][4], f32x4 (&acc)[4])
{
    // the sixteen reads go out together, ahead of the MFMAs (left to itself the compiler issues one, waits, and uses it)
    f32x4 xv[16];
    static_for<16>([&](auto Jc) {
        constexpr int J = Jc;
        xv[J] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(xrow_lds) + ((16 * J) ^ g16));
    });
    __builtin_amdgcn_sched_barrier(0);
    regs_times_quads<NC>(xv, op, acc);
}
// accP[q][v] (lane = column n) += u[m][4 q + v] * X[m][n] for the sub-tile's rows m = 0..63 in order.  us: the fp32 u tile
// [64][8]; X[m][n]: one ds_read_b32 at dword 64 m + 4 ((n >> 2) ^ xsw(m)) + (n & 3), a permutation of the row's 64 banks; the
// reads go out sixteen rows ahead of the MFMAs that use them.
template <int Q>
__device__ __forceinline__ void xt_u_quads(const float* Xs, const float* us, int lane, f32x4 (&accP)[2])
{
    float uq[Q][4];
#pragma unroll
    for (int q = 0; q < Q; q++)
#pragma unroll
        for (int s = 0; s < 4; s++) uq[q][s] = us[(16 * s + (lane >> 2)) * 8 + 4 * q + (lane & 3)];
    const char* xb = reinterpret_cast<const char*>(Xs);
    const int l4 = 4 * lane;
    static_for<4>([&](auto sc) {
        constexpr int s = sc;
        float xc[16];
        static_for<16>([&](auto cc) {
            constexpr int c = cc;
            xc[c] = *reinterpret_cast<const float*>(xb + 256 * (16 * s + c) + (l4 ^ (16 * c)));
        });
        static_for<16>([&](auto cc) {
            constexpr int c = cc;
#pragma unroll
            for (int q = 0; q < Q; q++) accP[q] = mfma_quad<c>(uq[q][s], xc[c], accP[q]);
        });
    });
}

// ---- ranks <= 8: one (matrix, 384-row block) on one wave — k_bcd_w<0> (lrf_bcdw_kernel.hip) element for element in the same
// order of operations, a = x V and a' += X^T u on 4x4x1 MFMA blocks (above) instead of the VALU chain and the 16-wide tiles, with
// the V table, the b table, the old int8 rows and the partial tables reached through sc1 accesses.  Xs: the wave's LDS share
// (X tile 16 KB, then the fp32 u tile 2 KB, then the U-span staging area, LRF_BCDP_USTAGE bytes).
// MODE 1 (round 5, k_bcd_p<.., .., true>): the call's FIRST iteration, k_bcd_w<1> — the old U is X @ W0 (the initialisation's
// table Wf, written before the launch), no int8 rows are read.
// BYTES (a luma block of a call that plan_luma_bytes accepted): the sub-tile comes from the caller's image bytes, three bytes an
// element instead of the four of X.  Lane m takes patch m of the sub-tile (luma_patch_byte0, lrf_plan.h): per pixel row and
// channel one 8-byte load, contiguous across the lanes of a patch row, 24 loads a sub-tile (48 registers against xq's 64), in
// flight one sub-tile ahead as xq is.  luma_of on them is k_planes16's arithmetic bit for bit, so the lane holds ROW m of the
// sub-tile in registers: the operand of the x V chain as it stands (no LDS read), and written to the tile's own-row slots —
// the addresses row_times_quads reads, conflict-free for the same reason — for xt_u_quads.  Everything behind the operand is
// the fp32 body's.
template <int MODE, bool BYTES>
__device__ __forceinline__ void bcdp_w_block(const float* __restrict__ X, const LumaSrc& ls, const PlaneDesc& pd, const BlockDesc& bd,
                                             const float* __restrict__ Vf, const float* __restrict__ Wf, const float* __restrict__ Bf,
                                             int8_t* __restrict__ U, float* __restrict__ Ppart, const GsParams& gp, float* Xs, const int lane)
{
    constexpr int RMAX = 8;
    const int li = lane & 15, lq = lane >> 4;
    float* us = Xs + 64 * 64;
    const float* uq = &us[(lq + 4 * (li >> 3)) * RMAX + (li & 7)];
    const float* xrow = &Xs[lane * 64];
    const int g16 = 16 * xsw(lane);
    const int R = pd.R;
    const float* Xp = X + pd.x_off + (long)bd.row0 * 64;
    const float* Vp = Vf + (long)bd.plane * 64 * LRF_RP;
    const float* gt = Bf + (long)bd.plane * LRF_GT_STRIDE;
    int8_t* Ub = U + pd.u_off + (long)bd.row0 * R;
    int nrows = pd.M - bd.row0;
    if (nrows > LRF_KC) nrows = LRF_KC;
    const int nsub = (nrows + 63) >> 6;
    const bool native = pd.native_t2_u != 0;

    // the V table (MODE 1: and W0) as quad operands (row_times_quads): vq[q][s], lane l = V[16 s + (l >> 2)][4 q + (l & 3)], one
    // word per lane out of the 16-B chunk q of that row.  Ranks at or past R are ZERO operands (the tables hold whatever an
    // earlier call of a higher rank left there); the second quad exists at R > 4 only (wave-uniform).
    // The b table: entry tn < 7 of row tr, or its reciprocal denominator (tn = 7), picked out of the 16-B chunk that holds it;
    // the denominator from the chunk at LRF_GT_RDEN
    const bool quads2 = R > 4;
    float vq[2][4], wq[2][4]; // (wq: MODE 1 only)
    {
        const int lr = lane & 3, lrow = lane >> 2;
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int s = 0; s < 4; s++) {
                vq[q][s] = 0.f;
                if (q == 0 || quads2) {
                    const f32x4 v4 = ld_sc1_x4(Vp, ((16 * s + lrow) * LRF_RP + 4 * q) * 4);
                    const float v = lr == 0 ? v4[0] : lr == 1 ? v4[1] : lr == 2 ? v4[2] : v4[3];
                    vq[q][s] = 4 * q + lr < R ? v : 0.f;
                }
                wq[q][s] = 0.f;
                if constexpr (MODE == 1) {
                    if (q == 0 || quads2) {
                        const float w = Wf[((long)bd.plane * 64 + 16 * s + lrow) * LRF_RP + 4 * q + lr];
                        wq[q][s] = 4 * q + lr < R ? w : 0.f;
                    }
                }
            }
    }
    static_assert(LRF_GT_LD % 4 == 0 && LRF_GT_RDEN % 4 == 0 && LRF_GT_DEN == LRF_GT_RDEN + 1, "b-table chunks");
    float tab[5];
    {
        const int tn = li & 7, e = tn < 7 ? (tn & 3) : 0;
        f32x4 t4[5];
#pragma unroll
        for (int j = 0; j < 4; j++) t4[j] = ld_sc1_x4(gt, ((2 * j + (li >> 3)) * LRF_GT_LD + (tn < 7 ? (tn & 4) : LRF_GT_RDEN)) * 4);
        t4[4] = ld_sc1_x4(gt, ((li & 7) * LRF_GT_LD + LRF_GT_RDEN) * 4);
#pragma unroll
        for (int j = 0; j < 4; j++) tab[j] = e == 0 ? t4[j][0] : e == 1 ? t4[j][1] : e == 2 ? t4[j][2] : t4[j][3];
        tab[4] = t4[4][1];
    }

    // The block's X source by cache policy (plan_x_residency, lrf_plan.h; wave-uniform): a streamed block loads non-temporal, so
    // that what it reads once a pass does not push the kept planes' X out of the Infinity Cache; a kept block, and every block
    // of a call without the policy, loads plain.  The policy bit is an immediate of the load: two load sequences, one branch.
    const bool x_nt = bd.x_nt != 0;
    f32x4 xq[4][4];
    auto issue_x_as = [&](auto ntc, int t, int T0, int T1, bool live) {
        constexpr bool NT = ntc;
        const int r0 = t * 64;
#pragma unroll
        for (int T = T0; T < T1; T++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int row = r0 + 16 * T + 4 * q + lq;
                row = row < nrows ? row : nrows - 1;
                const f32x4* src = reinterpret_cast<const f32x4*>(Xp + (long)row * 64 + 4 * li);
                if (live) xq[T][q] = NT ? __builtin_nontemporal_load(src) : *src;
                else xq[T][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    auto issue_x = [&](int t, int T0, int T1, bool live) {
        if (x_nt) issue_x_as(std::true_type{}, t, T0, T1, live);
        else issue_x_as(std::false_type{}, t, T0, T1, live);
    };
    // BYTES: by[ch][j] = the eight bytes of pixel row j of the lane's patch in channel ch.  One buffer resource per image
    // (wave-uniform: the plane index is the image), the patch's first byte as the lane's offset, channel and pixel row as the
    // scalar offset: no address arithmetic per load.  The resource ends with the image: 3 hw records.
    u32x2 by[3][8];
    __amdgpu_buffer_rsrc_t irs;
    if constexpr (BYTES)
        irs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(ls.img + (long)bd.plane * 3 * ls.hw), (short)0, 3 * ls.hw, 0x00020000);
    auto patch0_of = [&](int t) { // rows at or past nrows clamp to the block's last row, as issue_x's
        int row = t * 64 + lane;
        row = row < nrows ? row : nrows - 1;
        return luma_patch_byte0(bd.row0 + row, ls.W, ls.nwl);
    };
    auto issue_b_as = [&](auto ntc, int p0, int j0, int j1) {
        constexpr int AUX = decltype(ntc)::value ? 2 : 0; // (2: nt)
#pragma unroll
        for (int j = j0; j < j1; j++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
                by[ch][j] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(irs, p0, ch * ls.hw + j * ls.W, AUX));
    };
    auto issue_b = [&](int p0, int j0, int j1) {
        if constexpr (BYTES) {
            if (x_nt) issue_b_as(std::true_type{}, p0, j0, j1);
            else issue_b_as(std::false_type{}, p0, j0, j1);
        }
    };
    // int8 U rows as whole spans: the 64 rows of sub-tile t are ONE contiguous span of the wave's own, bytes [a, a + len) with
    // a = Ub + 64 R t.  It passes through the wave's LDS staging area `ust` at the address's phase (span byte i at a % 16 + i),
    // so that 16-B slot k of the staging area is the naturally aligned 16 bytes at (a & ~15) + 16 k; lane k < nslots moves slot k.
    //   old rows: lane k loads slot k with a compiler-tracked 16-B sc1 load one sub-tile ahead (a slot holds a byte of the span:
    //   never past the allocation's last aligned 16 bytes), lands it in staging, and every lane reads its row from there;
    //   new rows: every lane writes its R bytes to staging, and lane k stores the span's bytes of slot k — 16-B sc1 stores, and
    //   at an unaligned head or tail naturally aligned 8/4/2/1-byte sc1 stores that stay INSIDE the span (the bytes beside it
    //   belong to other waves' spans, written at the same time).
    uint8_t* ust = reinterpret_cast<uint8_t*>(Xs + 64 * 64 + 64 * RMAX);
    const uintptr_t uaddr = reinterpret_cast<uintptr_t>(Ub);
    const uint8_t* ub16 = reinterpret_cast<const uint8_t*>(uaddr & ~(uintptr_t)15); // wave-uniform base of the old-row loads
    auto span_of = [&](int t, uintptr_t& a, int& len, int& nsl) {
        a = uaddr + (uintptr_t)(64 * R * t);
        const int nr = nrows - 64 * t;
        len = (nr < 64 ? nr : 64) * R;
        nsl = ((int)(a & 15) + len + 15) >> 4;
    };
    u32x4 uvec;
    int unsl = 0, uph = 0; // the loaded span's slot count and phase
    auto issue_u = [&](int t) {
        uintptr_t a;
        int len;
        span_of(t, a, len, unsl);
        uph = (int)(a & 15);
        const int k = lane < unsl ? lane : unsl - 1;
        uvec = ld_sc1_x4u(ub16, (unsigned)((a & ~(uintptr_t)15) - reinterpret_cast<uintptr_t>(ub16)) + 16 * k);
    };
    auto row_bytes = [&](int ph, unsigned& lo, unsigned& hi) { // the lane's row in staging: bytes 0..3, 4..7 (at or past R: unspecified)
        const int o = ph + lane * R; // <= 15 + 63 * 8: the three aligned dwords end inside the staging area
        const unsigned* w = reinterpret_cast<const unsigned*>(ust + (o & ~3));
        const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
        lo = __builtin_amdgcn_alignbyte(w1, w0, (unsigned)(o & 3));
        hi = __builtin_amdgcn_alignbyte(w2, w1, (unsigned)(o & 3));
    };

    f32x4 accP[2], accQ = (f32x4){0.f, 0.f, 0.f, 0.f}; // accP[q][v], lane n = P[column n][rank 4 q + v]
#pragma unroll
    for (int q = 0; q < 2; q++) accP[q] = (f32x4){0.f, 0.f, 0.f, 0.f};

#ifdef LRF_BCDP_PROBE_3Q // timing experiment only (wrong results): planes below this index request three quarters of every sub-tile
    const bool probe3q = bd.plane < (LRF_BCDP_PROBE_3Q);
#else
    constexpr bool probe3q = false;
#endif
    if constexpr (MODE == 0) issue_u(0);
    if constexpr (BYTES) {
        issue_b(patch0_of(0), 0, 8);
    } else {
        issue_x(0, 0, 3, true);
        if (!probe3q) issue_x(0, 3, 4, true);
    }
    for (int t = 0; t < nsub; t++) {
        const int r0 = t * 64;
        __builtin_amdgcn_sched_barrier(0);
        f32x4 xv[16]; // BYTES: the lane's row, chunk J = pixels 4 (J & 1) .. + 3 of pixel row J >> 1
        if constexpr (BYTES) {
#pragma unroll
            for (int J = 0; J < 16; J++) {
                const unsigned r = by[0][J >> 1][J & 1], g = by[1][J >> 1][J & 1], b = by[2][J >> 1][J & 1];
#pragma unroll
                for (int i = 0; i < 4; i++)
                    xv[J][i] = luma_of((float)((r >> (8 * i)) & 255u), (float)((g >> (8 * i)) & 255u), (float)((b >> (8 * i)) & 255u));
            }
#pragma unroll
            for (int J = 0; J < 16; J++)
                *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(const_cast<float*>(xrow)) + ((16 * J) ^ g16)) = xv[J];
        } else {
#pragma unroll
            for (int T = 0; T < 4; T++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int m = 16 * T + 4 * q + lq;
                    *reinterpret_cast<f32x4*>(&Xs[m * 64 + 4 * (li ^ (4 * q + lq))]) = xq[probe3q && T == 3 ? 2 : T][q]; // (probe: a loaded quarter again)
                }
        }
        float u[RMAX];
        const int row = r0 + lane;
        int cph = 0;
        if constexpr (MODE == 0) {
            if (lane < unsl) *reinterpret_cast<u32x4*>(ust + 16 * lane) = uvec;
            cph = uph;
        }
        const int tn = t + 1;
        const bool more = tn < nsub;
        if constexpr (MODE == 0) {
            if (more) issue_u(tn);
        }
        int p0n = 0; // BYTES: the lane's patch of the next sub-tile
        if constexpr (BYTES) {
            if (more) {
                p0n = patch0_of(tn);
                issue_b(p0n, 0, 4);
            }
        } else
            issue_x(tn, 0, 2, more);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if constexpr (MODE == 0) {
            unsigned lo, hi;
            row_bytes(cph, lo, hi);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                u[r] = (float)(int)(int8_t)(lo >> (8 * r));
                u[4 + r] = (float)(int)(int8_t)(hi >> (8 * r));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // a = x V (MODE 1: and u = x W0) of the lane's row: one chain per quad, the chains of a sub-tile interleaved
        float a[RMAX];
        {
            f32x4 acc[4];
#pragma unroll
            for (int c = 0; c < 4; c++) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            float op[4][4];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                op[0][s] = vq[0][s];
                op[1][s] = vq[1][s];
                op[2][s] = wq[0][s];
                op[3][s] = wq[1][s];
            }
            auto rtq = [&](auto ncc) { // BYTES: the row is in registers already
                constexpr int NC = ncc;
                if constexpr (BYTES) regs_times_quads<NC>(xv, op, acc);
                else row_times_quads<NC>(xrow, g16, op, acc);
            };
            if constexpr (MODE == 0) {
                if (quads2) rtq(std::integral_constant<int, 2>{});
                else rtq(std::integral_constant<int, 1>{});
            } else {
                if (quads2) rtq(std::integral_constant<int, 4>{});
                else {
#pragma unroll
                    for (int s = 0; s < 4; s++) op[1][s] = wq[0][s];
                    rtq(std::integral_constant<int, 2>{});
                    acc[2] = acc[1];
                    acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int v = 0; v < 4; v++) {
                a[v] = acc[0][v];
                a[4 + v] = acc[1][v];
                if constexpr (MODE == 1) {
                    u[v] = acc[2][v];
                    u[4 + v] = acc[3][v];
                }
            }
        }
        if constexpr (BYTES) {
            if (more) issue_b(p0n, 4, 6);
        } else
            issue_x(tn, 2, 3, more);
        __builtin_amdgcn_sched_barrier(0);
        gs_regs_dispatch<RMAX>(R, a, u, tab, native, gp);
        if (row >= nrows) {
#pragma unroll
            for (int r = 0; r < RMAX; r++) u[r] = 0.f;
        }
        if constexpr (BYTES) {
            if (more) issue_b(p0n, 6, 8);
        } else if (!probe3q)
            issue_x(tn, 3, 4, more);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < RMAX; r += 4) *reinterpret_cast<f32x4*>(&us[lane * RMAX + r]) = (f32x4){u[r], u[r + 1], u[r + 2], u[r + 3]};
        // the new row into staging (the old span there has been read: every lane's row_bytes is behind it)
        uintptr_t sa;
        int slen, snsl;
        span_of(t, sa, slen, snsl);
        const int sph = (int)(sa & 15);
        if (row < nrows) {
            uint8_t* d = ust + sph + lane * R;
#pragma unroll
            for (int r = 0; r < RMAX; r++)
                if (r < R) d[r] = (uint8_t)(int)u[r];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < snsl) { // slot `lane` of the span: bytes [lo, hi) of the aligned 16 at s
            const uintptr_t s0 = (sa & ~(uintptr_t)15) + 16 * lane;
            const uint8_t* src = ust + 16 * lane;
            int lo = lane == 0 ? sph : 0;
            const int hi = lane == snsl - 1 ? sph + slen - 16 * lane : 16;
            if (lo == 0 && hi == 16) {
                st_sc1_x4(reinterpret_cast<void*>(s0), *reinterpret_cast<const u32x4*>(src));
            } else {
                while (lo < hi) { // naturally aligned pieces inside [lo, hi)
                    void* dst = reinterpret_cast<void*>(s0 + lo);
                    if ((lo & 7) == 0 && lo + 8 <= hi) {
                        st_sc1_x2(dst, *reinterpret_cast<const u32x2*>(src + lo));
                        lo += 8;
                    } else if ((lo & 3) == 0 && lo + 4 <= hi) {
                        st_sc1_b32(dst, *reinterpret_cast<const unsigned*>(src + lo));
                        lo += 4;
                    } else if ((lo & 1) == 0 && lo + 2 <= hi) {
                        st_sc1_b16(dst, *reinterpret_cast<const uint16_t*>(src + lo));
                        lo += 2;
                    } else {
                        st_sc1_b8(dst, src[lo]);
                        lo += 1;
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // b' += u^T u on its eight 16x16x4 tiles (small integers: exact in any order), a' += X^T u by rank quad
        float qu[8];
#pragma unroll
        for (int h = 0; h < 8; h++) qu[h] = uq[8 * h * RMAX];
#pragma unroll
        for (int h = 0; h < 8; h++) accQ = __builtin_amdgcn_mfma_f32_16x16x4f32(qu[h], qu[h], accQ, 0, 0, 0);
        if (quads2) xt_u_quads<2>(Xs, us, lane, accP);
        else xt_u_quads<1>(Xs, us, lane, accP);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // the dense slot (bcdp_dense_chunks) through the X tile's LDS, which the loop's closing barrier has freed: lane n holds
    // column n of P^T row 4 q + v in accP[q][v]; b' entry (4 lq + reg, li) = mine + other.  Then whole 16-B chunks out,
    // consecutive lanes on consecutive chunks.
    float* ps = Xs;
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
        for (int v = 0; v < 4; v++)
            if (4 * q + v < R) ps[(4 * q + v) * 64 + lane] = accP[q][v];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int i = 4 * lq + reg;
        const float mine = accQ[reg];
        const float other = __shfl(mine, ((lq + 2) & 3) * 16 + ((li + 8) & 15), 64);
        if (i < R && li < R) ps[64 * R + i * R + li] = mine + other;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float* Pp = Ppart + ((long)pd.blk0 + bd.blk) * 64 * LRF_RP;
    const int nch = bcdp_dense_chunks(R);
    for (int c = lane; c < nch; c += 64) st_sc1_x4(Pp + 4 * c, *reinterpret_cast<const u32x4*>(&ps[4 * c]));
}

// F16: planes of ranks 9..16 may occur (w16_block); NP32 > 0: planes of ranks 2 NP32 - 1 / 2 NP32 (17..32) may occur
// (w32_block<NP32>).  t16 / t64: the table sets of the two rank pitches (a call without ranks above 16 has only t16).
// wave_lds: bytes of LDS per wave (the largest share a family of the call needs; the V updates fit the smallest).
// FIRST (round 5; only without ranks above 16): item iteration 0 is the call's FIRST iteration — the bodies of k_bcd_w<1> /
// k_bcd_w16<1>, old U = X @ W0 from the initialisation's tables, which are complete before the launch: no flag to wait for —,
// so that the launch covers all K iterations and the call has no U-update or V-update launch of its own.
template <bool F16, int NP32, bool FIRST = false>
__global__ __launch_bounds__(64 * LRF_BCDW_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_bcd_p(
    const float* __restrict__ X, const PlaneDesc* __restrict__ planes, const BlockDesc* __restrict__ blocks, const BcdpTabs t16,
    const BcdpTabs t64, int8_t* __restrict__ U, int8_t* __restrict__ V8, GsParams gp, int nblocks, int niter, int nplanes, int plane0,
    BcdpSync* sync, int* err_host, int ncells, int seq, int wave_lds, const LumaSrc ls)
{
    extern __shared__ __attribute__((aligned(16))) float bcdp_lds[]; // LRF_BCDW_WAVES x wave_lds bytes
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    float* Xs = reinterpret_cast<float*>(reinterpret_cast<char*>(bcdp_lds) + wave * wave_lds);
    int* ticket = sync->cell;
    int* flag = sync->cell + nplanes;
    const int total = niter * nblocks;
    // leaving: the wave's own stores to the flags have landed before it is counted; the last one out zeroes the state
    auto leave = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int l = 0;
        if (lane == 0) l = __hip_atomic_fetch_add(&sync->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int d = __builtin_amdgcn_readfirstlane(__shfl(l, 0, 64));
        if (d == (int)(gridDim.x * LRF_BCDW_WAVES) - 1) {
            for (int i = lane; i < ncells; i += 64) __hip_atomic_store(&sync->cell[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sync->head, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sync->done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };

    // a launch queued behind a failed one: the queue state is dirty (head past the end, tickets of the failed launch): nothing
    // here may run on it.  The host word already names the first failed launch; this one is invalid by its sequence number.
    if (__hip_atomic_load(&sync->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    for (;;) {
        // lane 0 pulls, EVERY lane then holds lane 0's value (an explicit lane-0 broadcast: with `readfirstlane` of a variable
        // that is 0 in the other lanes the compiler's control flow let lanes 1..63 go on with item 0 after lane 0 had left)
        int idx_l = 0;
        if (lane == 0) idx_l = __hip_atomic_fetch_add(&sync->head, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int idx = __builtin_amdgcn_readfirstlane(__shfl(idx_l, 0, 64));
        if (idx >= total) {
            leave();
            return;
        }
        // (iteration-major, the blocks of an iteration in table order.  Tried and not kept, round 5: the rank families of a call
        // interleaved within an iteration — luma blocks beside chroma blocks on a SIMD: within noise —, and chunks of ~86 images
        // (2064 blocks, 200 MB of X) running all their iterations before the next chunk, so that X stays in the 256 MB Infinity
        // Cache: 139 -> 164 us per iteration at (7,3,3), 246 -> 353 at (26,13,13): a chunk is barely one round of the resident
        // waves, so blocks poll for V tables that are still being computed.  That experiment moved all of X and added the
        // polling, so it says nothing about the cache by itself; what the kernel does follow is how its X loads land: the
        // streamed sources loaded non-temporal took 7 % off the launch in this order — plan_x_residency)
        const int it = idx / nblocks, blk = idx - it * nblocks;
#ifdef LRF_BCDP_DEBUG
        atomicAdd(&sync->cell[2 * nplanes + blk], 1 + 1000 * it); // every active lane
#endif
        const BlockDesc bd = blocks[blk];
        const PlaneDesc pd = planes[bd.plane];
        const int pl = bd.plane - plane0; // index into the tickets / flags
        if (it > 0) { // the V update of (matrix, it - 1) must have been published
            int polls = 0;
            while (__hip_atomic_load(&flag[pl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < it) {
                __builtin_amdgcn_s_sleep(8);
                if (++polls > LRF_BCDP_MAX_POLLS) { // (the state stays dirty: the host sees the error word and zeroes it)
                    __hip_atomic_store(&sync->err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(err_host, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    return;
                }
            }
        }
        // nothing below may move above the poll: the hardware path is the sc1 loads behind the flag (MI355X_MICROARCH.md,
        // inter-workgroup visibility, first row of the sc1 table); this pins the compiler to the same order (relaxed atomics
        // to different addresses are not ordered among themselves by the memory model)
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        asm volatile("" ::: "memory");
#ifdef LRF_BCDP_FENCES
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        // the block, by the rank family of its plane (wave-uniform).  `ln` is the lane number behind an opaque move: left
        // visible as loop-invariant, the per-lane LDS addresses of EVERY family's body are hoisted out of the item loop and
        // stay live across the other families' bodies (15-25 registers: <true, 0> spilled 89 registers, the V operand of
        // w16_block's MFMAs among them, reloaded at every use)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int fam = (!F16 || pd.R <= 8) ? 0 : ((NP32 == 0 || pd.R <= 16) ? 1 : 2);
        static_assert(!FIRST || NP32 == 0, "the first iteration of ranks 17..32 stays a launch of its own (k_bcd_w32f)");
        const bool first = FIRST && it == 0; // wave-uniform
        if (fam == 0) {
            // a luma block of a call that reads luma from the image bytes (wave-uniform; only <false, 0, true> carries that body:
            // plan_luma_bytes)
            constexpr bool kBytes = FIRST && !F16 && NP32 == 0;
            bool bytes = false;
            if constexpr (kBytes) bytes = bd.plane < ls.nluma;
            if (first) {
                if constexpr (FIRST) {
                    if constexpr (kBytes) {
                        if (bytes) bcdp_w_block<1, true>(X, ls, pd, bd, t16.vf, t16.wf, t16.bf, U, t16.pp, gp, Xs, ln);
                    }
                    if (!bytes) bcdp_w_block<1, false>(X, ls, pd, bd, t16.vf, t16.wf, t16.bf, U, t16.pp, gp, Xs, ln);
                }
            } else {
                if constexpr (kBytes) {
                    if (bytes) bcdp_w_block<0, true>(X, ls, pd, bd, t16.vf, nullptr, t16.bf, U, t16.pp, gp, Xs, ln);
                }
                if (!bytes) bcdp_w_block<0, false>(X, ls, pd, bd, t16.vf, nullptr, t16.bf, U, t16.pp, gp, Xs, ln);
            }
        }
        if constexpr (F16) {
            if (fam == 1) {
                if (first) {
                    if constexpr (FIRST) w16_block<1, MemSc1>(X, pd, bd, t16.vf, t16.wf, t16.bf, U, t16.pp, t16.qp, gp, Xs, ln);
                } else
                    w16_block<0, MemSc1>(X, pd, bd, t16.vf, nullptr, t16.bf, U, t16.pp, t16.qp, gp, Xs, ln);
            }
        }
        if constexpr (NP32 > 0) {
            if (fam == 2) w32_block<NP32, MemSc1>(X, pd, bd, t64.vf, t64.bf, U, t64.pp, t64.qp, gp, Xs, ln, 0);
        }
        // every store of this wave has left (write-through) before it is counted
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef LRF_BCDP_FENCES
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        int arrived_l = 0;
        if (lane == 0) arrived_l = __hip_atomic_fetch_add(&ticket[pl], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int arrived = __builtin_amdgcn_readfirstlane(__shfl(arrived_l, 0, 64));
        __atomic_signal_fence(__ATOMIC_SEQ_CST); // the partial loads of the V update stay behind the returned ticket
        asm volatile("" ::: "memory");
        if (arrived == (it + 1) * pd.nblk - 1) { // the last block of (matrix, iteration): its V update
#ifdef LRF_BCDP_FENCES
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            const int last = it == niter - 1 ? 1 : 0;
            int lv = lane;
            asm volatile("" : "+v"(lv)); // (as `ln` above)
            if (fam == 0) bcdp_vupdate(pd, bd.plane, t16.pp, t16.vf, t16.bf, V8, gp, last, Xs, lv);
            if constexpr (F16) {
                if (fam == 1) bcdp_vupdate16(pd, bd.plane, t16.pp, t16.qp, t16.vf, t16.bf, V8, gp, last, Xs, lv);
            }
            if constexpr (NP32 > 0) {
                if (fam == 2) bcdp_vupdate32(pd, bd.plane, t64.pp, t64.qp, t64.vf, t64.bf, V8, gp, last, Xs, lv);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef LRF_BCDP_FENCES
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            // every lane stores the same word (no `if (lane == 0)` here: followed by the loop head's `if (lane == 0)` pull it let
            // the compiler thread lane 0 through both and retire it from the loop alone — lanes 1..63 then went on with item 0)
#ifdef LRF_BCDP_TEST_SKIP_FLAG // tests/test_persist_error.py, tools/dev_persist_expiry.py: in a call of FOUR iterations matrix 0 never
                               // publishes its first V update, its later blocks' polls expire; other calls of that build work
            if (!(pl == 0 && it == (FIRST ? 1 : 0) && niter == (FIRST ? 4 : 3)))
#endif
            __hip_atomic_store(&flag[pl], it + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
