// lrf_inflate_shared.h — the inflate of ONE zlib stream (RFC 1950 around RFC 1951) into one factor column, as plain C++ that
// compiles as host code (lrf_pack.cpp: lrf_pack_inflate_column_i8, the CPU-testable definition) and as device code
// (lrf_inflate_kernel.hip, one lane per stream).  Both include this file and nothing else decides a byte or a status, so the
// two cannot drift apart.  No library calls, no arrays on the stack (the device build must not spill to scratch).
//
// What is read: any sequence of stored, fixed and dynamic blocks, matches up to distance 32,768, the Adler-32; bytes behind
// the Adler-32 are ignored.  The output must be exactly `rows` bytes.  The rules of refusal are zlib's own (inflate.c,
// inftrees.c of a default build, whose zlib.decompress this routine follows case by case):
//   header        CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0, FDICT clear
//   code sets     over-subscribed sets are refused; an incomplete set only when it is not a single code of one bit (the
//                 code-length code may never be incomplete); a set with no code at all builds, and decoding from it fails
//   dynamic       HLIT <= 286, HDIST <= 30, a repeat needs a length before it and may not run past HLIT + HDIST, symbol 256
//                 needs a code
//   symbols       286 / 287 (fixed code only) and distance symbols 30 / 31 are refused, as is a distance before the output's start
// The window size CINFO names is not enforced (zlib enforces it only under INFLATE_STRICT).
//
// Tables: per stream LRFI_TAB_N 16-bit entries, reached through lrfi_tab so that the kernel can keep them in LDS, one lane's
// entry i at [i * 64 + lane], and the host in a plain array:
//   CNT_LIT, CNT_DIST   codes per length 0..15 of the literal/length and the distance code (canonical decoding)
//   SYM_LIT, SYM_DIST   the symbols in canonical order
//   FAST                the literal/length codes of at most LRFI_FAST_BITS bits, indexed by the next bits: (symbol << 4) | length,
//                       0 = a longer code (decoded bit by bit from CNT / SYM).  While a dynamic header is read the same entries
//                       hold the 320 code lengths, four bits each (80 entries), and the running offsets per length (16 entries);
//                       the code-length code itself borrows CNT_DIST / SYM_DIST, which are built after it has done its work.
//
// Every loop consumes input bits or produces output; on top of that an iteration count capped at 8 src_len + rows + 64 ends
// the routine with LRFI_E_CAP.  No byte outside [src, src + src_len) is read and nothing outside dst[0 .. rows - 1] (strided)
// is written, whatever the stream holds.  After an error the column's content is unspecified.
#ifndef LRF_INFLATE_SHARED_H
#define LRF_INFLATE_SHARED_H
#include <stdint.h>

#include "../../include/lrf_hip.h" // LRFI_E_*

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LRFI_HD __host__ __device__
#else
#define LRFI_HD
#endif

#define LRFI_FAST_BITS 7
#define LRFI_CNT_LIT 0
#define LRFI_CNT_DIST 16
#define LRFI_SYM_LIT 32
#define LRFI_SYM_DIST 320
#define LRFI_FAST 352
#define LRFI_TAB_N (LRFI_FAST + (1 << LRFI_FAST_BITS)) // 480
#define LRFI_LENS LRFI_FAST                            // 80 entries: 320 lengths of four bits
#define LRFI_OFFS (LRFI_FAST + 80)                     // 16 entries
#define LRFI_ADLER 65521u
#define LRFI_MAX_ROWS (1ll << 30)
static_assert(LRFI_OFFS + 16 <= LRFI_TAB_N, "the header's work area lies inside the fast table");

struct lrfi_tab {
    uint16_t* p;
    int stride; // entries between two of this stream's entries (host: 1; kernel: 64, the lanes interleaved)
    LRFI_HD uint16_t ld(int i) const { return p[i * stride]; }
    LRFI_HD void st(int i, uint32_t v) const { p[i * stride] = (uint16_t)v; }
};

struct lrfi_bits {
    const uint8_t* src;
    int64_t len, pos;
    uint64_t buf;
    int cnt;
};
// up to 57..64 bits in the buffer, never a byte from behind the stream
LRFI_HD inline void lrfi_refill(lrfi_bits& b)
{
    while (b.cnt <= 56 && b.pos < b.len) {
        b.buf |= (uint64_t)b.src[b.pos++] << b.cnt;
        b.cnt += 8;
    }
}
// n <= 32 bits into v; false: the input is exhausted
LRFI_HD inline bool lrfi_take(lrfi_bits& b, int n, uint32_t& v)
{
    if (b.cnt < n) {
        lrfi_refill(b);
        if (b.cnt < n) return false;
    }
    v = (uint32_t)(b.buf & ((1ull << n) - 1ull));
    b.buf >>= n;
    b.cnt -= n;
    return true;
}

LRFI_HD inline int lrfi_get_len(const lrfi_tab& t, int s) { return (t.ld(LRFI_LENS + (s >> 2)) >> (4 * (s & 3))) & 15; }
LRFI_HD inline void lrfi_set_len(const lrfi_tab& t, int s, int v)
{
    const int sh = 4 * (s & 3);
    t.st(LRFI_LENS + (s >> 2), (uint32_t)((t.ld(LRFI_LENS + (s >> 2)) & ~(15u << sh)) | ((uint32_t)v << sh)));
}
// position i of the code-length code's transmission order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (five bits each)
LRFI_HD inline int lrfi_order(int i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// Counts per length and the symbols in canonical order of the n symbols whose lengths L(s) gives; zlib's rule on incomplete
// sets (allow_single: a lone code of one bit passes).  Uses LRFI_OFFS.
template <class LenOf>
LRFI_HD inline int lrfi_build(const lrfi_tab& t, int cnt, int sym, int n, bool allow_single, LenOf L)
{
    for (int l = 0; l < 16; l++) t.st(cnt + l, 0);
    for (int s = 0; s < n; s++) {
        const int l = L(s);
        t.st(cnt + l, t.ld(cnt + l) + 1u);
    }
    int left = 1, maxl = 0, off = 0;
    for (int l = 1; l < 16; l++) {
        const int c = t.ld(cnt + l);
        left = (left << 1) - c;
        if (left < 0) return LRFI_E_OVERSUB;
        if (c) maxl = l;
        t.st(LRFI_OFFS + l, (uint32_t)off);
        off += c;
    }
    if (left > 0 && maxl != 0 && !(allow_single && maxl == 1)) return LRFI_E_INCOMPLETE;
    for (int s = 0; s < n; s++) {
        const int l = L(s);
        if (l) {
            const int o = t.ld(LRFI_OFFS + l);
            t.st(sym + o, (uint32_t)s);
            t.st(LRFI_OFFS + l, (uint32_t)o + 1u);
        }
    }
    return 0;
}

// the literal/length codes of at most LRFI_FAST_BITS bits into FAST (overwrites the header's work area)
LRFI_HD inline void lrfi_build_fast(const lrfi_tab& t)
{
    for (int i = 0; i < (1 << LRFI_FAST_BITS); i++) t.st(LRFI_FAST + i, 0);
    uint32_t code = 0;
    int idx = 0;
    for (int l = 1; l <= LRFI_FAST_BITS; l++) {
        const int c = t.ld(LRFI_CNT_LIT + l);
        for (int k = 0; k < c; k++, code++) {
            const uint32_t s = t.ld(LRFI_SYM_LIT + idx++);
            uint32_t rev = 0;
            for (int i = 0; i < l; i++) rev |= ((code >> i) & 1u) << (l - 1 - i);
            for (uint32_t j = rev; j < (1u << LRFI_FAST_BITS); j += 1u << l) t.st(LRFI_FAST + (int)j, (s << 4) | (uint32_t)l);
        }
        code <<= 1;
    }
}

// One symbol, bit by bit, from the canonical counts: >= 0 the symbol, < 0 a status.  The caller has refilled the buffer.
LRFI_HD inline int lrfi_decode(lrfi_bits& b, const lrfi_tab& t, int cnt, int sym)
{
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        if (b.cnt < 1) {
            lrfi_refill(b);
            if (b.cnt < 1) return -LRFI_E_INPUT;
        }
        code |= (int)(b.buf & 1u);
        b.buf >>= 1;
        b.cnt--;
        const int c = t.ld(cnt + l);
        if (code - c < first) return t.ld(sym + index + (code - first));
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -LRFI_E_CODE;
}

#define LRFI_TRY_TAKE(n, v) \
    do { if (!lrfi_take(b, (n), (v))) return LRFI_E_INPUT; } while (0)

// Inflates the zlib stream src[0 .. src_len - 1] into exactly `rows` elements dst[0], dst[stride], ...; 0 or LRFI_E_*.
// tab: LRFI_TAB_N entries of this stream's own.  max_dist (may be null): the largest match distance seen.
LRFI_HD inline int lrfi_inflate(const uint8_t* src, int64_t src_len, int8_t* dst, int64_t rows, int64_t stride, const lrfi_tab& t, int64_t* max_dist)
{
    if (src_len < 0 || rows < 1 || rows > LRFI_MAX_ROWS) return LRFI_E_OVERRUN;
    lrfi_bits b = {src, src_len, 0, 0, 0};
    uint32_t v = 0, cmf = 0, flg = 0;
    LRFI_TRY_TAKE(8, cmf);
    LRFI_TRY_TAKE(8, flg);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u || (flg & 0x20u)) return LRFI_E_HEADER;
    const uint64_t cap = 8ull * (uint64_t)src_len + (uint64_t)rows + 64ull;
    uint64_t it = 0;
    int64_t n = 0, far = 0;
    uint32_t a = 1, bsum = 0; // Adler-32 of what has been written
    uint32_t last = 0;
    do {
        uint32_t type = 0;
        if (++it > cap) return LRFI_E_CAP;
        LRFI_TRY_TAKE(1, last);
        LRFI_TRY_TAKE(2, type);
        if (type == 3) return LRFI_E_BTYPE;
        if (type == 0) {
            uint32_t lens = 0;
            b.buf >>= b.cnt & 7;
            b.cnt -= b.cnt & 7;
            LRFI_TRY_TAKE(32, lens);
            if ((lens & 0xffffu) != ((lens >> 16) ^ 0xffffu)) return LRFI_E_STORED;
            const int64_t len = (int64_t)(lens & 0xffffu);
            b.pos -= b.cnt >> 3; // whole bytes only are left in the buffer: hand them back
            b.buf = 0;
            b.cnt = 0;
            if (len > src_len - b.pos) return LRFI_E_INPUT;
            if (len > rows - n) return LRFI_E_OVERRUN;
            for (int64_t k = 0; k < len; k++) {
                const uint32_t d = src[b.pos++];
                dst[n++ * stride] = (int8_t)d;
                a += d; if (a >= LRFI_ADLER) a -= LRFI_ADLER;
                bsum += a; if (bsum >= LRFI_ADLER) bsum -= LRFI_ADLER;
            }
            it += (uint64_t)len;
            continue;
        }
        int nlen = 288, ndist = 32;
        for (int i = 0; i < 80; i++) t.st(LRFI_LENS + i, 0);
        if (type == 1) {
            for (int s = 0; s < 288; s++) lrfi_set_len(t, s, s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (int s = 0; s < 32; s++) lrfi_set_len(t, 288 + s, 5);
        } else {
            uint32_t hlit = 0, hdist = 0, hclen = 0;
            LRFI_TRY_TAKE(5, hlit);
            LRFI_TRY_TAKE(5, hdist);
            LRFI_TRY_TAKE(4, hclen);
            nlen = (int)hlit + 257;
            ndist = (int)hdist + 1;
            const int ncode = (int)hclen + 4;
            if (nlen > 286 || ndist > 30) return LRFI_E_COUNTS;
            uint64_t cl = 0; // the 19 lengths of the code-length code, three bits each
            for (int i = 0; i < ncode; i++) {
                LRFI_TRY_TAKE(3, v);
                cl |= (uint64_t)v << (3 * lrfi_order(i));
            }
            int rc = lrfi_build(t, LRFI_CNT_DIST, LRFI_SYM_DIST, 19, false, [cl](int s) { return (int)((cl >> (3 * s)) & 7); });
            if (rc) return rc;
            int have = 0, prev = 0;
            while (have < nlen + ndist) {
                if (++it > cap) return LRFI_E_CAP;
                lrfi_refill(b);
                const int s = lrfi_decode(b, t, LRFI_CNT_DIST, LRFI_SYM_DIST);
                if (s < 0) return -s;
                if (s < 16) {
                    lrfi_set_len(t, have++, s);
                    prev = s;
                    continue;
                }
                int rep, val = 0;
                if (s == 16) {
                    if (have == 0) return LRFI_E_REPEAT;
                    val = prev;
                    LRFI_TRY_TAKE(2, v);
                    rep = 3 + (int)v;
                } else if (s == 17) {
                    LRFI_TRY_TAKE(3, v);
                    rep = 3 + (int)v;
                } else {
                    LRFI_TRY_TAKE(7, v);
                    rep = 11 + (int)v;
                }
                if (have + rep > nlen + ndist) return LRFI_E_REPEAT;
                for (; rep > 0; rep--) lrfi_set_len(t, have++, val);
                prev = val;
            }
            if (lrfi_get_len(t, 256) == 0) return LRFI_E_NOEOB;
        }
        {
            int rc = lrfi_build(t, LRFI_CNT_LIT, LRFI_SYM_LIT, nlen, true, [&t](int s) { return lrfi_get_len(t, s); });
            if (rc) return rc;
            rc = lrfi_build(t, LRFI_CNT_DIST, LRFI_SYM_DIST, ndist, true, [&t, nlen](int s) { return lrfi_get_len(t, nlen + s); });
            if (rc) return rc;
            lrfi_build_fast(t);
        }
        for (;;) {
            if (++it > cap) return LRFI_E_CAP;
            lrfi_refill(b); // >= 57 bits unless the stream ends: a whole length/distance pair (48 bits at most) is in the buffer
            int s;
            const uint32_t e = t.ld(LRFI_FAST + (int)(b.buf & ((1u << LRFI_FAST_BITS) - 1u)));
            if (e & 15u) {
                const int l = (int)(e & 15u);
                if (l > b.cnt) return LRFI_E_INPUT;
                b.buf >>= l;
                b.cnt -= l;
                s = (int)(e >> 4);
            } else {
                s = lrfi_decode(b, t, LRFI_CNT_LIT, LRFI_SYM_LIT);
                if (s < 0) return -s;
            }
            if (s < 256) {
                if (n >= rows) return LRFI_E_OVERRUN;
                dst[n++ * stride] = (int8_t)s;
                a += (uint32_t)s; if (a >= LRFI_ADLER) a -= LRFI_ADLER;
                bsum += a; if (bsum >= LRFI_ADLER) bsum -= LRFI_ADLER;
                continue;
            }
            if (s == 256) break;
            if (s > 285) return LRFI_E_LENSYM;
            // lengths 3..258: symbols 257..264 one each, then four symbols per number of extra bits, 285 is 258
            int len = s - 254;
            if (s >= 265 && s < 285) {
                const int eb = (s - 261) >> 2;
                LRFI_TRY_TAKE(eb, v);
                len = 3 + ((4 + ((s - 261) & 3)) << eb) + (int)v;
            } else if (s == 285) {
                len = 258;
            }
            const int ds = lrfi_decode(b, t, LRFI_CNT_DIST, LRFI_SYM_DIST);
            if (ds < 0) return -ds;
            if (ds > 29) return LRFI_E_DISTSYM;
            int64_t dist = ds + 1;
            if (ds >= 4) {
                const int eb = (ds >> 1) - 1;
                LRFI_TRY_TAKE(eb, v);
                dist = 1 + ((int64_t)(2 + (ds & 1)) << eb) + (int64_t)v;
            }
            if (dist > n) return LRFI_E_FAR;
            if (len > rows - n) return LRFI_E_OVERRUN;
            if (dist > far) far = dist;
            for (int k = 0; k < len; k++, n++) { // the column's own earlier output; distance < length repeats it
                const int8_t d8 = dst[(n - dist) * stride];
                dst[n * stride] = d8;
                a += (uint32_t)(uint8_t)d8; if (a >= LRFI_ADLER) a -= LRFI_ADLER;
                bsum += a; if (bsum >= LRFI_ADLER) bsum -= LRFI_ADLER;
            }
            it += (uint64_t)len;
        }
    } while (!last);
    if (n != rows) return LRFI_E_SHORT;
    b.buf >>= b.cnt & 7;
    b.cnt -= b.cnt & 7;
    uint32_t want = 0;
    for (int i = 0; i < 4; i++) {
        LRFI_TRY_TAKE(8, v);
        want = (want << 8) | v;
    }
    if (want != ((bsum << 16) | a)) return LRFI_E_ADLER;
    if (max_dist) *max_dist = far;
    return 0;
}
#undef LRFI_TRY_TAKE
#endif
