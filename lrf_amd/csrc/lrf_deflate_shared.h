// lrf_deflate_shared.h — the Huffman-only deflate coder of factor columns: everything that decides a stream's bytes, as plain
// C++ that compiles as host code (lrf_pack.cpp: lrf_pack_deflate_column_i8, the CPU-testable definition) and as device code
// (lrf_deflate_kernel.hip; lrf_deflate_sizes_kernel.hip counts a stream's bytes without writing it).  All include this file and
// nothing else decides a byte or a size, so they cannot drift apart.
//
// The stream (RFC 1950 around RFC 1951) of one column of `rows` bytes:
//   header   0x78 0x01
//   blocks   one of three forms, all final:
//              DYNAMIC  one BTYPE 2 block of literals and the end-of-block symbol: HLIT = 257 codes (symbols 0..256),
//                       HDIST = 1 distance code of length 0 (no distances at all)
//              FIXED    one BTYPE 1 block
//              STORED   BTYPE 0 blocks of at most 65,535 bytes, as many as the length needs
//   trailer  Adler-32, big-endian
// Choice of form: the smallest total byte count; on equal counts STORED before FIXED before DYNAMIC (the cheaper one to write
// and to read).  The counts are exact and known before a byte is written (lrfd_measure, the first half of lrfd_plan).
//
// Code lengths (literals: at most 15 bits; the code-length alphabet: at most 7) come from one builder, lrfd_code_lengths:
//   1. the used symbols in ascending (count, symbol) order — a strict order, so the sorting method cannot matter
//   2. Huffman lengths by Moffat and Katajainen's in-place minimum-redundancy calculation on the sorted counts
//   3. fix-up when a length exceeds the limit: lengths above the limit are set to it, then, while the Kraft sum (in units of
//      2^-limit) exceeds 1, one code of the limit is taken away and the longest code below the limit is split into two
//      codes one bit longer (each step lowers the sum by exactly one unit, so it ends at exactly 1)
//   4. the lengths, longest first, go to the symbols in that ascending order
//   one used symbol gets length 1 (does not occur in a stream: the end-of-block symbol is always a second one).
// Codes are canonical (RFC 1951 3.2.2).  The 258 lengths (257 literal lengths and the distance length 0) are run-length coded
// as ONE sequence by this greedy rule, runs taken left to right:
//   a run of n zeros:      while n >= 11: symbol 18 for min(n, 138);  then if n >= 3: symbol 17 for n;  else n single zeros
//   a run of n lengths v:  v itself once; while the rest is >= 3: symbol 16 for min(rest, 6);  then the rest as single v
// HCLEN drops trailing zero lengths in the RFC's order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, never below 4.
#ifndef LRF_DEFLATE_SHARED_H
#define LRF_DEFLATE_SHARED_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LRFD_HD __host__ __device__
#else
#define LRFD_HD
#endif

#define LRFD_T 2048           // symbols of a column per tile (the kernel's unit of work; the host restatement has no use for it)
#define LRFD_NLIT 257         // literals 0..255 and end-of-block
#define LRFD_NSEQ 258         // code lengths sent: the literals' and one distance length
#define LRFD_LIT_LIMIT 15
#define LRFD_CL_LIMIT 7
#define LRFD_HDR_MAX 256      // bytes: 16 + 3 + 14 + 19 * 3 + 258 * 7 bits = 1896 bits at most before the first literal
#define LRFD_STORED_MAX 65535 // bytes of one stored block
#define LRFD_ADLER 65521u
#define LRFD_MAX_ROWS (1ll << 30)
enum { LRFD_DYNAMIC = 0, LRFD_FIXED = 1, LRFD_STORED = 2 };

// what one column's plan needs and gives; the kernel keeps one per workgroup in LDS
struct lrfd_work {
    uint32_t freq[LRFD_NLIT];  // in: counts of the column's bytes, freq[256] = 1
    uint32_t w[LRFD_NLIT];     // scratch of the builder
    uint16_t sym[LRFD_NLIT];   // scratch of the builder
    uint16_t code[LRFD_NLIT];  // out: the codes, bit-reversed (ready to be OR-ed in LSB first); DYNAMIC and FIXED
    uint8_t len[LRFD_NLIT];    // out: their lengths
    uint8_t seq[LRFD_NSEQ];    // the run-length coded sequence: symbols of the code-length alphabet ...
    uint8_t ext[LRFD_NSEQ];    // ... and the value of each one's extra bits
    int32_t form;              // out: LRFD_DYNAMIC / LRFD_FIXED / LRFD_STORED
    uint32_t hdr_bits;         // out: bits of the stream in front of the first literal (zlib header included); STORED: 16
    int64_t stream_len;        // out: bytes of the whole stream
};

// what a caller that only counts keeps per column (lrfd_measure): 3,085 bytes instead of lrfd_work's 3,880
struct lrfd_count {
    uint32_t freq[LRFD_NLIT]; // in: counts of the column's bytes, freq[256] = 1
    uint32_t w[LRFD_NLIT];    // scratch of the builder
    uint16_t sym[LRFD_NLIT];  // scratch of the builder
    uint8_t len[LRFD_NLIT];   // the literals' code lengths
    uint8_t seq[LRFD_NSEQ];   // the run-length coded sequence (symbols only)
};

LRFD_HD inline int64_t lrfd_bound(int64_t len) { return 2 + 5 * ((len + LRFD_STORED_MAX - 1) / LRFD_STORED_MAX) + len + 4; }

// byte position of the column's byte i in a STORED stream
LRFD_HD inline int64_t lrfd_stored_pos(int64_t i) { return 2 + 5 * (i / LRFD_STORED_MAX + 1) + i; }

// the five bytes in front of stored block k of a column of `rows` bytes
LRFD_HD inline void lrfd_stored_block_header(int64_t rows, int64_t k, uint8_t h[5])
{
    const int64_t nblocks = (rows + LRFD_STORED_MAX - 1) / LRFD_STORED_MAX;
    const uint32_t n = (uint32_t)(k + 1 < nblocks ? LRFD_STORED_MAX : rows - k * LRFD_STORED_MAX);
    h[0] = k + 1 == nblocks ? 1 : 0; // BFINAL, BTYPE 0, padding
    h[1] = (uint8_t)(n & 0xff);
    h[2] = (uint8_t)(n >> 8);
    h[3] = (uint8_t)(~n & 0xff);
    h[4] = (uint8_t)((~n >> 8) & 0xff);
}

// ORs the low n bits of v into a zeroed byte buffer at bit position pos (LSB first, as deflate packs bits)
LRFD_HD inline void lrfd_put_bits(uint8_t* buf, uint64_t pos, uint32_t v, int n)
{
    uint64_t x = (uint64_t)(v & ((1u << n) - 1u)) << (pos & 7);
    for (uint64_t b = pos >> 3; x; b++, x >>= 8) buf[b] |= (uint8_t)(x & 0xff);
}

LRFD_HD inline uint32_t lrfd_reverse(uint32_t code, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++) r |= ((code >> i) & 1u) << (n - 1 - i);
    return r;
}

// Code lengths of n symbols with counts freq[] under `limit` bits (the rule at the top).  sym, w: scratch of n entries.
LRFD_HD inline void lrfd_code_lengths(const uint32_t* freq, int n, int limit, uint8_t* len, uint16_t* sym, uint32_t* w)
{
    int m = 0;
    for (int s = 0; s < n; s++) {
        len[s] = 0;
        if (freq[s]) sym[m++] = (uint16_t)s;
    }
    if (m == 0) return;
    if (m == 1) { len[sym[0]] = 1; return; }
    // 1. ascending (count, symbol): Shell sort
    const int gaps[6] = {132, 57, 23, 10, 4, 1};
    for (int gi = 0; gi < 6; gi++) {
        const int gap = gaps[gi];
        for (int i = gap; i < m; i++) {
            const uint16_t s = sym[i];
            const uint32_t f = freq[s];
            int j = i;
            while (j >= gap && (freq[sym[j - gap]] > f || (freq[sym[j - gap]] == f && sym[j - gap] > s))) {
                sym[j] = sym[j - gap];
                j -= gap;
            }
            sym[j] = s;
        }
    }
    for (int i = 0; i < m; i++) w[i] = freq[sym[i]];
    // 2. Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": w[i] becomes the depth of leaf i
    {
        int root, leaf, next, avbl, used, dpth;
        w[0] += w[1];
        root = 0;
        leaf = 2;
        for (next = 1; next < m - 1; next++) {
            if (leaf >= m || w[root] < w[leaf]) { w[next] = w[root]; w[root++] = (uint32_t)next; }
            else w[next] = w[leaf++];
            if (leaf >= m || (root < next && w[root] < w[leaf])) { w[next] += w[root]; w[root++] = (uint32_t)next; }
            else w[next] += w[leaf++];
        }
        w[m - 2] = 0;
        for (next = m - 3; next >= 0; next--) w[next] = w[w[next]] + 1;
        avbl = 1;
        used = dpth = 0;
        root = m - 2;
        next = m - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)w[root] == dpth) { used++; root--; }
            while (avbl > used) { w[next--] = (uint32_t)dpth; avbl--; }
            avbl = 2 * used;
            dpth++;
            used = 0;
        }
    }
    // 3. codes per length, clamped to the limit, and the fix-up
    uint32_t cnt[16];
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int i = 0; i < m; i++) cnt[(int)w[i] < limit ? (int)w[i] : limit]++;
    uint64_t total = 0;
    for (int l = 1; l <= limit; l++) total += (uint64_t)cnt[l] << (limit - l);
    while (total > (1ull << limit)) {
        cnt[limit]--;
        for (int l = limit - 1; l >= 1; l--)
            if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
        total--;
    }
    // 4. the longest codes to the rarest symbols
    int i = 0;
    for (int l = limit; l >= 1; l--)
        for (uint32_t k = 0; k < cnt[l]; k++) len[sym[i++]] = (uint8_t)l;
}

// canonical codes of n symbols from their lengths (RFC 1951 3.2.2), bit-reversed
LRFD_HD inline void lrfd_canonical(const uint8_t* len, int n, uint16_t* code)
{
    uint32_t count[16], next[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int l = 1; l < 16; l++) {
        c = (c + count[l - 1]) << 1;
        next[l] = c;
    }
    for (int s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)lrfd_reverse(next[len[s]]++, len[s]) : 0;
}

// the RFC's order of the code-length code lengths in a dynamic block's header
LRFD_HD inline int lrfd_cl_order(int i)
{
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// The run-length coded sequence of the 258 lengths (the distance length 0 is the last) by the greedy rule at the top: the
// symbols of the code-length alphabet to seq and, where ext is not NULL, the value of each one's extra bits to ext -> how many
LRFD_HD inline int lrfd_run_lengths(const uint8_t* len, uint8_t* seq, uint8_t* ext)
{
    int nseq = 0;
    for (int i = 0; i < LRFD_NSEQ;) {
        const int v = i < LRFD_NLIT ? len[i] : 0;
        int run = 1;
        while (i + run < LRFD_NSEQ && (i + run < LRFD_NLIT ? len[i + run] : 0) == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int t = run < 138 ? run : 138;
                if (ext) ext[nseq] = (uint8_t)(t - 11);
                seq[nseq++] = 18;
                run -= t;
            }
            if (run >= 3) {
                if (ext) ext[nseq] = (uint8_t)(run - 3);
                seq[nseq++] = 17;
                run = 0;
            }
            for (; run > 0; run--) {
                if (ext) ext[nseq] = 0;
                seq[nseq++] = 0;
            }
        } else {
            if (ext) ext[nseq] = 0;
            seq[nseq++] = (uint8_t)v;
            run--;
            while (run >= 3) {
                const int t = run < 6 ? run : 6;
                if (ext) ext[nseq] = (uint8_t)(t - 3);
                seq[nseq++] = 16;
                run -= t;
            }
            for (; run > 0; run--) {
                if (ext) ext[nseq] = 0;
                seq[nseq++] = (uint8_t)v;
            }
        }
    }
    return nseq;
}

// what lrfd_measure decides
struct lrfd_measured {
    int32_t form;       // LRFD_DYNAMIC / LRFD_FIXED / LRFD_STORED
    int32_t nseq;       // entries of seq
    int32_t hclen;      // code-length code lengths sent
    int64_t stream_len; // bytes of the whole stream
    uint8_t cllen[19];  // lengths of the code-length code
};

// The size of one column's stream from its counts alone (freq[LRFD_NLIT], freq[256] = 1): the literals' code lengths (len), the
// run-length sequence (seq), the code-length code, the exact byte counts of the three forms and the tie rule.  Everything that
// decides a size is here; no code, no extra bits and no header byte is touched, so a caller that only counts (k_deflate_sizes,
// lrf_pack_deflate_size_column_i8) keeps an lrfd_count per column instead of an lrfd_work.  w, sym: scratch of LRFD_NLIT entries.
LRFD_HD inline void lrfd_measure(const uint32_t* freq, uint32_t* w, uint16_t* sym, uint8_t* len, uint8_t* seq, int64_t rows, lrfd_measured* m)
{
    lrfd_code_lengths(freq, LRFD_NLIT, LRFD_LIT_LIMIT, len, sym, w);
    const int nseq = lrfd_run_lengths(len, seq, nullptr);
    uint32_t clfreq[19];
    for (int s = 0; s < 19; s++) clfreq[s] = 0;
    for (int i = 0; i < nseq; i++) clfreq[seq[i]]++;
    lrfd_code_lengths(clfreq, 19, LRFD_CL_LIMIT, m->cllen, sym, w);
    int hclen = 19;
    while (hclen > 4 && m->cllen[lrfd_cl_order(hclen - 1)] == 0) hclen--;
    // exact bit counts of the three forms
    uint64_t dyn_bits = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen, fix_bits = 3;
    for (int i = 0; i < nseq; i++) dyn_bits += m->cllen[seq[i]] + (seq[i] == 16 ? 2 : seq[i] == 17 ? 3 : seq[i] == 18 ? 7 : 0);
    for (int s = 0; s < LRFD_NLIT; s++) {
        dyn_bits += (uint64_t)freq[s] * len[s];
        fix_bits += (uint64_t)freq[s] * (s < 144 ? 8 : s < 256 ? 9 : 7);
    }
    const int64_t dyn_len = 2 + (int64_t)((dyn_bits + 7) / 8) + 4, fix_len = 2 + (int64_t)((fix_bits + 7) / 8) + 4;
    m->form = LRFD_STORED;
    m->stream_len = lrfd_bound(rows);
    if (fix_len < m->stream_len) { m->form = LRFD_FIXED; m->stream_len = fix_len; }
    if (dyn_len < m->stream_len) { m->form = LRFD_DYNAMIC; m->stream_len = dyn_len; }
    m->nseq = nseq;
    m->hclen = hclen;
}

// The plan of one column from its counts (k->freq, freq[256] = 1): the form, the exact length of the stream (lrfd_measure), then
// the code table and the bits in front of the first literal, written to hdr (LRFD_HDR_MAX bytes, zero on entry).
LRFD_HD inline void lrfd_plan(lrfd_work* k, int64_t rows, uint8_t* hdr)
{
    lrfd_measured m;
    lrfd_measure(k->freq, k->w, k->sym, k->len, k->seq, rows, &m);
    const uint8_t* cllen = m.cllen;
    const int nseq = m.nseq, hclen = m.hclen;
    k->form = m.form;
    k->stream_len = m.stream_len;
    hdr[0] = 0x78;
    hdr[1] = 0x01;
    uint64_t pos = 16;
    if (k->form == LRFD_STORED) { k->hdr_bits = 16; return; }
    lrfd_put_bits(hdr, pos, 1, 1); pos += 1; // BFINAL
    if (k->form == LRFD_FIXED) {
        lrfd_put_bits(hdr, pos, 1, 2); pos += 2;
        for (int s = 0; s < LRFD_NLIT; s++) { // RFC 1951 3.2.6
            k->len[s] = s < 144 ? 8 : s < 256 ? 9 : 7;
            k->code[s] = (uint16_t)lrfd_reverse(s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : 0, k->len[s]);
        }
        k->hdr_bits = (uint32_t)pos;
        return;
    }
    lrfd_canonical(k->len, LRFD_NLIT, k->code);
    uint16_t clcode[19];
    lrfd_canonical(cllen, 19, clcode);
    lrfd_run_lengths(k->len, k->seq, k->ext); // (the same sequence again, now with the extra bits)
    lrfd_put_bits(hdr, pos, 2, 2); pos += 2;
    lrfd_put_bits(hdr, pos, LRFD_NLIT - 257, 5); pos += 5; // HLIT
    lrfd_put_bits(hdr, pos, 0, 5); pos += 5;               // HDIST: one code
    lrfd_put_bits(hdr, pos, (uint32_t)(hclen - 4), 4); pos += 4;
    for (int i = 0; i < hclen; i++) { lrfd_put_bits(hdr, pos, cllen[lrfd_cl_order(i)], 3); pos += 3; }
    for (int i = 0; i < nseq; i++) {
        const int s = k->seq[i];
        lrfd_put_bits(hdr, pos, clcode[s], cllen[s]); pos += cllen[s];
        const int eb = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
        if (eb) { lrfd_put_bits(hdr, pos, k->ext[i], eb); pos += eb; }
    }
    k->hdr_bits = (uint32_t)pos;
}

// the big-endian Adler-32 trailer from A = 1 + sum d and B = rows + sum (rows - i) d_i, both already reduced mod 65521
LRFD_HD inline void lrfd_adler_bytes(uint32_t A, uint32_t B, uint8_t t[4])
{
    t[0] = (uint8_t)(B >> 8); t[1] = (uint8_t)(B & 0xff); t[2] = (uint8_t)(A >> 8); t[3] = (uint8_t)(A & 0xff);
}
#endif
