// Test-only C entry to plan_metrics_ragged and plan_metrics_chunks (lrf_amd/csrc/lrf_plan.cpp) for
// tests/test_metrics_ragged_plan.py: built with the host compiler, no device.
#include "../lrf_amd/csrc/lrf_plan.h"

enum { PAIR_INTS = 10, SPAN_INTS = 5 };

// pairs: n x (H, W, a_off, b_off).  out_pairs: (a_off, b_off, H, W, ntx, nt, wg0, src, vec, 0) per pair; out_spans: (a_off, b_off,
// n, wg0, vec) per span, at most max_spans.  counts: (pairs built, spans built, tile_wgs, span_wgs); refusal: (check, pair, a, b).
// Returns the refusal's check (0: accepted), or -1 when the spans do not fit.
extern "C" int lrf_test_plan_metrics_ragged(long n, const long* pairs, int C, long a_len, long b_len, long a_base, long b_base, int want_ssim,
                                            long* out_pairs, long* out_spans, long max_spans, long* counts, long* refusal)
{
    static_assert(sizeof(lrf_image_pair) == 4 * sizeof(long), "the test hands the pairs over as longs");
    const MetricsCall k = {C, a_len, b_len, (uintptr_t)a_base, (uintptr_t)b_base, want_ssim != 0};
    const MetricsRaggedPlan p = plan_metrics_ragged(n, reinterpret_cast<const lrf_image_pair*>(pairs), k);
    counts[0] = (long)p.pairs.size();
    counts[1] = (long)p.spans.size();
    counts[2] = p.tile_wgs;
    counts[3] = p.span_wgs;
    refusal[0] = p.refusal.check;
    refusal[1] = (long)p.refusal.pair;
    refusal[2] = (long)p.refusal.a;
    refusal[3] = (long)p.refusal.b;
    if ((long)p.spans.size() > max_spans) return -1;
    for (size_t i = 0; i < p.pairs.size(); i++) {
        const MetricsPairDesc& d = p.pairs[i];
        const long v[PAIR_INTS] = {d.a_off, d.b_off, d.H, d.W, d.ntx, d.nt, d.wg0, d.src, d.vec, d.pad_};
        for (int j = 0; j < PAIR_INTS; j++) out_pairs[i * PAIR_INTS + j] = v[j];
    }
    for (size_t i = 0; i < p.spans.size(); i++) {
        const MetricsSpanDesc& d = p.spans[i];
        const long v[SPAN_INTS] = {d.a_off, d.b_off, d.n, d.wg0, d.vec};
        for (int j = 0; j < SPAN_INTS; j++) out_spans[i * SPAN_INTS + j] = v[j];
    }
    return p.refusal.check;
}

// sizes: n x (H, W).  out_chunks: (item0, nitems, bytes) per chunk, at most n; off: per item.  Returns the number of chunks;
// *max_bytes: the largest chunk.
extern "C" long lrf_test_plan_metrics_chunks(long n, const long* sizes, long cap, long* out_chunks, long* off, long* max_bytes)
{
    std::vector<lrf_ragged_image> items((size_t)n);
    for (long i = 0; i < n; i++) {
        items[(size_t)i] = lrf_ragged_image{};
        items[(size_t)i].H = sizes[2 * i];
        items[(size_t)i].W = sizes[2 * i + 1];
    }
    const MetricsChunks c = plan_metrics_chunks(n, items.data(), cap);
    for (size_t j = 0; j < c.chunks.size(); j++) {
        out_chunks[3 * j] = (long)c.chunks[j].item0;
        out_chunks[3 * j + 1] = (long)c.chunks[j].nitems;
        out_chunks[3 * j + 2] = (long)c.chunks[j].bytes;
    }
    for (long i = 0; i < n; i++) off[i] = (long)c.off[(size_t)i];
    *max_bytes = (long)c.max_bytes;
    return (long)c.chunks.size();
}
