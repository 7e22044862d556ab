// lrf_ctx.hip — host side of liblrf_hip.so that owns no kernel: error convention, the context and its workspace, image
// geometry, descriptor tables, the streams of a call's kernel families (its launch plan: lrf_plan.cpp), the memory helpers of the C ABI
// (include/lrf_hip.h).  The kernels and their launch sequences: lrf_encode8.hip (the 64-column path), lrf_any.hip (any-shape,
// RGB colour space, svd); the host -> host pipeline: lrf_pipe.hip.
#include "lrf_host.h"

static thread_local char g_err[512] = "";

int set_err(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
const char* last_err() { return g_err; }

int ensure(lrf_ctx* c, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return LRF_OK;
    if (b.p) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t cap = bytes + bytes / 8;
    hipError_t e = hipMalloc(&b.p, cap);
    if (e != hipSuccess) return set_err(LRF_ENOMEM, "hipMalloc(%zu) failed: %s", cap, hipGetErrorString(e));
    b.cap = cap;
    return LRF_OK;
}

int upload(lrf_ctx* c, DevBuf& b, const void* src, size_t bytes)
{
    int rc = ensure(c, b, bytes);
    if (rc) return rc;
    if (bytes > c->h_stage_cap) {
        if (c->h_stage) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipHostFree(c->h_stage));
        }
        HIP_TRY(hipHostMalloc(&c->h_stage, bytes * 2, hipHostMallocDefault));
        c->h_stage_cap = bytes * 2;
    }
    // the staging buffer may still be read by an earlier async copy
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(c->h_stage, src, bytes);
    HIP_TRY(hipMemcpyAsync(b.p, c->h_stage, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LRF_OK;
}

void fold_events(lrf_ctx* c)
{
    for (int k = 0; k < LRF_K_SLOTS; k++) {
        for (auto& pr : c->ev[k]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                c->acc_ms[k] += ms;
                c->acc_n[k] += 1;
            }
            c->ev_pool.push_back(pr.first);
            c->ev_pool.push_back(pr.second);
        }
        c->ev[k].clear();
    }
}

// ---- geometry ---------------------------------------------------------------------------------
// (plane_dims, geom_of: lrf_plan.cpp)
int make_geom(int64_t H, int64_t W, ImageGeom* g)
{
    int64_t h, w;
    const int bad = geom_of(H, W, g, &h, &w);
    if (bad == 0) return LRF_OK;
    if (bad < 10) return set_err(LRF_EINVAL, "image %ldx%ld too small", (long)H, (long)W);
    return set_err(LRF_EINVAL, "reflect padding larger than the plane (%ldx%ld)", (long)h, (long)w);
}

// ---- descriptor tables (add_plane: lrf_plan.cpp) ------------------------------------------------
int check_params(int64_t M, int64_t N, int R, int K, int lo, int hi)
{
    if (N != LRF_PATCH_ELEMS) return set_err(LRF_ENOTSUP, "N=%ld: only N=%d (8x8 patches) is implemented", (long)N, LRF_PATCH_ELEMS);
    if (R < 1) return set_err(LRF_EINVAL, "rank must be >= 1 (got %d)", R);
    if (R > LRF_MAX_RANK) return set_err(LRF_ENOTSUP, "rank %d > %d not implemented", R, LRF_MAX_RANK);
    if (K < 1) return set_err(LRF_ENOTSUP, "num_iters=%d: use lrf_qmf_svd_init_f32 for K=0", K);
    if (lo > hi || lo < -128 || hi > 127) return set_err(LRF_EINVAL, "bounds (%d,%d) outside int8", lo, hi);
    if (M < 1) return set_err(LRF_EINVAL, "M must be >= 1");
    // u.mT @ u: each 384-row block partial is an exact integer in fp32 for any int8 bounds (384 * 128^2 < 2^24), whatever the
    // order inside the block, and the block partials are added in block order like the reference's sgemm (K blocked by 384),
    // so the result is the reference's even where the running sum leaves the exact range.
    (void)M;
    return LRF_OK;
}

// ---- the launch plan's settings and what the context holds per run (struct FamRun, lrf_plan.h) --
PlanSettings plan_settings(const lrf_ctx* c)
{
    PlanSettings s = plan_settings_env();
    s.persist_arch = c->persist_arch;
    return s;
}
FamBufs run_bufs(lrf_ctx* c, const FamRun& r, bool mixed)
{
    if (mixed && r.pitch == 16) return FamBufs{(float*)c->vf16.p, (float*)c->wf16.p, (float*)c->bf16.p, (float*)c->pp16.p, (float*)c->qp16.p};
    return FamBufs{(float*)c->vf.p, (float*)c->wf.p, (float*)c->bf.p, (float*)c->ppart.p, (float*)c->qpart.p};
}

hipStream_t run_stream(lrf_ctx* c, size_t run_idx) { return (c->fam_forked && run_idx > 0) ? c->fam_stream[run_idx - 1] : c->stream; }
// FAM_STREAMS_INIT: the fork is joined again inside the caller's stage (run_init's initialisation kernels) — kernel profiling may
// stay on (the stage's event pair on the caller's stream encloses fork and join); a fork that lasts into run_bcd is refused
// while profiling is on (the per-launch event pairs are recorded on the caller's stream only).
int fam_fork_streams(lrf_ctx* c, FamStreams layout, size_t nruns)
{
    c->fam_forked = false;
    if (layout == FAM_STREAMS_NONE || (c->profile && layout != FAM_STREAMS_INIT) || nruns < 2 || nruns > 3) return LRF_OK;
    if (!c->fam_fork) HIP_TRY(hipEventCreateWithFlags(&c->fam_fork, hipEventDisableTiming));
    for (size_t i = 0; i + 1 < nruns; i++) {
        if (!c->fam_stream[i]) HIP_TRY(hipStreamCreateWithFlags(&c->fam_stream[i], hipStreamNonBlocking));
        if (!c->fam_join[i]) HIP_TRY(hipEventCreateWithFlags(&c->fam_join[i], hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(c->fam_fork, c->stream));
    for (size_t i = 0; i + 1 < nruns; i++) HIP_TRY(hipStreamWaitEvent(c->fam_stream[i], c->fam_fork, 0));
    c->fam_forked = true;
    return LRF_OK;
}
int fam_join_streams(lrf_ctx* c, size_t nruns)
{
    if (!c->fam_forked) return LRF_OK;
    c->fam_forked = false;
    for (size_t i = 0; i + 1 < nruns && i < 2; i++) {
        if (!c->fam_stream[i] || !c->fam_join[i]) continue;
        HIP_TRY(hipEventRecord(c->fam_join[i], c->fam_stream[i]));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->fam_join[i], 0));
    }
    return LRF_OK;
}

// Row chunks of the exact Gram pass (k_gram64: one workgroup per chunk, one 128-bit partial per chunk for k_init to add):
// LRF_GRAM_ROWS rows each — fewer for small calls, so that the pass still has a few workgroups per CU (a chunk is a latency
// chain of 64-row blocks: one 512x768 image 38 -> 14 us, 64 images 57 -> 44 us).  Exact integer sums: the cut does not change a bit.
static void finish_gram_chunks(Tables& t)
{
    long rows = 0;
    for (size_t pi = 0; pi < t.planes.size(); pi++)
        if (t.planes[pi].init_src == (int)pi) rows += t.planes[pi].M; // (planes that share another's initialisation need no Gram matrix)
    int per = LRF_GRAM_ROWS;
    while (per > 384 && rows / per < 768) per >>= 1;
    // the fused planes (k_planes16_gram: two workgroups per CU, 512 of them a round): chunks of LRF_GRAM_ROWS_FUSED rows
    long rows_f = 0;
    for (size_t pi = 0; pi < t.planes.size(); pi++)
        if (t.planes[pi].init_src == (int)pi && t.planes[pi].gram_fused) rows_f += t.planes[pi].M;
    int per_f = LRF_GRAM_ROWS_FUSED;
    while (per_f > 384 && rows_f / per_f < 768) per_f >>= 1;
    const int per_k = per;
    t.gchunks.clear();
    for (int pass = 0; pass < 2; pass++) { // the chunks of k_gram64 first, then those the planes kernel computes (k_planes16_gram)
        per = pass ? per_f : per_k;
        for (int pi = 0; pi < (int)t.planes.size(); pi++) {
            PlaneDesc& pd = t.planes[pi];
            if ((pd.gram_fused != 0) != (pass == 1)) continue;
            pd.gch0 = (int)t.gchunks.size();
            pd.ngch = pd.init_src == pi ? (pd.M + per - 1) / per : 0;
            for (int g = 0; g < pd.ngch; g++) {
                const int row0 = g * per;
                t.gchunks.push_back(GramChunk{pi, row0, pd.gch0 + g, pd.M - row0 < per ? pd.M - row0 : per});
            }
        }
        if (pass == 0) t.ngram_rest = (int)t.gchunks.size();
    }
}

int upload_tables(lrf_ctx* c, Tables& t, const BcdPlan& plan)
{
    finish_gram_chunks(t);
    // the tables only depend on the call's geometry: skip the (synchronising) upload when nothing changed
    // (the Gram chunk table follows from the plane table: it is not part of the key)
    size_t pb = t.planes.size() * sizeof(PlaneDesc), bb = t.blocks.size() * sizeof(BlockDesc);
    std::vector<char> key(pb + bb);
    memcpy(key.data(), t.planes.data(), pb);
    memcpy(key.data() + pb, t.blocks.data(), bb);
    if (key == c->table_key) return LRF_OK;
    int victim = 0;
    for (int j = 0; j < LRF_TABLE_SETS - 1; j++) {
        lrf_ctx::TableSet& a = c->talt[j];
        const bool hit = a.key == key;
        if (hit || a.stamp < c->talt[victim].stamp) victim = j;
        if (hit) break;
    }
    { // the current set goes to the victim's place, the victim's buffers become current (its tables, if this was a hit)
        lrf_ctx::TableSet& a = c->talt[victim];
        std::swap(c->planes, a.planes);
        std::swap(c->blocks, a.blocks);
        std::swap(c->gchunks, a.gchunks);
        c->table_key.swap(a.key);
        a.stamp = ++c->tstamp;
    }
    if (key == c->table_key) return LRF_OK;
    c->table_key.clear();
    int rc = upload(c, c->planes, t.planes.data(), pb);
    if (rc) return rc;
    rc = upload(c, c->blocks, t.blocks.data(), bb);
    if (rc) return rc;
    rc = upload(c, c->gchunks, t.gchunks.data(), t.gchunks.size() * sizeof(GramChunk));
    if (rc) return rc;
    if ((rc = ensure(c, c->gpart, t.gchunks.size() * (size_t)LRF_GRAM_SLOT * sizeof(ulonglong2)))) return rc;
    if ((rc = ensure(c, c->gexp, t.planes.size() * sizeof(int)))) return rc;
    size_t np = t.planes.size(), nb = t.blocks.size();
    size_t rp = (size_t)plan.rp, gts = rp == 16 ? (size_t)LRF_GT_STRIDE : (size_t)LRF_GTB_STRIDE;
    if ((rc = ensure(c, c->vf, np * 64 * rp * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->wf, np * 64 * rp * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->bf, np * gts * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->ppart, nb * 64 * rp * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->qpart, nb * rp * rp * sizeof(float)))) return rc;
    if (plan.mixed) {
        if ((rc = ensure(c, c->vf16, np * 64 * 16 * sizeof(float)))) return rc;
        if ((rc = ensure(c, c->wf16, np * 64 * 16 * sizeof(float)))) return rc;
        if ((rc = ensure(c, c->bf16, np * (size_t)LRF_GT_STRIDE * sizeof(float)))) return rc;
        if ((rc = ensure(c, c->pp16, nb * 64 * 16 * sizeof(float)))) return rc;
        if ((rc = ensure(c, c->qp16, nb * 16 * 16 * sizeof(float)))) return rc;
    }
    c->table_key.swap(key);
    return LRF_OK;
}

// The error word of k_bcd_p (no synchronisation here: the caller has waited for the stream, by whatever means).  A poll that
// expired invalidates the call it belongs to and every persistent call queued behind it on this context (those find the
// queue state marked and leave at once): the message names the first one, the state is cleared by the next launch.
int ctx_check(lrf_ctx* c)
{
    if (!c->h_perr || !*c->h_perr) return LRF_OK;
    const int first = *c->h_perr;
    *c->h_perr = 0;
    c->psync_dirty = true;
    return set_err(LRF_EHIP, "k_bcd_p: a wave's poll for a V update expired in persistent launch %d of this context (%d issued so far): "
                             "the factors of that call and of every later call up to this check are invalid", first, c->pseq);
}


// ---- C ABI ------------------------------------------------------------------------------------
extern "C" {

const char* lrf_last_error(void) { return last_err(); }


int lrf_version(void) { return 1; }

int lrf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lrf_ctx_create(int device, lrf_ctx** out)
{
    if (!out) return set_err(LRF_EINVAL, "out is NULL");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return set_err(LRF_EINVAL, "device %d out of range (%d visible)", device, n);
    DevGuard dev_guard_(device);
    if (dev_guard_.err != hipSuccess) return set_err(LRF_EHIP, "selecting device %d failed: %s", device, hipGetErrorString(dev_guard_.err));
    lrf_ctx* c = new lrf_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return set_err(LRF_EHIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    {
        // k_bcd_p hands data from wave to wave inside one launch with sc1 stores / loads and agent-scope tickets: a hardware
        // path measured on gfx950 (MI355X_MICROARCH.md), not a guarantee of the programming model — other parts keep the
        // launch-per-iteration path
        hipDeviceProp_t prop;
        c->persist_arch = hipGetDeviceProperties(&prop, device) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    }
    c->init_sweeps = (int)env_long("LRF_DEBUG_INIT_SWEEPS", 0); // test hook (lrf_env.h)
    *out = c;
    return LRF_OK;
}

void lrf_ctx_destroy(lrf_ctx* c)
{
    if (!c) return;
    DevGuard dev_guard_(c->device);
    (void)hipStreamSynchronize(c->stream);
    fold_events(c);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    DevBuf* bufs[] = {&c->gchunks, &c->gpart, &c->gexp, &c->planes, &c->blocks, &c->vf, &c->wf, &c->bf, &c->ppart, &c->qpart, &c->x, &c->sign,
                      &c->sx, &c->sg, &c->svn, &c->swn, &c->suf, &c->smm,
                      &c->any_uf, &c->any_vf, &c->any_a, &c->any_b, &c->any_p, &c->any_e2, &c->any_g, &c->any_td,
                      &c->vf16, &c->wf16, &c->bf16, &c->pp16, &c->qp16, &c->metrics, &c->ssim_scratch, &c->sse_tab, &c->ragged_tab, &c->enc_ragged_tab, &c->enc_gray_tab, &c->crop_desc, &c->crop_tab, &c->gray_desc, &c->scaled_pool, &c->deflate_tab, &c->inflate_tab};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (auto& a : c->talt) {
        DevBuf* tb[] = {&a.planes, &a.blocks, &a.gchunks};
        for (DevBuf* b : tb)
            if (b->p) (void)hipFree(b->p);
    }
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (auto& s : c->crop_slot) {
        if (s.h) (void)hipHostFree(s.h);
        if (s.copied) (void)hipEventDestroy(s.copied);
    }
    for (auto& s : c->deflate_slot) {
        if (s.h) (void)hipHostFree(s.h);
        if (s.copied) (void)hipEventDestroy(s.copied);
    }
    for (auto& s : c->inflate_slot) {
        if (s.h) (void)hipHostFree(s.h);
        if (s.copied) (void)hipEventDestroy(s.copied);
    }
    if (c->h_perr) (void)hipHostFree(c->h_perr);
    if (c->psync.p) (void)hipFree(c->psync.p);
    for (int i = 0; i < 2; i++) {
        if (c->fam_stream[i]) {
            (void)hipStreamSynchronize(c->fam_stream[i]);
            (void)hipStreamDestroy(c->fam_stream[i]);
        }
        if (c->fam_join[i]) (void)hipEventDestroy(c->fam_join[i]);
    }
    if (c->fam_fork) (void)hipEventDestroy(c->fam_fork);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int lrf_ctx_set_stream(lrf_ctx* c, void* hip_stream)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    hipStream_t s = (hipStream_t)hip_stream; // NULL is HIP's default stream, a valid handle
    if (s == c->stream) return LRF_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = s;
    return LRF_OK;
}

int lrf_ctx_use_own_stream(lrf_ctx* c)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    if (c->stream == c->own_stream) return LRF_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = c->own_stream;
    return LRF_OK;
}

int lrf_ctx_synchronize(lrf_ctx* c)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    LRF_ON_DEVICE(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ctx_check(c);
}

int lrf_ctx_check(lrf_ctx* c)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    return ctx_check(c);
}

int lrf_ctx_last_luma_source(const lrf_ctx* c) { return c ? c->last_luma_source : -1; }

int lrf_ctx_last_x_residency(const lrf_ctx* c, int64_t* kept_bytes)
{
    if (kept_bytes) *kept_bytes = c ? (int64_t)c->last_x_kept_bytes : -1;
    return c ? c->last_x_kept_planes : -1;
}

size_t lrf_ctx_workspace_bytes(const lrf_ctx* c)
{
    if (!c) return 0;
    const DevBuf* bufs[] = {&c->gchunks, &c->gpart, &c->gexp, &c->planes, &c->blocks, &c->vf, &c->wf, &c->bf, &c->ppart, &c->qpart, &c->x, &c->sign,
                            &c->sx, &c->sg, &c->svn, &c->swn, &c->suf, &c->smm,
                            &c->any_uf, &c->any_vf, &c->any_a, &c->any_b, &c->any_p, &c->any_e2, &c->any_g, &c->any_td,
                      &c->vf16, &c->wf16, &c->bf16, &c->pp16, &c->qp16, &c->metrics, &c->ssim_scratch, &c->sse_tab, &c->ragged_tab, &c->enc_ragged_tab, &c->enc_gray_tab, &c->crop_desc, &c->crop_tab, &c->gray_desc, &c->scaled_pool, &c->deflate_tab, &c->inflate_tab};
    size_t total = 0;
    for (const DevBuf* b : bufs) total += b->cap;
    for (const auto& a : c->talt) total += a.planes.cap + a.blocks.cap + a.gchunks.cap;
    return total;
}

int lrf_ctx_trim(lrf_ctx* c)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    LRF_ON_DEVICE(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    DevBuf* bufs[] = {&c->gchunks, &c->gpart, &c->gexp, &c->planes, &c->blocks, &c->vf,
                      &c->wf, &c->bf, &c->ppart, &c->qpart, &c->x, &c->sign, &c->sx, &c->sg, &c->svn, &c->swn, &c->suf, &c->smm,
                      &c->any_uf, &c->any_vf, &c->any_a, &c->any_b, &c->any_p, &c->any_e2, &c->any_g, &c->any_td,
                      &c->vf16, &c->wf16, &c->bf16, &c->pp16, &c->qp16, &c->metrics, &c->ssim_scratch, &c->sse_tab, &c->ragged_tab, &c->enc_ragged_tab, &c->enc_gray_tab, &c->crop_desc, &c->crop_tab, &c->gray_desc, &c->scaled_pool, &c->deflate_tab, &c->inflate_tab};
    for (DevBuf* b : bufs) {
        if (b->p) HIP_TRY(hipFree(b->p));
        b->p = nullptr;
        b->cap = 0;
    }
    for (auto& a : c->talt) {
        DevBuf* tb[] = {&a.planes, &a.blocks, &a.gchunks};
        for (DevBuf* b : tb) {
            if (b->p) HIP_TRY(hipFree(b->p));
            b->p = nullptr;
            b->cap = 0;
        }
        a.key.clear();
        a.stamp = 0;
    }
    c->table_key.clear();     // the descriptor tables went with their buffers
    return LRF_OK;
}

int lrf_ctx_profile(lrf_ctx* c, int enable)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    c->profile = enable != 0;
    c->profile_mask = ~0u;
    return LRF_OK;
}

int lrf_ctx_profile_kernels(lrf_ctx* c, unsigned mask)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    c->profile = mask != 0;
    c->profile_mask = mask;
    return LRF_OK;
}

int lrf_ctx_kernel_time(lrf_ctx* c, int id, double* total_ms, long* launches)
{
    if (!c || id < 0 || id >= LRF_K_SLOTS) return set_err(LRF_EINVAL, "bad kernel id");
    HIP_TRY(hipStreamSynchronize(c->stream));
    fold_events(c);
    if (total_ms) *total_ms = c->acc_ms[id];
    if (launches) *launches = c->acc_n[id];
    return LRF_OK;
}

int lrf_ctx_profile_reset(lrf_ctx* c)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    fold_events(c);
    for (int k = 0; k < LRF_K_SLOTS; k++) { c->acc_ms[k] = 0; c->acc_n[k] = 0; }
    return LRF_OK;
}

int lrf_malloc(lrf_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return set_err(LRF_EINVAL, "NULL argument");
    LRF_ON_DEVICE(c);
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) return set_err(LRF_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return LRF_OK;
}

int lrf_free(lrf_ctx* c, void* p)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    if (p) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(p));
    }
    return LRF_OK;
}

int lrf_memcpy_h2d(lrf_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LRF_OK;
}

int lrf_memcpy_d2h(lrf_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return set_err(LRF_EINVAL, "ctx is NULL");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LRF_OK;
}

int lrf_plane_dims(int64_t H, int64_t W, int c, int64_t* h, int64_t* w, int64_t* hp, int64_t* wp, int64_t* M)
{
    if (c < 0 || c > 2 || H < 1 || W < 1 || !h || !w || !hp || !wp || !M) return set_err(LRF_EINVAL, "bad argument");
    plane_dims(H, W, c, h, w, hp, wp, M);
    return LRF_OK;
}

int lrf_host_alloc(size_t bytes, void** out)
{
    if (!out) return set_err(LRF_EINVAL, "out is NULL");
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return set_err(LRF_ENOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return LRF_OK;
}

int lrf_host_free(void* p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return LRF_OK;
}

int lrf_host_register(void* p, size_t bytes)
{
    if (!p) return set_err(LRF_EINVAL, "NULL argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return LRF_OK;
}

int lrf_host_unregister(void* p)
{
    if (!p) return set_err(LRF_EINVAL, "NULL argument");
    HIP_TRY(hipHostUnregister(p));
    return LRF_OK;
}

} // extern "C"
