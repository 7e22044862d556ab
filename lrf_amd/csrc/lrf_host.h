// lrf_host.h — what the host-side translation units of liblrf_hip.so share: error convention, device guard, the context,
// descriptor tables (their builder and the launch plan of a call: lrf_plan.h).  lrf_ctx.hip defines the functions declared here unless noted.
#ifndef LRF_HOST_H
#define LRF_HOST_H
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../include/lrf_hip.h"
#include "lrf_internal.h"
#include "lrf_env.h"
#include "lrf_plan.h"

// the planes qmf_encode forms hold YCbCr samples, 0 or in [0.114, 255.5]: all below 2^8 and exact on the grid 2^(8-35)
// (run_init: selects k_gram64's integer digit extraction; callers with arbitrary X pass LRF_GRAM_EXP_FROM_DATA)
#define LRF_PLANES_GRAM_EXP 8
#define LRF_TABLE_SETS 6 // descriptor-table sets a context keeps resident (upload_tables)
#define LRF_CROP_SLOTS 4 // pinned staging slots of lrf_qmf_decode_crops_rgb_u8's crop table

int set_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const char* last_err();

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return set_err(LRF_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                             __FILE__, __LINE__);                                         \
    } while (0)

// Makes the context's device current for the duration of one ABI call and restores the caller's device on the way out
// (a torch process encoding a cuda:1 tensor while its current device is cuda:0 must not find cuda:1 current afterwards).
struct DevGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DevGuard(int device)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DevGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard&) = delete;
    DevGuard& operator=(const DevGuard&) = delete;
};
#define LRF_ON_DEVICE(c)                                                                                  \
    DevGuard dev_guard_((c)->device);                                                                     \
    if (dev_guard_.err != hipSuccess)                                                                     \
        return set_err(LRF_EHIP, "selecting device %d failed: %s", (c)->device, hipGetErrorString(dev_guard_.err))

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct lrf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    DevBuf planes, blocks, gchunks, vf, wf, bf, ppart, qpart, x, sign;
    DevBuf gpart, gexp; // exact Gram partials (128-bit integers per chunk) and per-matrix grid exponents (lrf_gram_kernels.hip)
    DevBuf sx, sg, svn, swn, suf, smm; // SVD baseline workspace
    DevBuf any_uf, any_vf, any_a, any_b, any_p, any_e2, any_g, any_td; // any-shape path (lrf_anyshape_host.inc)
    DevBuf metrics; // lrf_image_metrics_u8: a float64 slot per (image, channel, tile), then (max, 255 - min) per image
    DevBuf ssim_scratch; // lrf_qmf_ssim_ragged_rgb_u8: the decoded images of the chunk in flight (at most its cap, or the largest item)
    DevBuf sse_tab; // lrf_qmf_sweep_sse_rgb_u8: its table of rank triples (SseItem) ...
    std::vector<char> sse_key; // ... and the bytes now resident there (calls that repeat a sweep skip the synchronising upload)
    DevBuf ragged_tab; // lrf_qmf_decode_ragged_rgb_u8: the image descriptors (RaggedDesc), behind them the block table ...
    std::vector<char> ragged_key; // ... and the descriptor bytes now resident there
    DevBuf crop_desc; // lrf_qmf_decode_crops_rgb_u8: the image descriptors (RaggedDesc) ...
    std::vector<char> crop_desc_key; // ... and the descriptor bytes now resident there
    DevBuf crop_tab;  // the crop table (CropEntry) of the call in flight; filled stream-ordered from the pinned slots below, which take turns
    struct CropSlot {
        void* h = nullptr; // page-locked
        size_t cap = 0;
        hipEvent_t copied = nullptr; // recorded behind the slot's copy: the slot is written again only after it
        bool in_flight = false;
    };
    CropSlot crop_slot[LRF_CROP_SLOTS];
    int crop_next = 0;
    DevBuf gray_desc; // the gray loader (lrf_qmf_decode_gray_ragged_u8, _crops_, _resized_crops_): its image descriptors (GrayDesc) ...
    std::vector<char> gray_desc_key; // ... and the bytes now resident there; its item lists travel through crop_tab and the slots above
    DevBuf scaled_pool; // lrf_qmf_decode_scaled_*: the pooled V tables (int16) of the call in flight, written by its k_pool_v
    DevBuf enc_ragged_tab; // lrf_qmf_encode_ragged_rgb_u8: the image descriptors (EncRaggedDesc), behind them the workgroup table ...
    std::vector<char> enc_ragged_key; // ... and the descriptor bytes now resident there
    DevBuf enc_gray_tab; // lrf_qmf_encode_gray_ragged_sweep_u8: the image descriptors (EncGrayDesc), behind them the workgroup table ...
    std::vector<char> enc_gray_key; // ... and the descriptor bytes now resident there
    DevBuf deflate_tab; // lrf_deflate_columns_i8: the matrix table (DeflateMat) of the call in flight, filled stream-ordered from ...
    CropSlot deflate_slot[LRF_CROP_SLOTS]; // ... pinned slots of its own, which take turns as the crop table's do
    int deflate_next = 0;
    DevBuf inflate_tab; // lrf_inflate_columns_i8: the column table (InflateCol) of the call in flight, filled stream-ordered from ...
    CropSlot inflate_slot[LRF_CROP_SLOTS]; // ... pinned slots of its own
    int inflate_next = 0;
    DevBuf vf16, wf16, bf16, pp16, qp16; // the pitch-16 tables of a call that mixes kernel families (BcdPlan::mixed)
    // host staging for descriptor tables (pinned)
    void* h_stage = nullptr;
    size_t h_stage_cap = 0;
    // profiling
    bool profile = false;
    unsigned profile_mask = ~0u; // kernel ids (bit per LRF_K_*) that get event pairs while `profile` is on
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[LRF_K_SLOTS];
    std::vector<hipEvent_t> ev_pool;
    double acc_ms[LRF_K_SLOTS] = {0};
    long acc_n[LRF_K_SLOTS] = {0};
    int init_sweeps = 0; // developer aid: stop k_init after stage n (0 = run everything)
    std::vector<char> table_key; // bytes of the descriptor tables now resident on the device (planes / blocks)
    // earlier tables, least recently used one replaced: calls that alternate between a few geometries (a pipeline slot sees
    // its full sub-batch size and the two or three sizes of the tapered tail) find them resident and skip the synchronising upload
    struct TableSet {
        DevBuf planes, blocks, gchunks;
        std::vector<char> key;
        unsigned long stamp = 0;
    };
    TableSet talt[LRF_TABLE_SETS - 1];
    unsigned long tstamp = 0;
    unsigned attr_done = 0;      // hipFuncSetAttribute call sites already executed for this context's device (bit per site)
    unsigned attr_persist = 0;   // likewise, one bit per instantiation of k_bcd_p (lrf_bcd_persist.hip)
    // Kernel families of one call on streams of their own (BcdPlan::streams; run_init forks, run_bcd joins): the first run stays
    // on `stream`, the others fork behind the Gram pass.  Created on first use; never to the call's end while kernel profiling is on.
    hipStream_t fam_stream[2] = {nullptr, nullptr};
    hipEvent_t fam_fork = nullptr, fam_join[2] = {nullptr, nullptr};
    bool fam_forked = false;     // run_init forked: run_bcd uses the same streams and joins
    int last_luma_source = -1;   // where the luma blocks of the last lrf_qmf_encode_rgb_u8 read X: 0 = the X workspace, 1 = the image bytes; -1: no such call yet
    int last_x_kept_planes = -1; // the residency decision of the last lrf_qmf_encode_rgb_u8 (plan_x_residency): planes kept on the default cache
    long last_x_kept_bytes = -1; // policy and their X bytes, 0 / 0 when the policy did not apply; -1: no such call yet
    hipEvent_t planes_done = nullptr; // set by a pipe: recorded after the planes kernel of lrf_qmf_encode_rgb_u8 (input buffer free)
    // the persistent iteration kernel (k_bcd_p, default for large rank <= 8 calls): its queue head, tickets and flags; its error
    // word is page-locked host memory the kernel writes directly — the sequence number of the first launch whose poll expired.
    // It is looked at wherever results are handed back (ctx_check: lrf_ctx_check, lrf_ctx_synchronize, lrf_pipe_wait_next) and at
    // the next persistent call's entry.
    DevBuf psync;
    int* h_perr = nullptr;     // page-locked: k_bcd_p writes its launch number here when a poll expires
    int pseq = 0;              // persistent launches issued on this context so far (the numbers start at 1)
    bool psync_dirty = false;  // the queue state of k_bcd_p is not all-zero (a failed launch)
    bool persist_arch = false; // the device is the part the in-launch hand-offs of k_bcd_p were validated on (gfx950)
};


int ensure(lrf_ctx* c, DevBuf& b, size_t bytes);
int upload(lrf_ctx* c, DevBuf& b, const void* src, size_t bytes);
void fold_events(lrf_ctx* c);
int ctx_check(lrf_ctx* c); // the error word of k_bcd_p (no synchronisation): LRF_OK, or the failure and its message

struct Prof {
    lrf_ctx* c;
    int id;
    hipEvent_t a = nullptr, b = nullptr;
    bool on;
    Prof(lrf_ctx* c_, int id_) : c(c_), id(id_), on(c_->profile && ((c_->profile_mask >> id_) & 1u))
    {
        if (!on) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); }
            else (void)hipEventCreate(&e);
            return e;
        };
        a = get();
        b = get();
        (void)hipEventRecord(a, c->stream);
    }
    ~Prof()
    {
        if (!on) return;
        (void)hipEventRecord(b, c->stream);
        c->ev[id].push_back({a, b});
    }
};


#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

// ---- what the entries that decode windows share across units (lrf_encode8.hip defines the functions; lrf_channels.hip's gray
// loader calls them too)
// A table that stays resident in `buf` under the bytes of its key: `tab`, and behind it `tail` — a function of the key that is
// not part of it.  Calls that repeat the key skip the synchronising upload
int keep_resident(lrf_ctx* c, DevBuf& buf, std::vector<char>& key, const void* tab, size_t tb, const void* tail = nullptr, size_t tail_bytes = 0);
// the item list of one call into lrf_ctx::crop_tab through the pinned staging slots: stream-ordered, no wait for the stream
extern "C" int stage_crop_bytes(lrf_ctx* c, const void* table, size_t bytes);
// DecodeOut: where such an entry writes — the bytes of the _u8 entries or the tensor of the _tensor entries, `len` counted in
// its elements
struct DecodeOut {
    void* p;
    int64_t len;
    int dtype; // LRF_T_*, or -1: uint8
    TensorFmt f;
};
inline DecodeOut bytes_out(uint8_t* rgb, int64_t rgb_len) { return DecodeOut{rgb, rgb_len, -1, TensorFmt{}}; }
// fmt, out, out_bytes of a _tensor entry -> the output in elements; everything is checked before the body sees it
// (lrf_decode_tensor_host.inc)
int tensor_out(const lrf_tensor_format* fmt, void* out, int64_t out_bytes, DecodeOut* o);
// The checks of the ten entries that decode crops (lrf_plan.h: check_window_call, check_windows), refused in the entries' words
// (lrf_encode8.hip defines the two functions).
// check_crop_call: the prologue — NULL, then the ranges of n_images, n_crops and the size; checked_windows: the output's
// capacity and the crop list -> the items of the call's plan
int refuse_window(const WindowRefusal& r, const WindowCall& k);
int check_crop_call(bool null_argument, const WindowCall& k);
template <class Desc, class Crop, class Item>
static int checked_windows(const WindowCall& k, const std::vector<Desc>& descs, const Crop* crops, std::vector<Item>& items)
{
    const WindowRefusal r = check_windows(k, descs, crops, items);
    return r.check == WIN_OK ? LRF_OK : refuse_window(r, k);
}
// fn(T* out) with T the element type of a tensor output
template <class F>
static void with_tensor_type(const DecodeOut& o, F&& fn)
{
    switch (o.dtype) {
    case LRF_T_F32: fn((float*)o.p); break;
    case LRF_T_F16: fn((_Float16*)o.p); break;
    default: fn((__bf16*)o.p); break;
    }
}

// ---- the ragged metrics (lrf_metrics.hip), shared with lrf_qmf_ssim_ragged_rgb_u8 (lrf_encode8.hip)
int refuse_metrics(const MetricsRefusal& r); // a refusal of plan_metrics_ragged in the entries' words
size_t metrics_ragged_workspace(const MetricsRaggedPlan& p); // bytes of lrf_ctx::metrics the launches of p need
// the launches of an accepted plan on the context's stream: the caller holds the device and the timer
int metrics_ragged_launch(lrf_ctx* c, const MetricsRaggedPlan& p, int C, const uint8_t* a, const uint8_t* b, uint64_t* sse, double* ssim);

// ---- geometry (lrf_ctx.hip)
int make_geom(int64_t H, int64_t W, ImageGeom* g);

// ---- descriptor tables and the launch plan (lrf_plan.h: device-free) ----------------------------
int check_params(int64_t M, int64_t N, int R, int K, int lo, int hi);
PlanSettings plan_settings(const lrf_ctx* c); // the process's settings with the context's device
int upload_tables(lrf_ctx* c, Tables& t, const BcdPlan& plan);

// the V / W / b / partial tables a run uses
struct FamBufs {
    float *vf, *wf, *bf, *pp, *qp;
};
FamBufs run_bufs(lrf_ctx* c, const FamRun& r, bool mixed);
hipStream_t run_stream(lrf_ctx* c, size_t run_idx);
int fam_fork_streams(lrf_ctx* c, FamStreams layout, size_t nruns);
int fam_join_streams(lrf_ctx* c, size_t nruns);

// ---- the 64-column encoder (lrf_encode8.hip)
// The part of lrf_qmf_encode_rgb_u8 that may allocate or upload: argument checks, the X workspace, the plane / block tables of
// B images (resident afterwards: upload_tables).  A pipe calls it for every sub-batch size of a submission before any
// transfer is in flight, so that nothing synchronises or allocates once its threads and streams are busy.
struct EncodePlan {
    ImageGeom g;
    Tables t;
    BcdPlan bcd; // of the call that initialises and iterates (first_mode 1)
    long u_img = 0, v_img = 0, uoff[3], voff[3], u0c[4] = {0, 0, 0, 0}, v0c[4] = {0, 0, 0, 0};
};
// upload false: the caller uploads the tables itself (lrf_qmf_encode_rgb_u8, behind plan_x_residency, which marks blocks).
int encode_rgb_prepare(lrf_ctx* c, int64_t B, int64_t H, int64_t W, const int R[3], int K, int lo, int hi, bool with_sign, bool fuse_gram,
                       EncodePlan& ep, bool upload = true);
// B equal matrices [M,64]: the bodies of lrf_qmf_decompose_f32 (R <= LRF_MAX_RANK) and lrf_qmf_bcd_f32 (R <= LRF_BIG_TO_ANY_RANK)
// for N = 64, shared with lrf_qmf_encode_gray_u8 (lrf_channels.hip)
int decompose64(lrf_ctx* c, const float* X, int64_t B, int64_t M, int R, int K, int lo, int hi, const int8_t* sign, int8_t* U, int8_t* V);
int bcd64(lrf_ctx* c, const float* X, int64_t B, int64_t M, int R, int K, int lo, int hi, const float* U0, const float* V0, int8_t* U,
          int8_t* V);
// run_init then run_bcd on uploaded tables (upload_tables): what every entry that initialises and iterates at once ends in
int init_then_bcd64(lrf_ctx* c, const float* X, const Tables& t, const BcdPlan& plan, const int8_t* sign, int gram_exp, int8_t* U, int8_t* V);
bool planes_gram_eligible(const uint8_t* rgb, int64_t B, int64_t H, int64_t W); // lrf_planes_gram.hip
int planes_gram_from_rgb(lrf_ctx* c, const uint8_t* rgb, int64_t H, int64_t W, const ImageGeom& g, const Tables& t, float* X, bool luma_out = true);

// ---- kernels of other translation units behind launch functions ---------------------------------------------------------
// one BCD half-iteration of a run (U update + partials of the V update): what every family's kernel takes
struct BcdLaunch {
    const float* X;
    const PlaneDesc* pl;
    const BlockDesc* bl; // the run's first block
    int nblocks;
    const float *vf, *wf, *bf;
    const float* U0;     // mode 2: the caller's fp32 initial U
    int8_t* U;
    float *pp, *qp;
    GsParams gp;         // exact_int set for the run
    int mode;            // 0: iterations >= 2 (old U from int8); 1: the first, old U = X W0; 2: the first, old U = U0
};
// ranks 17..32 (lrf_bcd32.hip: k_bprep_big, k_bcd_w32 / k_bcd_w32f / k_bcd_mid, k_vupdate_mid)
int bcd32_bprep(hipStream_t rs, const PlaneDesc* pl, const float* vf, float* bf, int nplanes, int plane0);
int bcd32_update_u(lrf_ctx* c, hipStream_t rs, const BcdLaunch& a, BcdChoice ch); // ch: k_bcd_mid, k_bcd_w32 or k_bcd_w32f
int bcd32_update_v(lrf_ctx* c, hipStream_t rs, const PlaneDesc* pl, const float* pp, const float* qp, float* vf, float* bf, int8_t* V, float lo,
                   float hi, int last, int nplanes, int plane0);
// the plan's persistent launch (lrf_bcd_persist.hip: k_bcd_p<F16, NP32, FIRST>): iterations 2..K of a whole call, or all K
int bcdp_launch(lrf_ctx* c, const BcdPlan& plan, const float* X, const PlaneDesc* pl, const BlockDesc* bl, int nblocks, int nplanes, int plane0,
                const FamBufs& t16, const FamBufs& t64, int8_t* U, int8_t* V, GsParams gp);

// ---- the any-shape path (lrf_any.hip: other patch sizes, patch=False, the RGB colour space, ranks 33..64 of the 64-column path)
int any_workspace(lrf_ctx* c, int B, int M, int N, int R);
int any_run_bcd_ex(lrf_ctx* c, const float* X, long x_batch, int B, int M, int N, int R, int K, int lo, int hi, int8_t* U, long u_batch,
                   int8_t* V, long v_batch);
int any_decompose(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, int K, int lo, int hi, const int8_t* sign, int8_t* U,
                  int8_t* V);
int any_bcd(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, int K, int lo, int hi, const float* U0, const float* V0,
            int8_t* U, int8_t* V);
int any_svd_init(lrf_ctx* c, const float* X, int64_t B, int64_t M, int64_t N, int R, const int8_t* sign, float* U0, float* V0);
#endif
