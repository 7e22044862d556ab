// lrf_env.h — the environment variables the library reads.
//
// Service knobs (every build): test hooks that move a size threshold so that small test inputs reach the large-call
// kernels, and the pipe's schedule overrides.  Read once per process.
// The first four are the launch plan's (PlanSettings, lrf_plan.h: plan_settings_env reads them, plan_bcd decides by them).
//   LRF_PERSIST              0: never k_bcd_p; 1: k_bcd_p from LRF_BCDW_MIN_BLOCKS blocks on
//   LRF_FAMILY_SPLIT_BLOCKS  blocks from which a call's rank families run on kernels of their own  (plan_splits)
//   LRF_BCDW16_MIN_BLOCKS / LRF_BCDW32_MIN_BLOCKS  blocks from which the wave kernels of ranks 9..16 / 17..32 run
//   LRF_LUMA_BYTES           0: k_bcd_p always reads luma from X; else (the default) from the image bytes in every eligible
//                            call (plan_luma_bytes, lrf_plan.h); lrf_ctx_last_luma_source says which a call took
//   LRF_X_KEEP_MB            10^6 bytes of chroma X that a k_bcd_p call of ranks <= 8 keeps on the default cache policy, the rest of its
//                            X sources streaming non-temporal (plan_x_residency, lrf_plan.h; default LRF_X_KEEP_MB_DEFAULT);
//                            a call that fits the budget as a whole is left alone; 0: no policy, every load plain;
//                            lrf_ctx_last_x_residency says what a call kept
//   LRF_DEBUG_INIT_SWEEPS   stops k_init after a stage / forces the Sturm replacement loop       (tests/test_hip_parity.py)
//   LRF_PIPE_BULK / LRF_PIPE_TAIL  the pipe's piece sizes                                          (tests/test_pipeline.py)
//   LRF_FUSED_GRAM_MIN_CHUNKS  from how many luma Gram chunks on k_planes16_gram forms the patch matrices (tests/test_fused_gram.py)
//
// Developer comparison switches (LRF_PLANES_NO_TILED, LRF_BCD_WG, LRF_NO_BCDW32, LRF_ANY_*, ...: the kernels a later one
// replaced, kept for A/B timing) exist only in a -DLRF_DEV build (`make -C lrf_amd/csrc dev` -> liblrf_hip_dev.so): in
// the shipped library dev_flag() is the constant false and the replaced paths are dead code the compiler drops.
#ifndef LRF_ENV_H
#define LRF_ENV_H
#include <stdlib.h>

inline long env_long(const char* name, long dflt)
{
    const char* e = getenv(name);
    return (e && *e) ? atol(e) : dflt;
}
#ifdef LRF_DEV
inline bool dev_flag(const char* name)
{
    const char* e = getenv(name);
    return e && e[0] == '1';
}
inline long dev_long(const char* name, long dflt) { return env_long(name, dflt); }
#else
constexpr bool dev_flag(const char*) { return false; }
constexpr long dev_long(const char*, long dflt) { return dflt; }
#endif
#endif
