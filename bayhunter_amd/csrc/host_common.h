// host_common.h -- what the host side of the library shares between its translation units: the error channel, the
// device check, the LDS limit and the prototypes of the internal functions one file defines and another calls.  Each
// is declared here and nowhere else.  No HIP header: chains.cpp is a plain C++ translation unit.
#pragma once
#include <cstddef>
#include <vector>
#include "../../include/bayhunter_amd.h"

// a failed HIP call ends the enclosing function with BH_ERR_HIP and the call's text in bh_last_error (used where HIP
// is included anyway)
#define BH_HIP(call)                                                         \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return bh::fail_hip_((int)e_, #call);          \
    } while (0)

namespace bh {

constexpr size_t kLdsLimit = 160 * 1024;        // LDS of a CU: the most a workgroup's launch may ask for

// capi.hip.  The message goes to the calling thread's bh_last_error; the return value is the error code.
__attribute__((visibility("hidden"))) int fail_(int code, const char *what);   // `code`, any BH_ERR_*; not exported
int fail_arg_(const char *what);                // BH_ERR_ARG
int fail_hip_(int e, const char *what);         // BH_ERR_HIP, `e` a hipError_t: "<what>: <hipGetErrorString(e)>"
int require_device();                           // BH_OK, or BH_ERR_NO_DEVICE (there is no CPU fallback)

struct Scratch {  // per-thread device scratch for the synchronous single-model calls (bh_surfdisp96, bh_synrf)
    void *p = nullptr;
    size_t n = 0;
    int dev = -1;
    int ensure(size_t bytes);
};
extern thread_local Scratch g_scratch;

// rf_capi.hip.  bh_rf_batch's parameter checks: bh_forward_batch (evalplan.hip) makes them before its first launch
int check_rf_params(const bh_rf_params *par, int Lmax, int out_stride, bool zr);
// rf_capi.hip.  The two cached device tables of a receiver-function launch (FFT twiddles; per-frequency constants) for
// the launch constants P of rf_fill_launch: rf_sens_capi.hip launches with the tables bh_rf_batch's launches read.  The
// frequency table stays pinned in its cache until the RfTables object goes.
struct RfLaunch;
struct RfTables {
    const double *tw = nullptr, *ftab = nullptr;
    void *pin = nullptr;
    RfTables() = default;
    RfTables(const RfTables &) = delete;
    RfTables &operator=(const RfTables &) = delete;
    ~RfTables();
};
int rf_get_tables(const RfLaunch &P, double fsamp, RfTables *tables);

// like_capi.hip: the kept-sample tables of a set_present mask (evalplan.hip: bh_eval_set_gaps), and the likelihood of
// observation sets with or without data gaps (bh_likelihood_sets, bh_likelihood_sets_gaps; evalplan.hip)
int like_gaps_derive(const char *who, int nsets, int set_stride, int ntargets, const bh_like_target *targets,
                     const unsigned char *set_present, std::vector<int> &tables, bool *any_gap);
int likelihood_sets_(int stages, int B, int ntargets, const bh_like_target *targets, const double *out, int out_stride,
                     const int *err, int nflags, int nsets, const int *obs_id, const double *yobs, int set_stride,
                     const double *set_scale, const double *set_logdet, const double *noise, const double *aux,
                     double *logL, double *misfits, void *workspace, size_t workspace_bytes,
                     const unsigned char *set_present, void *gaps_workspace, size_t gaps_workspace_bytes,
                     const int *gap_cols, const int *gap_cnt, void *stream);

}  // namespace bh
