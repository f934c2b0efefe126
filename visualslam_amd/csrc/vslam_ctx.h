// The context of the C ABI and the pieces every translation unit of the library shares: error plumbing, the bench
// timing hook's scope object, and the interface of the side-stream scheduling unit (vslam_sched.cpp; its decisions are
// in vslam_sched_policy.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <deque>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/vslam.h"
#include "vslam_sched_policy.h"

// Diagnostic environment switches (the reference paths of VSLAM_HDIFF and VSLAM_ORIENT_SCALAR) exist only in a build with
// -DVSLAM_DIAGNOSTICS (lib/libvslam_diag.so, `make diag`): the shipped library never reads them.
#ifdef VSLAM_DIAGNOSTICS
#define VSLAM_DIAG_ENV(name) std::getenv(name)
#else
#define VSLAM_DIAG_ENV(name) (static_cast<const char*>(nullptr))
#endif

struct vslam_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // Every stream and event created for this context (own_stream / own_event in vslam_sched.cpp), the context's own main
    // stream included: vslam_ctx_destroy destroys what is listed here and nothing else.  Every other handle below is borrowed.
    vslam::Owned<hipStream_t> streams;
    vslam::Owned<hipEvent_t> events;
    std::string err;
    // bump workspace in HBM, grown between calls only (never inside a launch sequence)
    char* ws = nullptr;
    size_t ws_cap = 0;
    // device copies of the tap tables, each made once (get_table in vslam_hip.hip): (TableKind, bits of sigma or sigma0,
    // kernel width or octave) -> quantised taps / StripTaps / PyrTaps<CFG> / MxTaps<CFG> / f32 Gaussian taps
    std::map<std::tuple<int, uint64_t, int>, void*> tables;
    // OPT-IN matrix-core form of the LDS-tiled octave kernels (VSLAM_MX=1 / vslam_ctx_set_matrix_path): never the default
    bool mx = false;
    // vslam_ctx_set_f32_fused / VSLAM_F32_FUSED=1: the f32 stages (separable f32 filter of filterKeypoints / SIFT, the arctangent of
    // processGradients) with fused multiply-adds, as an OpenCV that dispatches its AVX2 + FMA3 code computes them (default: every
    // product and sum rounded, OpenCV's SSE2 baseline)
    bool f32_fused = false;
    bool orient_scalar_form = false;  // VSLAM_ORIENT_SCALAR=1: k_orient_survivors for every octave (the round-3 form, kept for comparison)
    // auxiliary streams of the batched path: the HBM-bound chains (Harris; extrema + compaction)
    // run beside the VALU-bound pyramid kernels; forked from / joined to `stream` by events
    // aux[2] carries only the second-half upsample of a large batch (enqueue_dog): it must not queue behind
    // the previous chunk's list chain on aux[1]
    static constexpr int kAux = 3;
    hipStream_t aux[kAux] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kAux] = {nullptr, nullptr, nullptr}, ev_oct[VSLAM_MAX_OCTAVES] = {};
    int prio_dev_lo = 0;  // the device's lowest stream priority (0: it has no priority levels)
    vslam::PairSlots<hipStream_t> pairs;  // the side-stream pairs in existence; aux[0], aux[1] are one of them
    vslam::StreamTuner tuner;  // which pair of side streams the batched path runs on (vslam_sched_policy.h)
    hipEvent_t tuner_ev[vslam::StreamTuner::M][2] = {};  // start, end of each timed call
    vslam::JoinWatch watch;  // steps the side streams down when their join lags (vslam_sched_policy.h)
    hipEvent_t watch_ev[vslam::JoinWatch::RING][3] = {};  // start, own work enqueued, end of each measured call
    hipEvent_t ev_phase = nullptr;  // recorded by every vslam_detect_batch_dev call once its octave-0 kernels are enqueued (vslam_ctx_follow)
    bool phase_marked = false;
    hipEvent_t ev_up2 = nullptr;  // the second half of a batch has been upsampled (enqueue_dog)
    hipEvent_t ev_chunk = nullptr;  // the main-stream kernels of a chunk (the readers of the octave bases) are enqueued up to here
    // matrix path, fused lattice scan: the side stream's k_extrema_pack launches of a chunk have read the site / seam maps
    // (the one scratch of the DoG path written on the main stream and read on a side stream: the next chunk's octave
    // kernels wait for this before they overwrite it)
    hipEvent_t ev_pack = nullptr;
    hipEvent_t ev_list0 = nullptr, ev_edge = nullptr;  // octave 0's part of the DoG list is written / its edge test is done
    hipEvent_t ev_or_fork = nullptr, ev_or_join[2] = {nullptr, nullptr};  // the orientation launches spread over the idle side streams (enqueue_orient_batch)
    // recycled pyramid blocks: a GaussPyramid per image would otherwise pay hipMalloc + hipFree of
    // >100 MB each time (milliseconds, more than the kernels)
    std::vector<std::pair<size_t, void*>> block_cache;
    // kernels whose dynamic-LDS ceiling has been raised on this device (once, not per launch)
    std::set<const void*> lds_raised;
    float* loc_lut = nullptr;  // FeaturePointLocalization table (kernels_localize.hip.h), built on first use
    uint8_t* dump = nullptr;   // 256 bytes nobody reads: where the Harris kernel's margin lanes store in its steady rows
    // bench timing hook
    std::string timing_name;
    int launch_tag = -1;  // octave of the launch being enqueued, for helpers that do not get it as an argument
    int timing_tag = -1;  // "name@N": only launches tagged N (the octave)
    std::deque<std::pair<hipEvent_t, hipEvent_t>> timing_ev;  // (a deque: a TimedScope keeps a pointer to its slot while later scopes append)
    size_t timing_used = 0;
};

static inline int fail(vslam_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(ctx, e_ == hipErrorOutOfMemory ? VSLAM_ERR_NOMEM : VSLAM_ERR_HIP,        \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                     \
    } while (0)

#define ARGCHK(ctx, cond, msg) \
    if (!(cond)) return fail(ctx, VSLAM_ERR_INVALID, msg)
#define TRY(expr)              \
    do {                       \
        int rc_ = (expr);      \
        if (rc_) return rc_;   \
    } while (0)

static inline int bind_device(vslam_ctx* c) {
    if (!c) return VSLAM_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return VSLAM_OK;
}

// ---- vslam_sched.cpp: the owner of the context's streams and events, the fork / join of a batch call, the timing hook
namespace vslam {
void sched_init_from_env(vslam_ctx* c);  // VSLAM_JOIN_WATCH, VSLAM_SIDE_PRIORITY, VSLAM_STREAM_TUNER (vslam_ctx_create)
int own_stream(vslam_ctx* c, int priority, hipStream_t* out);  // non-blocking; priority 0: the default one
int own_event(vslam_ctx* c, unsigned flags, hipEvent_t* out);
void sched_destroy(vslam_ctx* c);  // waits for every stream of the context, then destroys every handle it owns (vslam_ctx_destroy)
int sched_mark_phase(vslam_ctx* c);  // records ev_phase on the current stream (vslam_ctx_follow)
std::pair<hipEvent_t, hipEvent_t>* timing_slot(vslam_ctx* c);

// The fork and join of one vslam_detect_batch_dev call.  begin: the side streams exist (created on the context's first
// call), the watchdog and the tuner have had their say, and - unless the watchdog is at level 2 - aux[] wait for the main
// stream.  end (the main stream's own work is enqueued): aux[] are joined back, the call's measurements are closed.  A call
// that returns early in between leaves the scope with the fork open: the side streams are drained, so that they cannot run
// into buffers the caller (or the next ws_reserve) reuses.
struct BatchFork {
    vslam_ctx* c;
    bool side = false;  // the call has side streams
    bool open = false;
    // `eligible`: a full-size batch with both paths (what the tuner compares); `big`: one the watchdog measures too
    int begin(unsigned long long key, bool eligible, bool big, bool capturing);
    int end();
    ~BatchFork();
};
}  // namespace vslam

// Brackets the launches made inside its scope with HIP events on the context stream when the
// bench hook (vslam_kernel_timing_enable) names this kernel.
struct TimedScope {
    vslam_ctx* c;
    std::pair<hipEvent_t, hipEvent_t>* ev;
    hipStream_t st;
    // `tag`: the octave of the launch (-1: none) - "name@2" times only the launches tagged 2; `stream`: where the launch
    // goes when that is not the context's current stream (the scans go straight to the side stream)
    TimedScope(vslam_ctx* ctx, const char* name, int tag = -1, hipStream_t stream = nullptr)
        : c(ctx), ev(!ctx->timing_name.empty() && ctx->timing_name == name && (ctx->timing_tag < 0 || ctx->timing_tag == tag) ? vslam::timing_slot(ctx) : nullptr),
          st(stream ? stream : ctx->stream) {
        if (ev) (void)hipEventRecord(ev->first, st);
    }
    ~TimedScope() {
        if (ev) (void)hipEventRecord(ev->second, st);
    }
};
