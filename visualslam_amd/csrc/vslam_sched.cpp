// The owner of a context's streams and events, the fork / join of a batch call (side-stream placement, the join watchdog:
// the decisions themselves are in vslam_sched_policy.h) and the bench timing hook: host-side scheduling code only, no
// kernels.  Kept apart from the C ABI / launch plan (vslam_hip.hip).
#include "vslam_ctx.h"

#include <algorithm>

namespace vslam {

// ---- the owner -------------------------------------------------------------------------------------------------------
// Every stream and event of a context is created here and listed once (vslam_ctx::streams / events); teardown destroys
// the lists, an early release takes the handle off its list first.  Nothing else creates or destroys a handle.
int own_stream(vslam_ctx* c, int priority, hipStream_t* out) {
    if (priority == 0 || hipStreamCreateWithPriority(out, hipStreamNonBlocking, priority) != hipSuccess) {
        (void)hipGetLastError();  // priorities are a speed matter only
        HIPCHK(c, hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    }
    c->streams.add(*out);
    return VSLAM_OK;
}
int own_event(vslam_ctx* c, unsigned flags, hipEvent_t* out) {
    HIPCHK(c, flags ? hipEventCreateWithFlags(out, flags) : hipEventCreate(out));
    c->events.add(*out);
    return VSLAM_OK;
}
static void release(vslam_ctx* c, hipStream_t& st) {
    if (st && c->streams.remove(st)) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
    st = nullptr;
}
static void release(vslam_ctx* c, hipEvent_t& e) {
    if (e && c->events.remove(e)) (void)hipEventDestroy(e);
    e = nullptr;
}
void sched_destroy(vslam_ctx* c) {
    for (hipStream_t st : c->streams.list) (void)hipStreamSynchronize(st);  // a failed batch call may have left side-stream work un-joined
    for (hipEvent_t e : c->events.list) (void)hipEventDestroy(e);
    for (hipStream_t st : c->streams.list) (void)hipStreamDestroy(st);
}

std::pair<hipEvent_t, hipEvent_t>* timing_slot(vslam_ctx* c) {
    if (c->timing_used == c->timing_ev.size()) {
        if (c->timing_ev.size() >= 65536) return nullptr;
        hipEvent_t a = nullptr, b = nullptr;
        if (own_event(c, 0, &a) != VSLAM_OK || own_event(c, 0, &b) != VSLAM_OK) {
            release(c, a);
            return nullptr;
        }
        c->timing_ev.emplace_back(a, b);
    }
    return &c->timing_ev[c->timing_used++];
}

// vslam_ctx_follow: the point of a batch call, the end of octave 0, behind which a second context's batch may start (its
// heavy octave-0 kernels then run beside this call's remaining, shorter kernels instead of beside its own octave 0).
int sched_mark_phase(vslam_ctx* c) {
    if (!c->ev_phase) TRY(own_event(c, hipEventDisableTiming, &c->ev_phase));
    HIPCHK(c, hipEventRecord(c->ev_phase, c->stream));
    c->phase_marked = true;
    return VSLAM_OK;
}

// ---- carrying out what the policy (vslam_sched_policy.h) decides ----------------------------------------------------
// The call runs on the pair in `slot`, created now if the slot is empty (while the other pairs exist: it binds to another queue).
static int use_pair(vslam_ctx* c, int slot, int priority) {
    for (int i = 0; i < 2; ++i) {
        if (!c->pairs.h[slot][i]) TRY(own_stream(c, priority, &c->pairs.h[slot][i]));
        c->aux[i] = c->pairs.h[slot][i];  // the pair being left is idle: every call joins its side streams back
    }
    return VSLAM_OK;
}

static void tuner_finish(vslam_ctx* c, int chosen) {
    c->tuner.finish(chosen);
    c->pairs.keep(chosen, [c](hipStream_t& st) { release(c, st); });  // the losers are idle: every measured call has joined them back
    (void)use_pair(c, kLevel0, 0);  // (live: nothing is created)
    for (auto& pr : c->tuner_ev)
        for (hipEvent_t& e : pr) release(c, e);
}

// Before the fork of a batch call (ensure_aux has run): picks the pair of side streams this call uses.  Never blocks.
static int tuner_before_call(vslam_ctx* c, unsigned long long key, bool eligible, bool capturing) {
    StreamTuner& t = c->tuner;
    switch (t.before_call(c->watch.level, c->prio_dev_lo != 0, capturing, key, eligible)) {
    case StreamTuner::kIdle: break;
    case StreamTuner::kGiveUp: tuner_finish(c, 0); break;
    case StreamTuner::kFirstPair: TRY(use_pair(c, kLevel0, c->prio_dev_lo)); break;
    case StreamTuner::kMeasure: {
        hipEvent_t* ev = c->tuner_ev[t.measured];
        TRY(use_pair(c, c->pairs.of_candidate(StreamTuner::pair_of(t.measured)), c->prio_dev_lo));
        for (int j = 0; j < 2; ++j)
            if (!ev[j]) TRY(own_event(c, 0, &ev[j]));
        HIPCHK(c, hipEventRecord(ev[0], c->stream));
        t.started();
        break;
    }
    case StreamTuner::kDecide: {  // once the last measured call has finished - until then on the first pair
        TRY(use_pair(c, kLevel0, c->prio_dev_lo));
        const hipError_t q = hipEventQuery(c->tuner_ev[StreamTuner::M - 1][1]);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            break;
        }
        float ms[StreamTuner::M] = {};
        bool ok = q == hipSuccess;
        for (int m = 0; m < StreamTuner::M && ok; ++m) ok = hipEventElapsedTime(&ms[m], c->tuner_ev[m][0], c->tuner_ev[m][1]) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        tuner_finish(c, StreamTuner::choose(ok, ms));
        break;
    }
    }
    return VSLAM_OK;
}

// Before the fork of a batch call: reads finished measurements, moves between the levels, starts this call's measurement.
static int watch_before_call(vslam_ctx* c, unsigned long long key, bool eligible, bool capturing) {
    JoinWatch& w = c->watch;
    const int level = w.level;
    const auto follow = [&]() -> int {  // the policy has moved to another level: its pair (levels 0 and 1) is the one in use now
        if (w.level == level || w.level > 1) return VSLAM_OK;
        return use_pair(c, c->pairs.of_level(w.level), w.level == 0 ? c->prio_dev_lo : 0);
    };
    if (!w.before_call(key, eligible, capturing, c->tuner.busy())) return follow();
    for (int i = 0; i < JoinWatch::RING; ++i) {
        if (!w.live[i]) continue;
        hipEvent_t* ev = c->watch_ev[i];
        const hipError_t q = hipEventQuery(ev[2]);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            continue;
        }
        float total = 0.0f, lag = 0.0f;
        const bool ok = q == hipSuccess && hipEventElapsedTime(&total, ev[0], ev[2]) == hipSuccess && hipEventElapsedTime(&lag, ev[1], ev[2]) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        w.measured(i, ok, total, lag);
    }
    w.decide();
    TRY(follow());
    const int slot = w.start(eligible);
    if (slot < 0) return VSLAM_OK;
    for (hipEvent_t& e : c->watch_ev[slot])
        if (!e) TRY(own_event(c, 0, &e));
    HIPCHK(c, hipEventRecord(c->watch_ev[slot][0], c->stream));
    return VSLAM_OK;
}

// The side streams and the fork / join events, on the context's first batch call.  (Queue placement depends on the order
// of creation, DESIGN section 5.4: everything is created here, in this order, whether the call will use it or not.)
static int ensure_aux(vslam_ctx* c) {
    if (c->ev_fork) return VSLAM_OK;
    int prio_lo = 0, prio_hi = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) {  // numerically: lowest priority, highest priority
        (void)hipGetLastError();  // priorities are a speed matter only: do not leave the error for the next launch check
        prio_lo = 0;
    }
    c->prio_dev_lo = prio_lo;
    c->watch.device(prio_lo != 0);
    hipStream_t* pair = c->pairs.h[c->pairs.of_level(c->watch.level)];  // (a context pinned to level 2 never uses it)
    for (int i = 0; i < vslam_ctx::kAux; ++i) {
        // aux[0], aux[1] (Harris chain, scans and lists) yield to the octave kernels; aux[2] carries only the
        // second-half upsample, which the main stream WAITS for: at low priority it was starved for the whole
        // first-half octave kernel whenever its start slipped behind that kernel's (C++ host, 0.35 ms per step)
        TRY(own_stream(c, i < 2 && c->watch.level == 0 ? prio_lo : 0, &c->aux[i]));
        if (i < 2) pair[i] = c->aux[i];
        TRY(own_event(c, hipEventDisableTiming, &c->ev_join[i]));
    }
    for (auto& e : c->ev_oct) TRY(own_event(c, hipEventDisableTiming, &e));
    for (hipEvent_t* e : {&c->ev_up2, &c->ev_chunk, &c->ev_pack, &c->ev_list0, &c->ev_edge, &c->ev_or_fork, &c->ev_or_join[0], &c->ev_or_join[1], &c->ev_fork})
        TRY(own_event(c, hipEventDisableTiming, e));
    return VSLAM_OK;
}

int BatchFork::begin(unsigned long long key, bool eligible, bool big, bool capturing) {
    TRY(ensure_aux(c));
    // (calls of a few megapixels are dominated by launch latencies: their lag says nothing about starvation)
    TRY(watch_before_call(c, key, eligible && big, capturing));
    side = c->watch.level != 2;  // the watchdog's last step: everything on the caller's stream
    if (!side) return VSLAM_OK;
    TRY(tuner_before_call(c, key, eligible, capturing));
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    for (hipStream_t st : c->aux) HIPCHK(c, hipStreamWaitEvent(st, c->ev_fork, 0));
    open = true;
    return VSLAM_OK;
}

int BatchFork::end() {
    if (c->watch.recording >= 0) HIPCHK(c, hipEventRecord(c->watch_ev[c->watch.recording][1], c->stream));  // the main stream's own work ends here
    if (side)
        for (int i = 0; i < vslam_ctx::kAux; ++i) {
            HIPCHK(c, hipEventRecord(c->ev_join[i], c->aux[i]));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join[i], 0));
        }
    if (c->watch.recording >= 0) {
        HIPCHK(c, hipEventRecord(c->watch_ev[c->watch.recording][2], c->stream));
        c->watch.recorded();
    }
    if (!c->phase_marked) TRY(sched_mark_phase(c));  // no DoG path in this call: its end is the mark
    if (side && c->tuner.measuring >= 0) {
        HIPCHK(c, hipEventRecord(c->tuner_ev[c->tuner.measuring][1], c->stream));
        c->tuner.after_call();
    }
    open = false;
    return VSLAM_OK;
}

BatchFork::~BatchFork() {
    if (!open) return;
    for (hipStream_t st : c->aux)
        if (st) (void)hipStreamSynchronize(st);
    (void)hipStreamSynchronize(c->stream);
}

void sched_init_from_env(vslam_ctx* c) {
    const char* jw = std::getenv("VSLAM_JOIN_WATCH");
    c->watch.disabled = jw && jw[0] == '0';
    if (const char* sp = std::getenv("VSLAM_SIDE_PRIORITY")) c->watch.level = (sp[0] == 'l' || sp[0] == 'L') ? 0 : 1;  // low | main
    const char* t = std::getenv("VSLAM_STREAM_TUNER");
    if (t && t[0] == '1') (void)vslam_ctx_tune_side_streams(c, 1);
}

}  // namespace vslam

using namespace vslam;

extern "C" {

int vslam_kernel_timing_enable(vslam_ctx* c, const char* name) {
    if (!c) return VSLAM_ERR_INVALID;
    c->timing_name = name ? name : "";
    c->timing_tag = -1;
    const size_t at = c->timing_name.find('@');  // "k_pyr_octave@1": the launches of octave 1 only
    if (at != std::string::npos) {
        c->timing_tag = std::atoi(c->timing_name.c_str() + at + 1);
        c->timing_name.resize(at);
    }
    c->timing_used = 0;
    return VSLAM_OK;
}
int vslam_kernel_timing_read(vslam_ctx* c, int* launches, double* total_ms) {
    TRY(bind_device(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // every batch call joins its side streams back: their events are complete too
    double tot = 0;
    for (size_t i = 0; i < c->timing_used; ++i) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->timing_ev[i].first, c->timing_ev[i].second));
        tot += ms;
    }
    if (launches) *launches = (int)c->timing_used;
    if (total_ms) *total_ms = tot;
    c->timing_used = 0;
    return VSLAM_OK;
}

int vslam_ctx_side_stream_report(const vslam_ctx* c, int* pair, int* state) {
    if (!c) return VSLAM_ERR_INVALID;
    if (pair) *pair = c->tuner.chosen;
    if (state) *state = c->tuner.state();
    return VSLAM_OK;
}

int vslam_ctx_set_side_stream_priority(vslam_ctx* c, int low) {
    if (!c) return VSLAM_ERR_INVALID;
    if (c->ev_fork) return fail(c, VSLAM_ERR_UNSUPPORTED, "set_side_stream_priority: the side streams exist already - call it before the context's first batch call");
    if (!c->watch.pinned) c->watch.level = low ? 0 : 1;
    return VSLAM_OK;
}

int vslam_ctx_join_watch_report(const vslam_ctx* c, int* level, int* done, float* last_lag_fraction) {
    if (!c) return VSLAM_ERR_INVALID;
    if (level) *level = c->watch.level;
    if (done) *done = c->watch.done ? 1 : 0;
    if (last_lag_fraction) *last_lag_fraction = c->watch.last_lag_frac;
    return VSLAM_OK;
}

int vslam_ctx_tune_side_streams(vslam_ctx* c, int on) {
    if (!c) return VSLAM_ERR_INVALID;
    if (c->tuner.done) return VSLAM_OK;  // a finished comparison stays finished
    if (on && c->ev_fork)  // (the watchdog has cached the pair in use by then, and the pairs compared are created beside it)
        return fail(c, VSLAM_ERR_UNSUPPORTED, "tune_side_streams: the side streams exist already - call it before the context's first batch call");
    c->tuner.enabled = on != 0;
    // the comparison is between pairs of YIELDING streams: asking for it asks for those (a pinned level stays; the tuner then ends at
    // its first call and the join watchdog runs as if it had never been asked)
    if (on && !c->watch.pinned) c->watch.level = 0;
    return VSLAM_OK;
}

int vslam_ctx_set_join_watch(vslam_ctx* c, int on) {
    if (!c) return VSLAM_ERR_INVALID;
    c->watch.disabled = on == 0;
    return VSLAM_OK;
}

int vslam_ctx_pin_side_streams(vslam_ctx* c, int level) {
    if (!c || level < 0 || level > 2) return VSLAM_ERR_INVALID;
    if (c->ev_fork) return fail(c, VSLAM_ERR_UNSUPPORTED, "pin_side_streams: the side streams exist already - call it before the context's first batch call");
    c->watch.level = level;
    c->watch.done = c->watch.pinned = true;
    return VSLAM_OK;
}

}  // extern "C"
