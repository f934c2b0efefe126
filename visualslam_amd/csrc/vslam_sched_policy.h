// The decisions of the side-stream scheduling, apart from HIP: which handles a context owns, which slot holds which
// pair of side streams, the join watchdog's levels and trials, the opt-in tuner's order and choice.  No HIP header is
// included: vslam_sched.cpp turns events into (total, lag) figures, hands them over and carries out what comes back;
// tests/test_sched_policy_cpu.py plays scripts through the same code with integers as handles.
#pragma once
#include <algorithm>
#include <vector>

namespace vslam {

// Every stream and every event created for a context is recorded here once; everything else (aux[], the pair slots,
// the named events, the rings) only borrows the handle.  Teardown destroys what is listed; an early release removes
// the entry first, so teardown cannot see it again.
template <class H>
struct Owned {
    std::vector<H> list;
    void add(H h) { list.push_back(h); }
    bool remove(H h) {
        const auto it = std::find(list.begin(), list.end(), h);
        if (it == list.end()) return false;
        list.erase(it);
        return true;
    }
};

// The pairs of side streams a context can hold at one time.  The pair created on the first batch call sits in the
// slot of the level the context starts at; the watchdog fills the other level's slot when a trial needs it (both
// stay until the context goes), the tuner fills the candidate slots while it compares.
enum PairSlot { kLevel0 = 0, kLevel1 = 1, kCand1 = 2, kCand2 = 3, kPairSlots = 4 };
template <class H>
struct PairSlots {
    H h[kPairSlots][2] = {};
    bool live(int s) const { return h[s][0] != H(); }
    static int of_level(int level) { return level == 0 ? kLevel0 : kLevel1; }  // (level 2 runs without side streams)
    static int of_candidate(int k) { return k == 0 ? kLevel0 : kCand1 + k - 1; }  // the tuner compares yielding pairs: candidate 0 IS the level-0 pair
    // The end of the tuner's comparison: the pairs that lose are released (release(handle) empties the slot; an empty one is
    // passed too), and the survivor becomes the level-0 pair.
    template <class F>
    void keep(int chosen, F&& release) {
        const int win = of_candidate(chosen);
        for (int s : {(int)kLevel0, (int)kCand1, (int)kCand2})
            if (s != win) release(h[s][0]), release(h[s][1]);
        if (win != kLevel0)
            for (int i = 0; i < 2; ++i) h[kLevel0][i] = h[win][i], h[win][i] = H();
    }
};

// ---- side-stream placement: the opt-in tuner ----------------------------------------------------------------------
// HIP binds every stream to one of GPU_MAX_HW_QUEUES hardware queues per priority level, and the placement is not ours to
// choose.  Measured: depending on the queue a LOW-priority side stream lands on, the batch runs up
// to 20 % slower (the same binary: 11.4 k frames/s with 3 queues per level, 14.2 k with 12) - on one bad queue the side
// kernels crawl while the main stream's queue sits on the barrier that waits for them.  A host that wants the library to
// look for a better pair OPTS IN (vslam_ctx_tune_side_streams; `Stream --tuner`): the 2nd to 5th full-size batch
// call of the context then run on three candidate pairs of side streams (the first pair twice), each call bracketed by two
// events on the main stream, and the first later call that finds all of them complete (hipEventQuery: the entry point stays
// asynchronous, nothing waits on the host) adopts the fastest pair - the first one unless another is at least 3 % faster.
// Only calls of one shape are compared (calls of another shape, small or odd calls run on the pair in use and do not
// disturb the comparison; a caller whose full-size shape keeps changing ends it on the first pair after three restarts);
// nothing is timed while the stream is being captured.  Results never depend on the streams a call runs on.
struct StreamTuner {
    static constexpr int K = 3;      // candidate pairs
    static constexpr int M = K + 1;  // measured calls: pair 0, 1, 2, 0
    enum Act {
        kIdle,       // this call runs on the pair in use
        kFirstPair,  // another shape: start over, on pair 0
        kMeasure,    // time this call in slot `measured`, on pair pair_of(measured)
        kDecide,     // every candidate has been timed: on pair 0; choose() once the last timed call has finished
        kGiveUp      // the shape keeps changing: finish(0)
    };
    int measured = 0;         // calls measured so far
    int measuring = -1;       // slot being measured by the current call
    bool enabled = false;     // vslam_ctx_tune_side_streams (or VSLAM_STREAM_TUNER=1 when the context was created)
    bool done = false;
    int chosen = 0;
    unsigned long long key = 0;  // shape of the calls being compared (0: none yet)
    int calls = 0, resets = 0;

    static int pair_of(int slot) { return slot == K ? 0 : slot; }
    bool busy() const { return enabled && !done; }  // the join watchdog sleeps meanwhile
    int state() const { return done ? 2 : ((enabled && calls > 1) ? 1 : 0); }  // vslam_ctx_side_stream_report

    // Before the fork of a batch call that has side streams.  `level`: the watchdog's; `has_prio`: the device has priority levels.
    Act before_call(int level, bool has_prio, bool capturing, unsigned long long k, bool eligible) {
        if (done || !enabled) return kIdle;
        if (level > 0 || !has_prio) {  // the pairs it compares are yielding ones: at the main stream's priority, or where one pair is
            done = true;               // as good as another, there is nothing to compare, and the join watchdog must not wait for a verdict
            return kIdle;
        }
        if (capturing) return kIdle;  // a captured call records no timing events and runs on the pair in use
        ++calls;
        if (calls == 1 || !eligible) return kIdle;  // the first call pays one-time costs; small / odd calls are not what is being tuned
        if (key == 0) key = k;
        if (k != key) {  // another full-size shape: start over with it (the pairs created so far stay), but not for ever
            if (++resets > 3) return kGiveUp;
            key = k;
            measured = 0;
            return kFirstPair;
        }
        return measured < M ? kMeasure : kDecide;
    }
    void started() { measuring = measured; }  // the call's first event is recorded
    void after_call() {
        if (measuring >= 0) measuring = -1, ++measured;
    }
    // `ok`: every timed call's events could be read.  Pair 0 was timed twice (the early calls run on cold clocks).
    static int choose(bool ok, const float ms[M]) {
        int best = 0;
        if (ok) {
            const float first = std::min(ms[0], ms[K]);
            float best_ms = first;
            for (int k = 1; k < K; ++k)
                if (ms[k] < 0.97f * first && ms[k] < best_ms) best = k, best_ms = ms[k];
        }
        return best;
    }
    void finish(int k) { chosen = k, done = true, measuring = -1; }
};

// ---- side-stream priority and the join watchdog (round 5) ---------------------------------------------------------
// The batched path's two side streams (Harris chain; scans and lists) may run at the LOWEST stream priority, so that they
// yield to the octave kernels, or at the main stream's.  Which is faster is decided by the hardware queue each stream
// happens to land on (HIP multiplexes streams onto GPU_MAX_HW_QUEUES queues per priority level, default 4; DESIGN section
// 5.4).  Same box, C++ host, device-resident, frames/s with 2 / 3 / 4 / 6 / 12 queues: yielding 14.1 k / 11.5 k / 13.4 k /
// 14.0 k / 14.0 k, same priority 13.7 k / 13.7 k / 14.0 k / 13.7 k / 14.2 k - yielding wins 2-3 % on a lucky layout and
// loses 18 % on an unlucky one (a low-priority queue behind the main queue's barrier packet crawls), same priority never
// moves more than 3.5 %.  The default is therefore the SAME priority (level 1): a caller that embeds the library in a
// process with streams of its own gets a sane schedule with HIP's default queue count, without setting an environment
// variable or opting in to anything.  A host that owns its queue layout asks for yielding streams (level 0) with
// vslam_ctx_set_side_stream_priority / VSLAM_SIDE_PRIORITY=low (Stream's host-fed mode, which also asks for 12 queues).
//
// The watchdog keeps either choice honest.  The first full-size batch calls of a context are bracketed by three events on
// the main stream - start, "my own kernels are enqueued up to here" (just before the waits on the side streams' join
// events) and end.  t(end) - t(own) is how long the main stream sat waiting for side work: 0.4 % of an 18 ms batch when
// the side streams run freely, 5 % with yielding streams on four queues, 20 % when one of them is being starved.  A later
// call reads the events once they are complete (hipEventQuery: nothing ever waits on the host).  Three measured calls with
// a median lag above the level's limit (3 % at level 0, 10 % at level 1) start a TRIAL of the next level - same priority,
// then no side streams at all (level 2) - and the trial is kept only if its fastest call beats the previous level's fastest
// by 1 %; otherwise the context goes back.  Either way the watch ends after at most ten measured calls.  Off while a capture
// is on, while the opt-in tuner is comparing pairs, and under VSLAM_JOIN_WATCH=0; vslam_ctx_pin_side_streams pins a level.
// Results never depend on the level.
struct JoinWatch {
    static constexpr int RING = 4, NEED = 3;
    bool live[RING] = {};       // events of slot i are recorded and not yet read
    int head = 0;               // next slot to record
    int recording = -1;         // slot of the call being enqueued
    int calls = 0;              // eligible calls at the current level (the first is not measured)
    int n_meas = 0;             // measurements at the current level
    float lag[NEED] = {}, best_total = 0.0f;
    float level_best[3] = {0.0f, 0.0f, 0.0f};  // fastest measured call at each level tried
    int level = 1;              // 0: low-priority (yielding) side streams, 1: the main stream's priority, 2: no side streams
    int trial_from = -1;        // the level a running trial came from (-1: the current level is not a trial)
    unsigned long long key = 0; // shape of the calls being measured (only calls of one shape are compared)
    int restarts = 0;
    bool done = false, disabled = false, pinned = false;
    bool has_prio = false;      // the device has stream priority levels
    float last_lag_frac = -1.0f;

    void device(bool priority_levels) {  // the first batch call of the context
        has_prio = priority_levels;
        if (!has_prio && level == 0) level = 1;  // level 0 without priority levels IS level 1
    }
    void set_level(int l) {
        forget();  // measurements in flight belong to the form being left
        level = l;
    }
    // Before the fork of a batch call.  false: the watch sleeps through this call.  May change `level` (a trial called off).
    bool before_call(unsigned long long k, bool eligible, bool capturing, bool tuner_busy) {
        recording = -1;
        if (done || disabled || capturing || tuner_busy) return false;
        if (eligible && k != key) {  // calls of another shape: their times say nothing about the ones measured so far
            forget();
            if (key != 0 && ++restarts > 3) {  // a caller whose shape keeps changing: stop watching (a running trial ends where it started)
                if (trial_from >= 0) set_level(trial_from);
                trial_from = -1;
                done = true;
                return false;
            }
            key = k;
        }
        return true;
    }
    // The events of live slot `slot` are complete: `ok` if both times could be read (ms).
    void measured(int slot, bool ok, float total, float lag_ms) {
        live[slot] = false;
        if (!ok || !(total > 0.0f)) return;
        last_lag_frac = lag_ms / total;
        if (n_meas < NEED) {
            lag[n_meas++] = lag_ms / total;
            best_total = (best_total == 0.0f || total < best_total) ? total : best_total;
        }
    }
    // With a full window: keeps or calls off a running trial, starts the next one, or ends the watch.  May change `level`.
    void decide() {
        if (n_meas < NEED) return;
        const float a = lag[0], b = lag[1], m = lag[2];
        const float med = std::max(std::min(a, b), std::min(std::max(a, b), m));
        level_best[level] = best_total;
        if (trial_from >= 0 && !(best_total < 0.99f * level_best[trial_from])) {  // the trial did not pay: go back, stop
            set_level(trial_from);
            trial_from = -1;
            done = true;
            return;
        }
        trial_from = -1;
        const float limit = level == 0 ? 0.03f : 0.10f;
        if (level < 2 && med > limit && (level == 1 || has_prio)) {
            const int from = level;
            set_level(from + 1);
            trial_from = from;
        } else
            done = true;
    }
    // The ring slot this call is measured in, or -1.
    int start(bool eligible) {
        if (done || !eligible) return -1;
        if (++calls == 1) return -1;  // the first call of a form pays one-time costs
        if (live[head]) return -1;    // the host is more than RING calls ahead: skip this one
        recording = head;
        head = (head + 1) % RING;
        return recording;
    }
    void recorded() {  // the call's three events are on the stream
        if (recording >= 0) live[recording] = true;
        recording = -1;
    }

private:
    void forget() {
        for (bool& l : live) l = false;
        calls = n_meas = 0;
        best_total = 0.0f;
    }
};

}  // namespace vslam
