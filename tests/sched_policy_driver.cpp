// Plays scripted measurements through csrc/vslam_sched_policy.h with integers as handles (tests/test_sched_policy_cpu.py).
// `Sim` is the thin part of vslam_sched.cpp without HIP: it creates and releases handles through the same Owned lists,
// keeps the pairs in the same PairSlots, and does what StreamTuner / JoinWatch return.  One line of key=value per script.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vslam_sched_policy.h"

using namespace vslam;

struct Meas {
    float total, lag_frac;
};

struct Sim {
    Owned<int> streams, events;
    PairSlots<int> pairs;
    StreamTuner t;
    JoinWatch w;
    int aux[3] = {}, watch_ev[JoinWatch::RING][3] = {}, tuner_ev[StreamTuner::M][2] = {};
    int dev_lo = -1;  // the device's lowest priority (0: no priority levels)
    bool started = false;
    // the script
    std::vector<Meas> plan[3];  // per level: what the calls measured there take, in order
    int taken[3] = {};
    float tuner_ms[StreamTuner::M] = {10, 10, 10, 10};
    bool tuner_readable = true, gpu_finishes = true;
    // the record
    int next = 1, pairs_created = 0, low_prio = 0, skipped = 0, recorded = 0, read = 0, bad_read = 0;
    std::map<int, int> released;  // handle -> times released
    Meas pending[JoinWatch::RING] = {};
    bool ready[JoinWatch::RING] = {};
    std::string path, states;

    int new_stream(int prio) {
        low_prio += prio != 0;
        streams.add(next);
        return next++;
    }
    int new_event() {
        events.add(next);
        return next++;
    }
    void release_stream(int& h) {
        if (h && streams.remove(h)) ++released[h];
        h = 0;
    }
    void release_event(int& h) {
        if (h && events.remove(h)) ++released[h];
        h = 0;
    }
    void use_pair(int slot, int prio) {
        if (!pairs.live(slot)) ++pairs_created;
        for (int i = 0; i < 2; ++i) {
            if (!pairs.h[slot][i]) pairs.h[slot][i] = new_stream(prio);
            aux[i] = pairs.h[slot][i];
        }
    }
    void tuner_finish(int chosen) {
        t.finish(chosen);
        pairs.keep(chosen, [this](int& st) { release_stream(st); });
        use_pair(kLevel0, 0);
        for (auto& pr : tuner_ev)
            for (int& e : pr) release_event(e);
    }
    void follow(int before) {
        if (w.level != before && w.level <= 1) use_pair(pairs.of_level(w.level), w.level == 0 ? dev_lo : 0);
    }
    void note_level() {
        const char c = (char)('0' + w.level);
        if (path.empty() || path.back() != c) path += c;
    }
    // one batch call of shape `key`
    void call(unsigned long long key, bool eligible = true, bool capturing = false) {
        if (!started) {  // ensure_aux
            started = true;
            w.device(dev_lo != 0);
            use_pair(pairs.of_level(w.level), w.level == 0 ? dev_lo : 0);
            aux[2] = new_stream(0);
            for (int i = 0; i < 4; ++i) new_event();  // (stands for the named events)
        }
        note_level();
        const int before = w.level;
        if (!w.before_call(key, eligible, capturing, t.busy())) {
            follow(before);
        } else {
            for (int i = 0; i < JoinWatch::RING; ++i) {
                if (!w.live[i] || !ready[i]) continue;
                ++read;
                ready[i] = false;
                w.measured(i, true, pending[i].total, pending[i].lag_frac * pending[i].total);
            }
            w.decide();
            follow(before);
            const int head = w.head;
            const int calls = w.calls;
            const int slot = w.start(eligible);
            if (slot >= 0) {
                if (ready[slot]) ++bad_read;  // a slot with an unread measurement must not be recorded over
                for (int& e : watch_ev[slot])
                    if (!e) e = new_event();
            } else if (!w.done && eligible && calls >= 1 && w.live[head])
                ++skipped;
        }
        note_level();
        const bool side = w.level != 2;
        if (side) switch (t.before_call(w.level, dev_lo != 0, capturing, key, eligible)) {
            case StreamTuner::kIdle: break;
            case StreamTuner::kGiveUp: tuner_finish(0); break;
            case StreamTuner::kFirstPair: use_pair(kLevel0, dev_lo); break;
            case StreamTuner::kMeasure:
                use_pair(pairs.of_candidate(StreamTuner::pair_of(t.measured)), dev_lo);
                for (int& e : tuner_ev[t.measured])
                    if (!e) e = new_event();
                t.started();
                break;
            case StreamTuner::kDecide:
                use_pair(kLevel0, dev_lo);
                if (gpu_finishes) tuner_finish(StreamTuner::choose(tuner_readable, tuner_ms));
                break;
            }
        // ... the call's own work, the join ...
        if (w.recording >= 0) {
            const int slot = w.recording, lv = w.level;
            const std::vector<Meas>& pl = plan[lv];
            pending[slot] = pl.empty() ? Meas{10.0f, 0.001f} : pl[taken[lv]++ % pl.size()];
            ready[slot] = gpu_finishes;
            ++recorded;
            w.recorded();
        }
        if (side) t.after_call();
        states += (char)('0' + t.state());
    }
    void gpu_catches_up() {
        gpu_finishes = true;
        for (int i = 0; i < JoinWatch::RING; ++i) ready[i] = w.live[i];
    }
    // vslam_ctx_destroy, then the line of results
    void finish(const char* name) {
        int slots_before[kPairSlots][2];
        std::memcpy(slots_before, pairs.h, sizeof slots_before);
        const int early = (int)released.size();
        for (int e : events.list) ++released[e];
        for (int s : streams.list) ++released[s];
        events.list.clear(), streams.list.clear();
        int never = 0, twice = 0;
        for (int h = 1; h < next; ++h) never += released[h] == 0, twice += released[h] > 1;
        std::printf("%s level=%d done=%d trial_from=%d path=%s pairs_created=%d low_prio=%d created=%d early=%d never=%d twice=%d "
                    "tuner_done=%d chosen=%d states=%s resets=%d cand1=%d cand2=%d aux_is_level0=%d "
                    "recorded=%d read=%d skipped=%d bad_read=%d lag=%.4f slots_touched=%d\n",
                    name, w.level, (int)w.done, w.trial_from, path.c_str(), pairs_created, low_prio, next - 1, early, never, twice,
                    (int)t.done, t.chosen, states.c_str(), t.resets, (int)pairs.live(kCand1), (int)pairs.live(kCand2),
                    (int)(aux[0] == pairs.h[kLevel0][0] && aux[1] == pairs.h[kLevel0][1]),
                    recorded, read, skipped, bad_read, w.last_lag_frac, std::memcmp(slots_before, pairs.h, sizeof slots_before) != 0);
    }
    void run(unsigned long long key, int max_calls) {
        for (int i = 0; i < max_calls && !w.done; ++i) call(key);
    }
};

static std::vector<Meas> three(float fastest, float l0, float l1, float l2) { return {{fastest + 0.7f, l0}, {fastest, l1}, {fastest + 0.4f, l2}}; }

int main() {
    const unsigned long long A = 0x1234, B = 0x5678;
    {  // 1
        Sim s;
        s.plan[1] = three(18.0f, 0.004f, 0.005f, 0.003f);
        s.run(A, 20);
        s.finish("s1");
    }
    for (int v = 2; v <= 3; ++v) {  // 2, 3
        Sim s;
        s.plan[1] = three(18.0f, 0.20f, 0.15f, 0.30f);
        s.plan[2] = three(v == 2 ? 17.0f : 17.9f, 0.0f, 0.0f, 0.0f);
        s.run(A, 20);
        s.finish(v == 2 ? "s2" : "s3");
    }
    {  // 4: the ADVICE case - the tuner never ran, the watchdog moved from level 0 to level 1
        Sim s;
        s.w.level = 0;
        s.plan[0] = three(20.0f, 0.05f, 0.05f, 0.05f);
        s.plan[1] = three(19.0f, 0.2f, 0.2f, 0.2f);
        s.plan[2] = three(19.5f, 0.0f, 0.0f, 0.0f);
        s.run(A, 30);
        s.finish("s4");
    }
    {  // 5
        Sim s;
        s.w.level = 0;
        s.dev_lo = 0;
        s.call(A);
        const int after_first = s.w.level;
        s.run(A, 20);
        std::printf("s5first level=%d\n", after_first);
        s.finish("s5");
    }
    {  // 6: a trial of level 2 is running when the shape starts to change
        Sim s;
        s.plan[1] = three(18.0f, 0.20f, 0.15f, 0.30f);
        while (s.w.trial_from < 0) s.call(A);
        std::printf("s6trial level=%d trial_from=%d\n", s.w.level, s.w.trial_from);
        for (int i = 0; i < 4; ++i) s.call(B + i);
        s.finish("s6");
    }
    {  // 7
        Sim s;
        for (int i = 0; i < 40 && !s.w.done; ++i) s.call(i % 2 ? A : B);
        s.finish("s7");
    }
    {  // 8: eight eligible calls enqueued before the first measured one has finished
        Sim s;
        s.plan[1] = three(18.0f, 0.01f, 0.02f, 0.03f);
        s.gpu_finishes = false;
        for (int i = 0; i < 9; ++i) s.call(A);
        s.gpu_catches_up();
        s.run(A, 20);
        s.finish("s8");
    }
    const float times[3][4] = {{10, 9.8f, 9.0f, 10.2f}, {10, 9.6f, 9.65f, 9.9f}, {10, 9.95f, 9.9f, 10}};
    for (int v = 0; v < 4; ++v) {  // 9
        Sim s;
        s.w.level = 0, s.t.enabled = true;
        if (v < 3) std::memcpy(s.tuner_ms, times[v], sizeof s.tuner_ms);
        s.tuner_readable = v < 3;
        for (int i = 0; i < 7; ++i) s.call(A);
        s.finish(("s9" + std::string(1, (char)('a' + v))).c_str());
    }
    {  // 10
        Sim s;
        s.w.level = 0, s.t.enabled = true;
        for (int i = 0; i < 12 && !s.t.done; ++i) s.call(i >= 2 && i % 2 == 0 ? B : A);
        s.finish("s10");
    }
    for (int pinned = 0; pinned < 2; ++pinned) {  // 11
        Sim s;
        s.t.enabled = true;
        if (pinned) s.w.done = s.w.pinned = true;
        s.call(A);
        std::printf("s11first%d tuner_done=%d\n", pinned, (int)s.t.done);
        s.run(A, 20);
        s.finish(pinned ? "s11pinned" : "s11");
    }
    {  // the tuner's report for seven identical calls (s9 prints it too), then the watchdog at level 0
        Sim s;
        s.w.level = 0, s.t.enabled = true;
        for (int i = 0; i < 7; ++i) s.call(A);
        s.finish("seven");
    }
    {  // closed in mid-comparison
        Sim s;
        s.w.level = 0, s.t.enabled = true;
        for (int i = 0; i < 3; ++i) s.call(A);
        std::printf("midfirst measured=%d tuner_events=%d\n", s.t.measured, (s.tuner_ev[0][0] != 0) + (s.tuner_ev[0][1] != 0) + (s.tuner_ev[1][0] != 0) + (s.tuner_ev[1][1] != 0) + (s.tuner_ev[2][0] != 0));
        s.finish("mid");
    }
    {  // the tuner was never enabled: teardown leaves the pair slots alone
        Sim s;
        s.w.level = 0;
        s.plan[0] = three(20.0f, 0.05f, 0.05f, 0.05f);
        for (int i = 0; i < 7; ++i) s.call(A);
        s.finish("plain");
    }
    return 0;
}
