// Host driver of tests/test_loop_cpu.py: the argument checks and the grid and scratch sizing of the loop verification entry points
// (visualslam_amd/csrc/vslam_loop_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities, set counts
// and slot counts up to their extremes and checks every size against its product formed in 128 bits and every grid dimension
// against HIP's limits; then the empty-pair rule at its edges, and every rejection of the four checks over pointers they never
// follow, with its message byte for byte, each output one element short at the largest call, and the order of the checks.
//   driver          "plan checked=N bad=B first=...", "args checked=N bad=B first=...", and one "size ..." line per plan the
//                   test works out by hand
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "plan_driver.h"
#include "vslam_loop_plan.h"

using namespace vslam;

namespace {
struct Mem {
    alignas(16) float desc[8];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_place_cand cand[1];
    vslam_set_pair pair[1];
    vslam_match match[1];
    vslam_nn2 nn[1];
    vslam_epipolar model[1];
    vslam_loop loop[1];
    int32_t i32[1];
};

struct Pairs : Mem {  // a valid vslam_loop_pairs_dev call: 20 query frames of 3 slots, 30 database frames from 7
    const vslam_place_cand* cands = cand;
    const uint32_t* cc = counts;
    uint32_t nq = 20, c = 3, nd = 30;
    vslam_set_pair* out = pair;
    size_t bytes = 20 * 3 * 8;
    const char* why() const { return loop_pairs_check(cands, cc, nq, c, nd, out, bytes); }
};

struct Match : Mem {  // a valid vslam_match_pairs_dev call: 12 slots over 8 query sets of capacity 320 and 5 train sets of capacity 100
    vslam_desc_sets Q{desc, nullptr, points, counts, 320}, T{desc, nullptr, points, counts, 100};
    const vslam_desc_sets *q = &Q, *t = &T;
    int nqs = 8, nts = 5, n_pairs = 12, same_octave = 1;
    const vslam_set_pair* pairs = pair;
    float ratio2 = 0.64f;
    bool device = true;
    vslam_match_out out{};
    const vslam_match_out* o = &out;
    Match() {
        out.struct_size = sizeof(out);
        out.nn = nn, out.nn_bytes = 12 * 320 * 12;
        out.matches = match, out.matches_bytes = 12 * 50 * 12, out.match_cap = 50;
        out.match_counts = counts, out.match_counts_bytes = 12 * 4;
    }
    const char* why() const { return match_pairs_check(q, nqs, t, nts, pairs, n_pairs, ratio2, same_octave, o, device); }
};

struct Points : Mem {  // a valid vslam_pair_points_dev call: 12 slots of 50 records
    const vslam_match* matches = match;
    const uint32_t* mc = counts;
    uint32_t match_cap = 50, qcap = 320, tcap = 100;
    const vslam_set_pair* pairs = pair;
    int n_pairs = 12, nqs = 8, nts = 5;
    const vslam_point *qp = points, *tp = points;
    vslam_point *qo = points, *to = points;
    vslam_match* local = match;
    size_t qo_bytes = 12 * 50 * 24, to_bytes = 12 * 50 * 24, local_bytes = 12 * 50 * 12;
    const char* why() const {
        return pair_points_check(matches, mc, match_cap, pairs, n_pairs, qp, qcap, nqs, tp, tcap, nts, qo, qo_bytes, to, to_bytes, local, local_bytes);
    }
};

struct Verdict : Mem {  // a valid vslam_loop_verdict_dev call: 20 query frames of 3 slots, 30 train sets
    const vslam_epipolar* models = model;
    const vslam_set_pair* pairs = pair;
    uint32_t nq = 20, c = 3, nts = 30;
    vslam_loop_params P{12, 2, 5, 0};
    const vslam_loop_params* p = &P;
    vslam_loop_out out{};
    const vslam_loop_out* o = &out;
    Verdict() {
        out.struct_size = sizeof(out);
        out.loops = loop, out.loops_bytes = 20 * 20;
        out.loop_list = i32, out.loop_list_bytes = 20 * 4;
        out.n_loops = counts, out.n_loops_bytes = 4;
    }
    const char* why() const { return loop_verdict_check(models, pairs, nq, c, nts, p, o); }
};

// a valid call of `Type`, one change to it, and the whole message it must be refused with (nullptr: it stays valid)
#define EXPECT(Type, what, message, stmt)                                                                              \
    {                                                                                                                  \
        Type c;                                                                                                        \
        stmt;                                                                                                          \
        const char *why = c.why(), *want = message;                                                                    \
        args.expect(want ? (why && std::strcmp(why, want) == 0) : why == nullptr, #Type " " what);                      \
    }
}  // namespace

int main() {
    static_assert(sizeof(vslam_set_pair) == 8 && sizeof(vslam_loop_params) == 16 && sizeof(vslam_loop) == 20, "record layouts");
    static_assert(sizeof(vslam_loop_out) == 7 * sizeof(size_t), "out layout");
    typedef unsigned __int128 u128;
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff81u, 0xffffffffu};
    const int counts[] = {0, 1, 2, 7, 8, 9, 12, 40, 127, 128, 129, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t qc : caps)
        for (uint32_t tc : caps)
            for (int np : counts) {
                if (np == 0) continue;  // (a call without slots launches nothing and sizes nothing)
                for (int ns : {0, 1, 17, 65535}) {
                    const MatchPairsPlan p = match_pairs_plan(qc, ns, tc, 65535 - ns, np);
                    const u128 q = qc, t = tc, s = (unsigned)np;
                    plan.expect((u128)p.m.qtiles * MT_Q >= q && ((u128)p.m.qtiles - 1) * MT_Q < q && p.m.qtiles < (1u << 31), "qtiles", qc, tc, np);
                    plan.expect((u128)p.m.ttiles * MT_T >= t && ((u128)p.m.ttiles - 1) * MT_T < t, "ttiles", qc, tc, np);
                    plan.expect(p.m.nsplit >= 1 && p.m.nsplit <= (unsigned int)MT_MAX_SPLIT && p.m.nsplit <= p.m.ttiles, "nsplit", qc, tc, np);
                    plan.expect((u128)p.m.qrow_blocks * MT_ROW_WG >= q && ((u128)p.m.qrow_blocks - 1) * MT_ROW_WG < q && p.m.qrow_blocks < (1u << 31), "qrow_blocks", qc, tc, np);
                    plan.expect((u128)p.m.part_elems == s * p.m.nsplit * q && (u128)p.m.part_elems * 12 < ((u128)1 << 63), "part", qc, tc, np);
                    plan.expect((u128)p.m.q_elems == s * q && (u128)p.m.flag_words == s * p.m.fwords && (u128)p.m.fwords * 64 >= q, "per pair", qc, tc, np);
                    plan.expect((u128)p.qnorm_elems == (u128)(unsigned)ns * q && (u128)p.tnorm_elems == (u128)(unsigned)(65535 - ns) * t, "norms by the sets", qc, tc, ns);
                }
                const PairPointsPlan g = pair_points_plan(qc, np);
                plan.expect((u128)g.row_blocks * LP_WG >= qc && ((u128)g.row_blocks - 1) * LP_WG < qc && g.row_blocks < (1u << 31), "row_blocks", qc, np);
                plan.expect((u128)g.records == (u128)qc * (unsigned)np && (u128)g.records * 24 < ((u128)1 << 63), "records", qc, np);
            }
    for (int nq : counts)
        for (uint32_t c = 1; c <= LP_MAX_C; ++c) {
            const LoopPairsPlan p = loop_pairs_plan((uint32_t)nq, c);
            plan.expect((u128)p.slots == (u128)(unsigned)nq * c, "slots", nq, c);
            plan.expect((u128)p.blocks * LP_WG >= p.slots && (p.slots == 0 ? p.blocks == 0 : ((u128)p.blocks - 1) * LP_WG < p.slots), "blocks", nq, c);
        }
    // the empty-pair rule at its edges
    const int32_t lo = std::numeric_limits<int32_t>::min(), hi = std::numeric_limits<int32_t>::max();
    plan.expect(pair_empty(vslam_set_pair{-1, -1}, 65535, 65535) && pair_empty(vslam_set_pair{-1, 0}, 8, 8) && pair_empty(vslam_set_pair{0, -1}, 8, 8), "minus one");
    plan.expect(!pair_empty(vslam_set_pair{0, 0}, 1, 1) && !pair_empty(vslam_set_pair{7, 4}, 8, 5), "last set");
    plan.expect(pair_empty(vslam_set_pair{8, 4}, 8, 5) && pair_empty(vslam_set_pair{7, 5}, 8, 5), "set index equal to the count");
    plan.expect(pair_empty(vslam_set_pair{0, 0}, 0, 5) && pair_empty(vslam_set_pair{0, 0}, 5, 0), "no sets");
    plan.expect(pair_empty(vslam_set_pair{lo, 0}, 65535, 65535) && pair_empty(vslam_set_pair{0, hi}, 65535, 65535), "extremes");
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);
    const struct {
        uint32_t qc, tc;
        int nqs, nts, np;
    } shown[] = {{320, 320, 8, 8, 12}, {320, 320, 8, 8, 1}, {320, 320, 8, 8, 40}, {2000, 2000, 256, 256, 2048}, {0xffffffffu, 0xffffffffu, 65535, 65535, 65535}};
    for (const auto& s : shown) {
        const MatchPairsPlan p = match_pairs_plan(s.qc, s.nqs, s.tc, s.nts, s.np);
        std::printf("size %u %d %d qtiles=%u ttiles=%u nsplit=%u qrow_blocks=%u part_elems=%zu qnorm_elems=%zu flag_words=%zu\n", s.qc, s.nqs, s.np, p.m.qtiles,
                    p.m.ttiles, p.m.nsplit, p.m.qrow_blocks, p.m.part_elems, p.qnorm_elems, p.m.flag_words);
    }

    Tally args;
    const float nan = std::nanf(""), inf = std::numeric_limits<float>::infinity();
    // ---- vslam_loop_pairs_dev
    EXPECT(Pairs, "valid", nullptr, (void)0)
    EXPECT(Pairs, "no query frames", nullptr, (c.nq = 0, c.bytes = 0))
    EXPECT(Pairs, "an empty database", nullptr, c.nd = 0)
    EXPECT(Pairs, "largest", nullptr, (c.nq = c.nd = 65535, c.c = 8, c.bytes = (size_t)65535 * 8 * 8))
    EXPECT(Pairs, "largest - 1", "pairs buffer too small", (c.nq = c.nd = 65535, c.c = 8, c.bytes = (size_t)65535 * 8 * 8 - 1))
    EXPECT(Pairs, "null candidates", "null argument", c.cands = nullptr)
    EXPECT(Pairs, "null cand_counts", "null argument", c.cc = nullptr)
    EXPECT(Pairs, "null pairs", "null argument", c.out = nullptr)
    EXPECT(Pairs, "nq", "at most 65535 frames on either side", c.nq = 65536)
    EXPECT(Pairs, "nd", "at most 65535 frames on either side", c.nd = 65536)
    EXPECT(Pairs, "c 0", "c must be 1 .. 8", c.c = 0)
    EXPECT(Pairs, "c 9", "c must be 1 .. 8", c.c = 9)
    EXPECT(Pairs, "pairs small", "pairs buffer too small", c.bytes -= 1)
    EXPECT(Pairs, "pairs sized for c = 3 with c = 4", "pairs buffer too small", c.c = 4)
    EXPECT(Pairs, "null before frames", "null argument", (c.out = nullptr, c.nq = 65536))
    EXPECT(Pairs, "frames before c", "at most 65535 frames on either side", (c.nd = 65536, c.c = 0))
    EXPECT(Pairs, "c before size", "c must be 1 .. 8", (c.c = 9, c.bytes = 0))
    // ---- vslam_match_pairs_dev / vslam_match_pairs_host
    EXPECT(Match, "valid", nullptr, (void)0)
    EXPECT(Match, "no pairs", nullptr, c.n_pairs = 0)
    EXPECT(Match, "no sets on either side", nullptr, (c.nqs = 0, c.nts = 0))
    EXPECT(Match, "one buffer on both sides", nullptr, (c.t = c.q, c.nts = c.nqs))
    EXPECT(Match, "nn alone", nullptr, (c.out.matches = nullptr, c.out.match_counts = nullptr))
    EXPECT(Match, "match_counts alone", nullptr, (c.out.nn = nullptr, c.out.matches = nullptr))
    EXPECT(Match, "without points", nullptr, (c.same_octave = 0, c.Q.points = nullptr, c.T.points = nullptr))
    EXPECT(Match, "largest", nullptr,
           (c.n_pairs = c.nqs = c.nts = 65535, c.Q.cap = c.T.cap = 0xffffffffu, c.out.nn_bytes = (size_t)65535 * 0xffffffffu * 12, c.out.match_cap = 0xffffffffu,
            c.out.matches_bytes = (size_t)65535 * 0xffffffffu * 12, c.out.match_counts_bytes = 65535 * 4))
    EXPECT(Match, "largest nn - 1", "nn buffer too small",
           (c.n_pairs = 65535, c.Q.cap = 0xffffffffu, c.out.nn_bytes = (size_t)65535 * 0xffffffffu * 12 - 1, c.out.matches_bytes = 65535 * 50 * 12, c.out.match_counts_bytes = 65535 * 4))
    EXPECT(Match, "largest matches - 1", "matches buffer too small",
           (c.n_pairs = 65535, c.out.nn_bytes = (size_t)65535 * 320 * 12, c.out.match_cap = 0xffffffffu, c.out.matches_bytes = (size_t)65535 * 0xffffffffu * 12 - 1,
            c.out.match_counts_bytes = 65535 * 4))
    EXPECT(Match, "null query", "null argument", c.q = nullptr)
    EXPECT(Match, "null train", "null argument", c.t = nullptr)
    EXPECT(Match, "null pairs", "null argument", c.pairs = nullptr)
    EXPECT(Match, "null out", "null argument", c.o = nullptr)
    EXPECT(Match, "struct_size", "out->struct_size is not sizeof(vslam_match_out)", c.out.struct_size -= 8)
    EXPECT(Match, "pairs < 0", "0 .. 65535 pairs per call", c.n_pairs = -1)
    EXPECT(Match, "pairs 65536", "0 .. 65535 pairs per call", c.n_pairs = 65536)
    EXPECT(Match, "query sets < 0", "0 .. 65535 sets on either side", c.nqs = -1)
    EXPECT(Match, "query sets 65536", "0 .. 65535 sets on either side", c.nqs = 65536)
    EXPECT(Match, "train sets < 0", "0 .. 65535 sets on either side", c.nts = -1)
    EXPECT(Match, "train sets 65536", "0 .. 65535 sets on either side", c.nts = 65536)
    EXPECT(Match, "ratio2 0", "ratio2 must be finite and positive", c.ratio2 = 0.0f)
    EXPECT(Match, "ratio2 < 0", "ratio2 must be finite and positive", c.ratio2 = -0.64f)
    EXPECT(Match, "ratio2 NaN", "ratio2 must be finite and positive", c.ratio2 = nan)
    EXPECT(Match, "ratio2 inf", "ratio2 must be finite and positive", c.ratio2 = inf)
    EXPECT(Match, "query desc", "a descriptor set needs desc, counts and a capacity", c.Q.desc = nullptr)
    EXPECT(Match, "train counts", "a descriptor set needs desc, counts and a capacity", c.T.counts = nullptr)
    EXPECT(Match, "train cap", "a descriptor set needs desc, counts and a capacity", c.T.cap = 0)
    EXPECT(Match, "query desc misaligned", "desc must be 16-byte aligned", c.Q.desc = c.desc + 1)
    EXPECT(Match, "train desc misaligned", "desc must be 16-byte aligned", c.T.desc = c.desc + 2)
    EXPECT(Match, "host arrays need no alignment", nullptr, (c.device = false, c.Q.desc = c.desc + 1, c.T.desc = c.desc + 2))
    EXPECT(Match, "same_octave without query points", "same_octave needs the points of both sets", c.Q.points = nullptr)
    EXPECT(Match, "same_octave without train points", "same_octave needs the points of both sets", c.T.points = nullptr)
    EXPECT(Match, "no output", "no output requested", (c.out.nn = nullptr, c.out.matches = nullptr, c.out.match_counts = nullptr))
    EXPECT(Match, "nn small", "nn buffer too small", c.out.nn_bytes -= 1)
    EXPECT(Match, "nn sized by the sets", "nn buffer too small", c.out.nn_bytes = 8 * 320 * 12)
    EXPECT(Match, "matches without counts", "matches needs match_counts and a match_cap", c.out.match_counts = nullptr)
    EXPECT(Match, "matches without a cap", "matches needs match_counts and a match_cap", c.out.match_cap = 0)
    EXPECT(Match, "matches small", "matches buffer too small", c.out.matches_bytes -= 1)
    EXPECT(Match, "match_counts small", "match_counts buffer too small", c.out.match_counts_bytes -= 1)
    EXPECT(Match, "null before struct_size", "null argument", (c.pairs = nullptr, c.out.struct_size = 0))
    EXPECT(Match, "struct_size before pairs", "out->struct_size is not sizeof(vslam_match_out)", (c.out.struct_size = 0, c.n_pairs = -1))
    EXPECT(Match, "pairs before sets", "0 .. 65535 pairs per call", (c.n_pairs = -1, c.nqs = -1))
    EXPECT(Match, "sets before ratio2", "0 .. 65535 sets on either side", (c.nts = 65536, c.ratio2 = nan))
    EXPECT(Match, "ratio2 before the sets' pointers", "ratio2 must be finite and positive", (c.ratio2 = nan, c.Q.desc = nullptr))
    EXPECT(Match, "query set before train set", "desc must be 16-byte aligned", (c.Q.desc = c.desc + 1, c.T.desc = nullptr))
    EXPECT(Match, "alignment before points", "desc must be 16-byte aligned", (c.Q.desc = c.desc + 1, c.Q.points = nullptr))
    EXPECT(Match, "points before outputs", "same_octave needs the points of both sets", (c.T.points = nullptr, c.out.nn = nullptr, c.out.matches = nullptr, c.out.match_counts = nullptr))
    EXPECT(Match, "nn before matches", "nn buffer too small", (c.out.nn_bytes = 0, c.out.matches_bytes = 0))
    EXPECT(Match, "matches before match_counts", "matches buffer too small", (c.out.matches_bytes = 0, c.out.match_counts_bytes = 0))
    // ---- vslam_pair_points_dev
    EXPECT(Points, "valid", nullptr, (void)0)
    EXPECT(Points, "no pairs", nullptr, (c.n_pairs = 0, c.qo_bytes = c.to_bytes = c.local_bytes = 0))
    EXPECT(Points, "largest", nullptr,
           (c.n_pairs = c.nqs = c.nts = 65535, c.match_cap = c.qcap = c.tcap = 0xffffffffu, c.qo_bytes = c.to_bytes = (size_t)65535 * 0xffffffffu * 24,
            c.local_bytes = (size_t)65535 * 0xffffffffu * 12))
    EXPECT(Points, "largest local - 1", "local buffer too small",
           (c.n_pairs = 65535, c.match_cap = 0xffffffffu, c.qo_bytes = c.to_bytes = (size_t)65535 * 0xffffffffu * 24, c.local_bytes = (size_t)65535 * 0xffffffffu * 12 - 1))
    EXPECT(Points, "null matches", "null argument", c.matches = nullptr)
    EXPECT(Points, "null match_counts", "null argument", c.mc = nullptr)
    EXPECT(Points, "null pairs", "null argument", c.pairs = nullptr)
    EXPECT(Points, "null query_points", "null argument", c.qp = nullptr)
    EXPECT(Points, "null train_points", "null argument", c.tp = nullptr)
    EXPECT(Points, "null query_points_out", "null argument", c.qo = nullptr)
    EXPECT(Points, "null train_points_out", "null argument", c.to = nullptr)
    EXPECT(Points, "null local", "null argument", c.local = nullptr)
    EXPECT(Points, "pairs < 0", "0 .. 65535 pairs per call", c.n_pairs = -1)
    EXPECT(Points, "pairs 65536", "0 .. 65535 pairs per call", c.n_pairs = 65536)
    EXPECT(Points, "query sets", "0 .. 65535 sets on either side", c.nqs = 65536)
    EXPECT(Points, "train sets", "0 .. 65535 sets on either side", c.nts = -1)
    EXPECT(Points, "match_cap 0", "match_cap, query_cap and train_cap must be positive", c.match_cap = 0)
    EXPECT(Points, "query_cap 0", "match_cap, query_cap and train_cap must be positive", c.qcap = 0)
    EXPECT(Points, "train_cap 0", "match_cap, query_cap and train_cap must be positive", c.tcap = 0)
    EXPECT(Points, "query_points_out small", "query_points_out buffer too small", c.qo_bytes -= 1)
    EXPECT(Points, "train_points_out small", "train_points_out buffer too small", c.to_bytes -= 1)
    EXPECT(Points, "local small", "local buffer too small", c.local_bytes -= 1)
    EXPECT(Points, "null before pairs", "null argument", (c.local = nullptr, c.n_pairs = -1))
    EXPECT(Points, "pairs before sets", "0 .. 65535 pairs per call", (c.n_pairs = -1, c.nqs = -1))
    EXPECT(Points, "sets before capacities", "0 .. 65535 sets on either side", (c.nqs = -1, c.match_cap = 0))
    EXPECT(Points, "capacities before sizes", "match_cap, query_cap and train_cap must be positive", (c.tcap = 0, c.qo_bytes = 0))
    EXPECT(Points, "query before train", "query_points_out buffer too small", (c.qo_bytes = 0, c.to_bytes = 0))
    EXPECT(Points, "train before local", "train_points_out buffer too small", (c.to_bytes = 0, c.local_bytes = 0))
    // ---- vslam_loop_verdict_dev / vslam_loop_verdict_host
    EXPECT(Verdict, "valid", nullptr, (void)0)
    EXPECT(Verdict, "no query frames", nullptr, c.nq = 0)
    EXPECT(Verdict, "loops alone", nullptr, (c.out.loop_list = nullptr, c.out.n_loops = nullptr))
    EXPECT(Verdict, "n_loops alone", nullptr, (c.out.loops = nullptr, c.out.loop_list = nullptr))
    EXPECT(Verdict, "the list with its count", nullptr, c.out.loops = nullptr)
    EXPECT(Verdict, "extreme params", nullptr, (c.P.min_inliers = 0xffffffffu, c.P.num = 0xffffffffu, c.P.den = 0xffffffffu))
    EXPECT(Verdict, "largest", nullptr, (c.nq = c.nts = 65535, c.c = 8, c.out.loops_bytes = 65535 * 20, c.out.loop_list_bytes = 65535 * 4))
    EXPECT(Verdict, "largest loops - 1", "loops buffer too small", (c.nq = 65535, c.out.loops_bytes = 65535 * 20 - 1, c.out.loop_list_bytes = 65535 * 4))
    EXPECT(Verdict, "null models", "null argument", c.models = nullptr)
    EXPECT(Verdict, "null pairs", "null argument", c.pairs = nullptr)
    EXPECT(Verdict, "null params", "null argument", c.p = nullptr)
    EXPECT(Verdict, "null out", "null argument", c.o = nullptr)
    EXPECT(Verdict, "struct_size", "out->struct_size is not sizeof(vslam_loop_out)", c.out.struct_size += 8)
    EXPECT(Verdict, "nq", "at most 65535 frames on either side", c.nq = 65536)
    EXPECT(Verdict, "train sets", "at most 65535 frames on either side", c.nts = 65536)
    EXPECT(Verdict, "c 0", "c must be 1 .. 8", c.c = 0)
    EXPECT(Verdict, "c 9", "c must be 1 .. 8", c.c = 9)
    EXPECT(Verdict, "min_inliers", "min_inliers must be positive", c.P.min_inliers = 0)
    EXPECT(Verdict, "den", "den must be positive", c.P.den = 0)
    EXPECT(Verdict, "reserved", "params->reserved must be 0", c.P.reserved = 1)
    EXPECT(Verdict, "no output", "no output requested", (c.out.loops = nullptr, c.out.loop_list = nullptr, c.out.n_loops = nullptr))
    EXPECT(Verdict, "loop_list without n_loops", "loop_list needs n_loops", c.out.n_loops = nullptr)
    EXPECT(Verdict, "loops small", "loops buffer too small", c.out.loops_bytes -= 1)
    EXPECT(Verdict, "loop_list small", "loop_list buffer too small", c.out.loop_list_bytes -= 1)
    EXPECT(Verdict, "n_loops small", "n_loops buffer too small", c.out.n_loops_bytes -= 1)
    EXPECT(Verdict, "null before struct_size", "null argument", (c.models = nullptr, c.out.struct_size = 0))
    EXPECT(Verdict, "struct_size before frames", "out->struct_size is not sizeof(vslam_loop_out)", (c.out.struct_size = 0, c.nq = 65536))
    EXPECT(Verdict, "frames before c", "at most 65535 frames on either side", (c.nq = 65536, c.c = 0))
    EXPECT(Verdict, "c before min_inliers", "c must be 1 .. 8", (c.c = 0, c.P.min_inliers = 0))
    EXPECT(Verdict, "min_inliers before den", "min_inliers must be positive", (c.P.min_inliers = 0, c.P.den = 0))
    EXPECT(Verdict, "den before reserved", "den must be positive", (c.P.den = 0, c.P.reserved = 1))
    EXPECT(Verdict, "reserved before outputs", "params->reserved must be 0", (c.P.reserved = 1, c.out.n_loops = nullptr))
    EXPECT(Verdict, "list rule before sizes", "loop_list needs n_loops", (c.out.n_loops = nullptr, c.out.loops_bytes = 0))
    EXPECT(Verdict, "loops before loop_list", "loops buffer too small", (c.out.loops_bytes = 0, c.out.loop_list_bytes = 0))
    EXPECT(Verdict, "loop_list before n_loops", "loop_list buffer too small", (c.out.loop_list_bytes = 0, c.out.n_loops_bytes = 0))
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
