// Host driver of tests/test_guided_cpu.py: the argument checks and the grid and scratch sizing of vslam_match_guided_dev
// (visualslam_amd/csrc/vslam_guided_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps query and train
// capacities and pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the tiles, row
// blocks and ballot words cover the capacities and no more, the split within 1 .. min(train tiles, MT_MAX_SPLIT), and every
// scratch size equal to its product computed in 128 bits (nothing wrapped).  Then every rejection of the ABI over pointers it
// never follows, each output one record short at the largest call, and the order of the checks by their messages.
//   driver          one line each: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_guided_plan.h"

using namespace vslam;

namespace {
struct Call {
    alignas(16) float desc[4];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_epipolar models[1];
    vslam_nn2 nn[1];
    vslam_match matches[1];
    vslam_desc_sets Q{desc, nullptr, points, counts, 50}, T{desc, nullptr, points, counts, 60};
    vslam_guided_params prm{0.64f, 1.0f, 4.0, 0, 0};
    vslam_match_out out{};
    int n_pairs = 3;
    const vslam_desc_sets *q = &Q, *t = &T;
    const vslam_epipolar* m = models;
    const vslam_guided_params* p = &prm;
    const vslam_match_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.nn = nn;
        out.nn_bytes = 3 * 50 * sizeof(vslam_nn2);
        out.matches = matches;
        out.matches_bytes = 3 * 10 * sizeof(vslam_match);
        out.match_counts = counts;
        out.match_counts_bytes = 3 * 4;
        out.match_cap = 10;
    }
    const char* why() const { return guided_check_args(q, t, m, n_pairs, p, o); }
    bool valid() const { return why() == nullptr; }
};
}  // namespace

int main() {
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff81u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 127, 128, 129, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t qc : caps)
        for (uint32_t tc : caps)
            for (int np : pairs) {
                const GuidedPlan p = guided_plan(qc, tc, np);
                const unsigned __int128 q = qc, t = tc, n = (unsigned)np;
                plan.expect((unsigned __int128)p.qtiles * MT_Q >= q && p.qtiles >= 1 && ((unsigned __int128)p.qtiles - 1) * MT_Q < q && p.qtiles < (1u << 31), "qtiles", qc, tc, np);
                plan.expect((unsigned __int128)p.ttiles * MT_T >= t && p.ttiles >= 1 && ((unsigned __int128)p.ttiles - 1) * MT_T < t, "ttiles", qc, tc, np);
                plan.expect(p.nsplit >= 1 && p.nsplit <= (unsigned int)MT_MAX_SPLIT && p.nsplit <= p.ttiles && p.nsplit <= 65535, "nsplit", qc, tc, np);
                plan.expect((unsigned __int128)p.fwords * 64 >= q && ((unsigned __int128)p.fwords - 1) * 64 < q, "fwords", qc, tc, np);
                plan.expect((unsigned __int128)p.qrow_blocks * MT_ROW_WG >= q && ((unsigned __int128)p.qrow_blocks - 1) * MT_ROW_WG < q && p.qrow_blocks < (1u << 31), "qrow_blocks", qc, tc, np);
                plan.expect((unsigned __int128)p.trow_blocks * MT_ROW_WG >= t && ((unsigned __int128)p.trow_blocks - 1) * MT_ROW_WG < t && p.trow_blocks < (1u << 31), "trow_blocks", qc, tc, np);
                plan.expect((unsigned __int128)p.q_elems == n * q && (unsigned __int128)p.q_elems * sizeof(GuidedRow) < ((unsigned __int128)1 << 63), "q_elems", qc, tc, np);
                plan.expect((unsigned __int128)p.t_elems == n * t && (unsigned __int128)p.t_elems * sizeof(GuidedRow) < ((unsigned __int128)1 << 63), "t_elems", qc, tc, np);
                plan.expect((unsigned __int128)p.part_elems == n * p.nsplit * q && (unsigned __int128)p.part_elems * 12 < ((unsigned __int128)1 << 63), "part_elems", qc, tc, np);
                plan.expect((unsigned __int128)p.flag_words == n * p.fwords, "flag_words", qc, tc, np);
            }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.prm.max_desc_dist2 = HUGE_VALF;
        args.expect(c.valid(), "no bound");
        c.prm.same_octave = 1;
        args.expect(c.valid(), "same_octave");
        c.n_pairs = 65535, c.Q.cap = 0xffffffffu, c.T.cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.nn_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_nn2);
        c.out.match_cap = 0xffffffffu;
        c.out.matches_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_match);
        c.out.match_counts_bytes = 65535 * 4;
        args.expect(c.valid(), "largest");
        c.out.nn_bytes -= 1;
        args.expect(!c.valid(), "largest nn - 1");
        c.out.nn_bytes += 1, c.out.matches_bytes -= 1;
        args.expect(!c.valid(), "largest matches - 1");
        c.out.matches_bytes += 1, c.out.match_counts_bytes -= 1;
        args.expect(!c.valid(), "largest counts - 1");
        c.out.match_counts_bytes += 1;
        args.expect(c.valid(), "largest again");
    }
    REJECT("null query", c.q = nullptr)
    REJECT("null train", c.t = nullptr)
    REJECT("null models", c.m = nullptr)
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("struct_size", c.out.struct_size -= 8)
    REJECT("pairs < 0", c.n_pairs = -1)
    REJECT("pairs > 65535", c.n_pairs = 65536)
    REJECT("reserved", c.prm.reserved = 1)
    REJECT("ratio2 0", c.prm.ratio2 = 0.0f)
    REJECT("ratio2 < 0", c.prm.ratio2 = -0.64f)
    REJECT("ratio2 nan", c.prm.ratio2 = std::nanf(""))
    REJECT("ratio2 inf", c.prm.ratio2 = HUGE_VALF)
    REJECT("bound 0", c.prm.max_desc_dist2 = 0.0f)
    REJECT("bound < 0", c.prm.max_desc_dist2 = -1.0f)
    REJECT("bound -inf", c.prm.max_desc_dist2 = -HUGE_VALF)
    REJECT("bound nan", c.prm.max_desc_dist2 = std::nanf(""))
    REJECT("dist 0", c.prm.max_dist2 = 0.0)
    REJECT("dist < 0", c.prm.max_dist2 = -4.0)
    REJECT("dist nan", c.prm.max_dist2 = std::nan(""))
    REJECT("dist inf", c.prm.max_dist2 = HUGE_VAL)
    REJECT("query desc", c.Q.desc = nullptr)
    REJECT("train desc", c.T.desc = nullptr)
    REJECT("query counts", c.Q.counts = nullptr)
    REJECT("train counts", c.T.counts = nullptr)
    REJECT("query cap", c.Q.cap = 0)
    REJECT("train cap", c.T.cap = 0)
    REJECT("query misaligned", c.Q.desc = c.desc + 1)
    REJECT("train misaligned", c.T.desc = c.desc + 2)
    REJECT("query points", c.Q.points = nullptr)
    REJECT("train points", c.T.points = nullptr)
    REJECT("no output", (c.out.nn = nullptr, c.out.matches = nullptr, c.out.match_counts = nullptr))
    REJECT("nn small", c.out.nn_bytes -= 1)
    REJECT("matches without counts", c.out.match_counts = nullptr)
    REJECT("match_cap 0", c.out.match_cap = 0)
    REJECT("matches small", c.out.matches_bytes -= 1)
    REJECT("counts small", c.out.match_counts_bytes -= 1)
    {
        // the order of the checks: with two faults the earlier kind is the one reported
        auto first = [&](const char* what, const char* expect, auto change) {
            Call c;
            change(c);
            const char* why = c.why();
            args.expect(why && std::strstr(why, expect), what);
        };
        first("null before struct_size", "null argument", [](Call& c) { c.m = nullptr, c.out.struct_size = 0; });
        first("struct_size before pairs", "struct_size", [](Call& c) { c.out.struct_size = 0, c.n_pairs = -1; });
        first("pairs before params", "pairs", [](Call& c) { c.n_pairs = 65536, c.prm.reserved = 7; });
        first("reserved before ratio2", "reserved", [](Call& c) { c.prm.reserved = 7, c.prm.ratio2 = 0.0f; });
        first("ratio2 before bound", "ratio2", [](Call& c) { c.prm.ratio2 = 0.0f, c.prm.max_desc_dist2 = 0.0f; });
        first("bound before dist", "max_desc_dist2", [](Call& c) { c.prm.max_desc_dist2 = 0.0f, c.prm.max_dist2 = 0.0; });
        first("dist before sets", "max_dist2", [](Call& c) { c.prm.max_dist2 = 0.0, c.Q.desc = nullptr; });
        first("set before alignment", "needs desc", [](Call& c) { c.Q.cap = 0, c.Q.desc = c.desc + 1; });
        first("query set before train set", "16-byte", [](Call& c) { c.Q.desc = c.desc + 1, c.T.points = nullptr; });
        first("points before outputs", "points", [](Call& c) { c.T.points = nullptr, c.out.nn_bytes = 0; });
        first("no output before sizes", "no output", [](Call& c) { c.out.nn = nullptr, c.out.matches = nullptr, c.out.match_counts = nullptr, c.out.nn_bytes = 0; });
        first("nn before matches", "nn buffer", [](Call& c) { c.out.nn_bytes = 0, c.out.match_cap = 0; });
        first("match_cap before matches size", "match_cap", [](Call& c) { c.out.match_cap = 0, c.out.matches_bytes = 0; });
        first("matches before counts", "matches buffer", [](Call& c) { c.out.matches_bytes = 0, c.out.match_counts_bytes = 0; });
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
