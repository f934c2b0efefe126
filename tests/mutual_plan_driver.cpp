// Host driver of tests/test_mutual_cpu.py: the argument checks and the grid and scratch sizing of vslam_match_mutual_dev
// (visualslam_amd/csrc/vslam_mutual_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps query and train
// capacities and pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the tiles, row
// blocks and ballot words cover the capacities and no more, the split within 1 .. min(train tiles, MT_MAX_SPLIT), and every
// scratch size equal to its product computed in 128 bits (nothing wrapped).  Then every rejection of the ABI over pointers it
// never follows, with its message byte for byte, each output one record short at the largest call, and the order of the checks.
//   driver          "plan checked=N bad=B first=...", "args checked=N bad=B first=...", and one "size ..." line per plan the
//                   test works out by hand
#include <cmath>
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_mutual_plan.h"

using namespace vslam;

namespace {
struct Call {
    alignas(16) float desc[4];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_nn2 nn[1];
    vslam_rnn rnn[1];
    vslam_match matches[1];
    vslam_desc_sets Q{desc, nullptr, points, counts, 50}, T{desc, nullptr, points, counts, 60};
    vslam_match_mutual_out out{};
    int n_pairs = 3, same_octave = 0;
    float ratio2 = 0.64f;
    const vslam_desc_sets *q = &Q, *t = &T;
    const vslam_match_mutual_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.nn = nn;
        out.nn_bytes = 3 * 50 * sizeof(vslam_nn2);
        out.rnn = rnn;
        out.rnn_bytes = 3 * 60 * sizeof(vslam_rnn);
        out.matches = matches;
        out.matches_bytes = 3 * 10 * sizeof(vslam_match);
        out.match_counts = counts;
        out.match_counts_bytes = 3 * 4;
        out.match_cap = 10;
    }
    const char* why() const { return mutual_check_args(q, t, n_pairs, ratio2, same_octave, o); }
    bool valid() const { return why() == nullptr; }
};

// a valid Call, one change to it, and the whole message it must be refused with
#define REFUSED(what, message, stmt)                              \
    {                                                             \
        Call c;                                                   \
        stmt;                                                     \
        const char* why = c.why();                                \
        args.expect(why && std::strcmp(why, message) == 0, what); \
    }
}  // namespace

int main() {
    static_assert(sizeof(vslam_rnn) == 8 && sizeof(vslam_match_mutual_out) == 10 * sizeof(size_t), "record layouts");
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff81u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 127, 128, 129, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t qc : caps)
        for (uint32_t tc : caps)
            for (int np : pairs) {
                const MutualPlan p = mutual_plan(qc, tc, np);
                const unsigned __int128 q = qc, t = tc, n = (unsigned)np;
                plan.expect((unsigned __int128)p.qtiles * MT_Q >= q && p.qtiles >= 1 && ((unsigned __int128)p.qtiles - 1) * MT_Q < q && p.qtiles < (1u << 31), "qtiles", qc, tc, np);
                plan.expect((unsigned __int128)p.ttiles * MT_T >= t && p.ttiles >= 1 && ((unsigned __int128)p.ttiles - 1) * MT_T < t, "ttiles", qc, tc, np);
                plan.expect(p.nsplit >= 1 && p.nsplit <= (unsigned int)MT_MAX_SPLIT && p.nsplit <= p.ttiles && p.nsplit <= 65535, "nsplit", qc, tc, np);
                plan.expect((unsigned __int128)p.fwords * 64 >= q && ((unsigned __int128)p.fwords - 1) * 64 < q, "fwords", qc, tc, np);
                plan.expect((unsigned __int128)p.qrow_blocks * MT_ROW_WG >= q && ((unsigned __int128)p.qrow_blocks - 1) * MT_ROW_WG < q && p.qrow_blocks < (1u << 31), "qrow_blocks", qc, tc, np);
                plan.expect((unsigned __int128)p.trow_blocks * MT_ROW_WG >= t && ((unsigned __int128)p.trow_blocks - 1) * MT_ROW_WG < t && p.trow_blocks < (1u << 31), "trow_blocks", qc, tc, np);
                plan.expect((unsigned __int128)p.q_elems == n * q && (unsigned __int128)p.t_elems == n * t, "norm elems", qc, tc, np);
                plan.expect((unsigned __int128)p.part_elems == n * p.nsplit * q && (unsigned __int128)p.part_elems * 12 < ((unsigned __int128)1 << 63), "part_elems", qc, tc, np);
                plan.expect((unsigned __int128)p.flag_words == n * p.fwords, "flag_words", qc, tc, np);
                plan.expect((unsigned __int128)p.rev_elems == n * t && (unsigned __int128)p.rev_bytes == n * t * 8 && (unsigned __int128)p.rev_bytes < ((unsigned __int128)1 << 63), "rev", qc, tc, np);
            }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);
    const struct {
        uint32_t qc, tc;
        int np;
    } shown[] = {{1, 1, 1}, {64, 64, 1}, {65, 65, 1}, {65536, 65536, 1}, {1, 65, 65535}, {65536, 64, 65535}, {1000, 777, 40}};
    for (const auto& s : shown) {
        const MutualPlan p = mutual_plan(s.qc, s.tc, s.np);
        std::printf("size %u %u %d qtiles=%u ttiles=%u nsplit=%u fwords=%u qrow_blocks=%u trow_blocks=%u part_elems=%zu flag_words=%zu rev_bytes=%zu\n", s.qc, s.tc, s.np,
                    p.qtiles, p.ttiles, p.nsplit, p.fwords, p.qrow_blocks, p.trow_blocks, p.part_elems, p.flag_words, p.rev_bytes);
    }

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.same_octave = 1;
        args.expect(c.valid(), "same_octave");
        c.same_octave = 0, c.Q.points = nullptr, c.T.points = nullptr;
        args.expect(c.valid(), "no points without same_octave");
        c.n_pairs = 65535, c.Q.cap = 0xffffffffu, c.T.cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.nn_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_nn2);
        c.out.rnn_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_rnn);
        c.out.match_cap = 0xffffffffu;
        c.out.matches_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_match);
        c.out.match_counts_bytes = 65535 * 4;
        args.expect(c.valid(), "largest");
        c.out.nn_bytes -= 1;
        args.expect(!c.valid(), "largest nn - 1");
        c.out.nn_bytes += 1, c.out.rnn_bytes -= 1;
        args.expect(!c.valid(), "largest rnn - 1");
        c.out.rnn_bytes += 1, c.out.matches_bytes -= 1;
        args.expect(!c.valid(), "largest matches - 1");
        c.out.matches_bytes += 1, c.out.match_counts_bytes -= 1;
        args.expect(!c.valid(), "largest counts - 1");
        c.out.match_counts_bytes += 1;
        args.expect(c.valid(), "largest again");
    }
    {
        // each optional output alone is a valid call
        Call c;
        c.out.rnn = nullptr, c.out.matches = nullptr, c.out.match_counts = nullptr, c.out.match_cap = 0;
        args.expect(c.valid(), "nn alone");
        Call d;
        d.out.nn = nullptr, d.out.matches = nullptr, d.out.match_counts = nullptr, d.out.match_cap = 0;
        args.expect(d.valid(), "rnn alone");
        Call e;
        e.out.nn = nullptr, e.out.rnn = nullptr, e.out.matches = nullptr, e.out.match_cap = 0;
        args.expect(e.valid(), "match_counts alone");
    }
    REFUSED("null query", "null argument", c.q = nullptr)
    REFUSED("null train", "null argument", c.t = nullptr)
    REFUSED("null out", "null argument", c.o = nullptr)
    REFUSED("struct_size", "out->struct_size is not sizeof(vslam_match_mutual_out)", c.out.struct_size -= 8)
    REFUSED("struct_size of vslam_match_out", "out->struct_size is not sizeof(vslam_match_mutual_out)", c.out.struct_size = sizeof(vslam_match_out))
    REFUSED("pairs < 0", "0 .. 65535 pairs per call", c.n_pairs = -1)
    REFUSED("pairs > 65535", "0 .. 65535 pairs per call", c.n_pairs = 65536)
    REFUSED("ratio2 0", "ratio2 must be finite and positive", c.ratio2 = 0.0f)
    REFUSED("ratio2 < 0", "ratio2 must be finite and positive", c.ratio2 = -0.64f)
    REFUSED("ratio2 nan", "ratio2 must be finite and positive", c.ratio2 = std::nanf(""))
    REFUSED("ratio2 inf", "ratio2 must be finite and positive", c.ratio2 = HUGE_VALF)
    REFUSED("query desc", "a descriptor set needs desc, counts and a capacity", c.Q.desc = nullptr)
    REFUSED("train desc", "a descriptor set needs desc, counts and a capacity", c.T.desc = nullptr)
    REFUSED("query counts", "a descriptor set needs desc, counts and a capacity", c.Q.counts = nullptr)
    REFUSED("train counts", "a descriptor set needs desc, counts and a capacity", c.T.counts = nullptr)
    REFUSED("query cap", "a descriptor set needs desc, counts and a capacity", c.Q.cap = 0)
    REFUSED("train cap", "a descriptor set needs desc, counts and a capacity", c.T.cap = 0)
    REFUSED("query misaligned", "desc must be 16-byte aligned", c.Q.desc = c.desc + 1)
    REFUSED("train misaligned", "desc must be 16-byte aligned", c.T.desc = c.desc + 2)
    REFUSED("query points", "same_octave needs the points of both sets", (c.same_octave = 1, c.Q.points = nullptr))
    REFUSED("train points", "same_octave needs the points of both sets", (c.same_octave = 1, c.T.points = nullptr))
    REFUSED("no output", "no output requested", (c.out.nn = nullptr, c.out.rnn = nullptr, c.out.matches = nullptr, c.out.match_counts = nullptr))
    REFUSED("nn small", "nn buffer too small", c.out.nn_bytes -= 1)
    REFUSED("rnn small", "rnn buffer too small", c.out.rnn_bytes -= 1)
    REFUSED("rnn sized by the query capacity", "rnn buffer too small", c.out.rnn_bytes = 3 * 50 * sizeof(vslam_rnn))
    REFUSED("matches without counts", "matches needs match_counts and a match_cap", c.out.match_counts = nullptr)
    REFUSED("match_cap 0", "matches needs match_counts and a match_cap", c.out.match_cap = 0)
    REFUSED("matches small", "matches buffer too small", c.out.matches_bytes -= 1)
    REFUSED("counts small", "match_counts buffer too small", c.out.match_counts_bytes -= 1)
    {
        // the order of the checks: with two faults the earlier kind is the one reported
        auto first = [&](const char* what, const char* expect, auto change) {
            Call c;
            change(c);
            const char* why = c.why();
            args.expect(why && std::strstr(why, expect), what);
        };
        first("null before struct_size", "null argument", [](Call& c) { c.t = nullptr, c.out.struct_size = 0; });
        first("struct_size before pairs", "struct_size", [](Call& c) { c.out.struct_size = 0, c.n_pairs = -1; });
        first("pairs before ratio2", "pairs", [](Call& c) { c.n_pairs = 65536, c.ratio2 = 0.0f; });
        first("ratio2 before sets", "ratio2", [](Call& c) { c.ratio2 = 0.0f, c.Q.desc = nullptr; });
        first("set before alignment", "needs desc", [](Call& c) { c.Q.cap = 0, c.Q.desc = c.desc + 1; });
        first("query set before train set", "16-byte", [](Call& c) { c.Q.desc = c.desc + 1, c.T.cap = 0; });
        first("points before outputs", "points", [](Call& c) { c.same_octave = 1, c.T.points = nullptr, c.out.nn_bytes = 0; });
        first("no output before sizes", "no output", [](Call& c) { c.out.nn = nullptr, c.out.rnn = nullptr, c.out.matches = nullptr, c.out.match_counts = nullptr, c.out.nn_bytes = 0; });
        first("nn before rnn", "nn buffer", [](Call& c) { c.out.nn_bytes = 0, c.out.rnn_bytes = 0; });
        first("rnn before matches", "rnn buffer", [](Call& c) { c.out.rnn_bytes = 0, c.out.match_cap = 0; });
        first("match_cap before matches size", "match_cap", [](Call& c) { c.out.match_cap = 0, c.out.matches_bytes = 0; });
        first("matches before counts", "matches buffer", [](Call& c) { c.out.matches_bytes = 0, c.out.match_counts_bytes = 0; });
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
