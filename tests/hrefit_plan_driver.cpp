// Host driver of tests/test_hrefit_cpu.py: the argument checks and the grid and scratch sizing of vslam_hrefit_dev
// (visualslam_amd/csrc/vslam_hrefit_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities and
// pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the sum blocks, record
// blocks and pair blocks cover the capacities, and every scratch size equal to its product computed in 128 bits (nothing
// wrapped).  Then every rejection of the ABI with its message, over pointers it never follows, a buffer one record short
// for each output, and the order of the checks: of two things wrong, which one is reported.
//   driver          "plan checked=N bad=B first=...", "args checked=N bad=B first=..." and one "msg name|message" per rejection
#include <cmath>
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_hrefit_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_homography models[1];
    vslam_epipolar epis[1];
    vslam_hrefit_params prm{4, 4.0, 1, 2, 16};
    vslam_hrefit_out out{};
    uint32_t match_cap = 100, query_cap = 50, train_cap = 60;
    int n_pairs = 3;
    const vslam_homography* md = models;
    const vslam_epipolar* epi = epis;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const vslam_point *qp = points, *tp = points;
    const vslam_hrefit_params* p = &prm;
    const vslam_hrefit_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.models = models;  // in place
        out.models_bytes = 3 * sizeof(vslam_homography);
        out.info = reinterpret_cast<vslam_hrefit*>(matches);
        out.info_bytes = 3 * sizeof(vslam_hrefit);
        out.inlier_bits = reinterpret_cast<uint64_t*>(matches);
        out.inlier_bits_bytes = 3 * 2 * 8;
        out.inliers = matches;
        out.inliers_bytes = 3 * 40 * sizeof(vslam_match);
        out.inlier_counts = counts;
        out.inlier_counts_bytes = 3 * sizeof(uint32_t);
        out.inlier_cap = 40;
        out.gated_models = epis;  // in place
        out.gated_models_bytes = 3 * sizeof(vslam_epipolar);
    }
    const char* why() const { return hrefit_check_args(md, m, mc, match_cap, qp, query_cap, tp, train_cap, n_pairs, epi, p, o); }
    bool valid() const { return why() == nullptr; }
    bool says(const char* word) const { return why() && std::strstr(why(), word); }
};
}  // namespace

// REJECT, and the message goes to the output for the test to compare
#define REJECT_MSG(what, stmt)                                        \
    {                                                                 \
        Call c;                                                       \
        stmt;                                                         \
        args.expect(!c.valid(), what);                                \
        std::printf("msg %s|%s\n", what, c.why() ? c.why() : "-");    \
    }

int main() {
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xfffff000u, 0xfffff001u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t cap : caps)
        for (int np : pairs) {
            const HRefitPlan p = hrefit_plan(cap, np);
            const unsigned __int128 c = cap, n = (unsigned)np, lim = (unsigned __int128)1 << 63;
            plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np);
            plan.expect((unsigned __int128)p.rec_blocks * TWOVIEW_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                            ((unsigned __int128)p.rec_blocks - 1) * TWOVIEW_REC_WG < c, "rec_blocks", cap, np);
            plan.expect((unsigned __int128)p.sum_blocks * REFIT_BLOCK >= c && p.sum_blocks >= 1 && p.sum_blocks <= (1u << 20) &&
                            ((unsigned __int128)p.sum_blocks - 1) * REFIT_BLOCK < c, "sum_blocks", cap, np);
            plan.expect((unsigned __int128)p.pair_blocks * REFIT_PAIR_WG >= n && p.pair_blocks >= 1 && (p.pair_blocks - 1) * REFIT_PAIR_WG < (unsigned)np,
                        "pair_blocks", cap, np);
            plan.expect(np <= 65535, "grid.y", cap, np);
            plan.expect((unsigned __int128)p.coords_elems == n * c && (unsigned __int128)p.coords_elems * 32 < lim, "coords", cap, np);
            plan.expect((unsigned __int128)p.partial_elems == n * p.sum_blocks * HREFIT_SUMS && (unsigned __int128)p.partial_elems * 8 < lim, "partial", cap, np);
            plan.expect((unsigned __int128)p.state_elems == n && (unsigned __int128)p.state_elems * sizeof(HRefitState) < lim, "state", cap, np);
            plan.expect((unsigned __int128)p.flag_words == n * p.fwords && (unsigned __int128)p.flag_words * 8 < lim, "flags", cap, np);
        }
    plan.expect(sizeof(HRefitState) == 520 && HREFIT_SUMS == 24, "state record");
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.n_pairs = 3;
        c.out.info = nullptr, c.out.inlier_bits = nullptr, c.out.inliers = nullptr, c.out.inlier_counts = nullptr, c.out.gated_models = nullptr;
        c.out.info_bytes = c.out.inlier_bits_bytes = c.out.inliers_bytes = c.out.inlier_counts_bytes = c.out.gated_models_bytes = 0, c.out.inlier_cap = 0;
        args.expect(c.valid(), "models alone");
        c.epi = nullptr, c.prm.degenerate_den = 0;
        args.expect(c.valid(), "no verdict: degenerate_den is not read");
        c.epi = c.epis, c.prm.degenerate_den = 2;
        c.out.inlier_counts = c.counts, c.out.inlier_counts_bytes = 3 * sizeof(uint32_t);
        args.expect(c.valid(), "totals alone");
        c.prm.rounds = 1;
        args.expect(c.valid(), "1 round");
        c.prm.rounds = 8;
        args.expect(c.valid(), "8 rounds");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu, c.out.inlier_cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.models_bytes = 65535 * sizeof(vslam_homography);
        c.out.info_bytes = 65535 * sizeof(vslam_hrefit);
        c.out.inlier_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        c.out.inliers_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_match);
        c.out.inlier_counts_bytes = 65535 * sizeof(uint32_t);
        c.out.gated_models_bytes = 65535 * sizeof(vslam_epipolar);
        args.expect(c.valid(), "largest");
        c.out.inliers_bytes -= 1;
        args.expect(!c.valid(), "largest inliers - 1");
        c.out.inliers_bytes += 1, c.out.inlier_bits_bytes -= 1;
        args.expect(!c.valid(), "largest bits - 1");
        c.out.inlier_bits_bytes += 1, c.out.info_bytes -= 1;
        args.expect(!c.valid(), "largest info - 1");
        c.out.info_bytes += 1, c.out.models_bytes -= 1;
        args.expect(!c.valid(), "largest models - 1");
        c.out.models_bytes += 1, c.out.inlier_counts_bytes -= 1;
        args.expect(!c.valid(), "largest counts - 1");
        c.out.inlier_counts_bytes += 1, c.out.gated_models_bytes -= 1;
        args.expect(!c.valid(), "largest gated - 1");
        c.out.gated_models_bytes += 1;
        args.expect(c.valid(), "largest again");
    }
    REJECT_MSG("null params", c.p = nullptr)
    REJECT_MSG("null out", c.o = nullptr)
    REJECT_MSG("struct_size", c.out.struct_size -= 8)
    REJECT_MSG("pairs < 0", c.n_pairs = -1)
    REJECT_MSG("pairs > 65535", c.n_pairs = 65536)
    REJECT_MSG("rounds 0", c.prm.rounds = 0)
    REJECT_MSG("rounds 9", c.prm.rounds = 9)
    REJECT_MSG("rounds max", c.prm.rounds = 0xffffffffu)
    REJECT_MSG("dist 0", c.prm.max_dist2 = 0.0)
    REJECT_MSG("dist < 0", c.prm.max_dist2 = -4.0)
    REJECT_MSG("dist nan", c.prm.max_dist2 = std::nan(""))
    REJECT_MSG("dist inf", c.prm.max_dist2 = HUGE_VAL)
    REJECT_MSG("den 0 with epipolar_models", c.prm.degenerate_den = 0)
    REJECT_MSG("null models_in", c.md = nullptr)
    REJECT_MSG("null matches", c.m = nullptr)
    REJECT_MSG("null counts", c.mc = nullptr)
    REJECT_MSG("null query", c.qp = nullptr)
    REJECT_MSG("null train", c.tp = nullptr)
    REJECT_MSG("match_cap 0", c.match_cap = 0)
    REJECT_MSG("query_cap 0", c.query_cap = 0)
    REJECT_MSG("train_cap 0", c.train_cap = 0)
    REJECT_MSG("no models", c.out.models = nullptr)
    // a buffer one record short, for each output
    REJECT_MSG("models short", c.out.models_bytes -= sizeof(vslam_homography))
    REJECT_MSG("models small", c.out.models_bytes -= 1)
    REJECT_MSG("info short", c.out.info_bytes -= sizeof(vslam_hrefit))
    REJECT_MSG("info small", c.out.info_bytes -= 1)
    REJECT_MSG("bits short", c.out.inlier_bits_bytes -= 8)
    REJECT_MSG("bits small", c.out.inlier_bits_bytes -= 1)
    REJECT_MSG("inliers without counts", c.out.inlier_counts = nullptr)
    REJECT_MSG("inliers without cap", c.out.inlier_cap = 0)
    REJECT_MSG("inliers short", c.out.inliers_bytes -= sizeof(vslam_match))
    REJECT_MSG("inliers small", c.out.inliers_bytes -= 1)
    REJECT_MSG("counts short", c.out.inlier_counts_bytes -= sizeof(uint32_t))
    REJECT_MSG("counts small", c.out.inlier_counts_bytes -= 1)
    REJECT_MSG("gated without epipolar_models", c.epi = nullptr)
    REJECT_MSG("gated short", c.out.gated_models_bytes -= sizeof(vslam_epipolar))
    REJECT_MSG("gated small", c.out.gated_models_bytes -= 1)
    {
        // the header's order: of two things wrong, the earlier check speaks
        Call c;
        c.out.struct_size -= 8, c.n_pairs = -1;
        args.expect(c.says("struct_size"), "order: struct_size before pairs");
        c.out.struct_size += 8, c.prm.rounds = 0;
        args.expect(c.says("pairs"), "order: pairs before rounds");
        c.n_pairs = 3, c.prm.max_dist2 = 0.0;
        args.expect(c.says("rounds"), "order: rounds before max_dist2");
        c.prm.rounds = 4, c.prm.degenerate_den = 0;
        args.expect(c.says("max_dist2"), "order: max_dist2 before degenerate_den");
        c.prm.max_dist2 = 4.0, c.m = nullptr;
        args.expect(c.says("degenerate_den"), "order: degenerate_den before the inputs");
        c.prm.degenerate_den = 2, c.match_cap = 0;
        args.expect(c.says("null input"), "order: null input before the capacities");
        c.m = c.matches, c.out.models = nullptr;
        args.expect(c.says("capacity"), "order: capacities before the buffers");
        c.match_cap = 100, c.out.info_bytes = 0;
        args.expect(c.says("models is required"), "order: models before info");
        c.out.models = c.models, c.epi = nullptr;
        args.expect(c.says("info buffer"), "order: info before gated_models");
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
