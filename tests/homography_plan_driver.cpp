// Host driver of tests/test_homography_cpu.py: the argument checks and the grid and scratch sizing of vslam_homography_dev
// (visualslam_amd/csrc/vslam_homography_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities,
// pair counts and hypothesis counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the
// blocks cover the capacities, the tiles are dealt to 1 .. EPI_MAX_SPLIT workgroups, and every scratch size equal to its
// product computed in 128 bits (nothing wrapped).  Then every rejection of the ABI, over pointers it never follows, a buffer
// one record short for each output, and the order of the checks: of two things wrong, which one is reported.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_homography_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_epipolar epi[1];
    vslam_homography models[1];
    vslam_homography_params prm{512, 1, 4.0, 1, 2, 16};
    vslam_homography_out out{};
    uint32_t match_cap = 100, query_cap = 50, train_cap = 60;
    int n_pairs = 3;
    const vslam_epipolar* em = epi;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const vslam_point *qp = points, *tp = points;
    const vslam_homography_params* p = &prm;
    const vslam_homography_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.models = models;
        out.models_bytes = 3 * sizeof(vslam_homography);
        out.inlier_bits = reinterpret_cast<uint64_t*>(matches);
        out.inlier_bits_bytes = 3 * 2 * 8;
        out.inliers = matches;
        out.inliers_bytes = 3 * 40 * sizeof(vslam_match);
        out.inlier_counts = counts;
        out.inlier_counts_bytes = 3 * sizeof(uint32_t);
        out.inlier_cap = 40;
        out.hypotheses = reinterpret_cast<vslam_homography_hyp*>(matches);
        out.hypotheses_bytes = (size_t)3 * 512 * sizeof(vslam_homography_hyp);
        out.gated_models = epi;  // in place
        out.gated_models_bytes = 3 * sizeof(vslam_epipolar);
    }
    const char* why() const { return homography_check_args(m, mc, match_cap, qp, query_cap, tp, train_cap, n_pairs, em, p, o); }
    bool valid() const { return why() == nullptr; }
    bool says(const char* word) const { return why() && std::strstr(why(), word); }
};
}  // namespace

int main() {
    static_assert(sizeof(vslam_homography_hyp) == 152 && sizeof(vslam_homography) == 168, "record layouts");
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    const uint32_t hyps[] = {1, 63, 64, 65, 255, 256, 257, 512, 65534, 65535};
    for (uint32_t cap : caps)
        for (int np : pairs)
            for (uint32_t nh : hyps) {
                const HomographyPlan p = homography_plan(cap, np, nh);
                const unsigned __int128 c = cap, n = (unsigned)np, lim = (unsigned __int128)1 << 63;
                plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np, nh);
                plan.expect((unsigned __int128)p.rec_blocks * TWOVIEW_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                                ((unsigned __int128)p.rec_blocks - 1) * TWOVIEW_REC_WG < c, "rec_blocks", cap, np, nh);
                plan.expect(p.model_blocks >= 1 && p.model_blocks * HOM_MODEL_WG >= nh && (p.model_blocks - 1) * HOM_MODEL_WG < nh, "model_blocks", cap, np, nh);
                plan.expect(p.score_blocks >= 1 && p.score_blocks * EPI_SCORE_WG >= nh && (p.score_blocks - 1) * EPI_SCORE_WG < nh, "score_blocks", cap, np, nh);
                plan.expect((unsigned __int128)p.tiles * EPI_TILE >= c && ((unsigned __int128)p.tiles - 1) * EPI_TILE < c, "tiles", cap, np, nh);
                plan.expect(p.nsplit >= 1 && p.nsplit <= EPI_MAX_SPLIT && p.nsplit <= p.tiles, "nsplit", cap, np, nh);
                plan.expect(p.pair_blocks >= 1 && (unsigned __int128)p.pair_blocks * HOM_PAIR_WG >= n && (p.pair_blocks - 1) * HOM_PAIR_WG < (unsigned)np,
                            "pair_blocks", cap, np, nh);
                plan.expect(np <= 65535, "grid.y / grid.z", cap, np, nh);
                plan.expect((unsigned __int128)p.coords_elems == n * c && (unsigned __int128)p.coords_elems * 32 < lim, "coords", cap, np, nh);
                plan.expect((unsigned __int128)p.hyp_elems == n * nh && (unsigned __int128)p.hyp_elems * sizeof(vslam_homography_hyp) < lim, "hyp", cap, np, nh);
                plan.expect((unsigned __int128)p.flag_words == n * p.fwords && (unsigned __int128)p.flag_words * 8 < lim, "flags", cap, np, nh);
            }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.n_pairs = 3;
        c.out.gated_models = nullptr, c.out.gated_models_bytes = 0;
        args.expect(c.valid(), "verdict without the gate");
        c.em = nullptr;
        args.expect(c.valid(), "no epipolar models");
        c.out.inlier_bits = nullptr, c.out.inliers = nullptr, c.out.inlier_counts = nullptr, c.out.hypotheses = nullptr;
        c.out.inlier_bits_bytes = c.out.inliers_bytes = c.out.inlier_counts_bytes = c.out.hypotheses_bytes = 0, c.out.inlier_cap = 0;
        args.expect(c.valid(), "models alone");
        c.out.inlier_counts = c.counts, c.out.inlier_counts_bytes = 3 * sizeof(uint32_t);
        args.expect(c.valid(), "totals alone");
        c.prm.n_hypotheses = 1;
        args.expect(c.valid(), "1 hypothesis");
        c.prm.n_hypotheses = 65535;
        args.expect(c.valid(), "65535 hypotheses");
        c.prm.degenerate_num = 0, c.prm.degenerate_den = 0xffffffffu, c.prm.min_inliers = 0xffffffffu;
        args.expect(c.valid(), "extreme verdict parameters");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu, c.out.inlier_cap = 0xffffffffu, c.prm.n_hypotheses = 65535;  // the largest call: the byte sizes it needs, as size_t
        c.out.models_bytes = 65535 * sizeof(vslam_homography);
        c.out.inlier_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        c.out.inliers_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_match);
        c.out.inlier_counts_bytes = 65535 * sizeof(uint32_t);
        c.out.hypotheses_bytes = (size_t)65535 * 65535 * sizeof(vslam_homography_hyp);
        c.out.gated_models_bytes = 65535 * sizeof(vslam_epipolar);
        args.expect(c.valid(), "largest");
        c.out.inliers_bytes -= 1;
        args.expect(!c.valid(), "largest inliers - 1");
        c.out.inliers_bytes += 1, c.out.inlier_bits_bytes -= 1;
        args.expect(!c.valid(), "largest bits - 1");
        c.out.inlier_bits_bytes += 1, c.out.hypotheses_bytes -= 1;
        args.expect(!c.valid(), "largest hypotheses - 1");
        c.out.hypotheses_bytes += 1, c.out.models_bytes -= 1;
        args.expect(!c.valid(), "largest models - 1");
        c.out.models_bytes += 1, c.out.inlier_counts_bytes -= 1;
        args.expect(!c.valid(), "largest counts - 1");
        c.out.inlier_counts_bytes += 1, c.out.gated_models_bytes -= 1;
        args.expect(!c.valid(), "largest gated - 1");
        c.out.gated_models_bytes += 1;
        args.expect(c.valid(), "largest again");
    }
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("null matches", c.m = nullptr)
    REJECT("null counts", c.mc = nullptr)
    REJECT("null query", c.qp = nullptr)
    REJECT("null train", c.tp = nullptr)
    REJECT("struct_size", c.out.struct_size -= 8)
    REJECT("pairs < 0", c.n_pairs = -1)
    REJECT("pairs > 65535", c.n_pairs = 65536)
    REJECT("hypotheses 0", c.prm.n_hypotheses = 0)
    REJECT("hypotheses 65536", c.prm.n_hypotheses = 65536)
    REJECT("hypotheses max", c.prm.n_hypotheses = 0xffffffffu)
    REJECT("dist 0", c.prm.max_dist2 = 0.0)
    REJECT("dist < 0", c.prm.max_dist2 = -4.0)
    REJECT("dist nan", c.prm.max_dist2 = std::nan(""))
    REJECT("dist inf", c.prm.max_dist2 = HUGE_VAL)
    REJECT("den 0", c.prm.degenerate_den = 0)
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("query_cap 0", c.query_cap = 0)
    REJECT("train_cap 0", c.train_cap = 0)
    REJECT("no models", c.out.models = nullptr)
    REJECT("gate without epipolar models", c.em = nullptr)
    // a buffer one record short, for each output
    REJECT("models short", c.out.models_bytes -= sizeof(vslam_homography))
    REJECT("models small", c.out.models_bytes -= 1)
    REJECT("bits short", c.out.inlier_bits_bytes -= 8)
    REJECT("bits small", c.out.inlier_bits_bytes -= 1)
    REJECT("inliers short", c.out.inliers_bytes -= sizeof(vslam_match))
    REJECT("inliers small", c.out.inliers_bytes -= 1)
    REJECT("counts short", c.out.inlier_counts_bytes -= sizeof(uint32_t))
    REJECT("counts small", c.out.inlier_counts_bytes -= 1)
    REJECT("hypotheses short", c.out.hypotheses_bytes -= sizeof(vslam_homography_hyp))
    REJECT("hypotheses small", c.out.hypotheses_bytes -= 1)
    REJECT("gated short", c.out.gated_models_bytes -= sizeof(vslam_epipolar))
    REJECT("gated small", c.out.gated_models_bytes -= 1)
    REJECT("inliers without counts", c.out.inlier_counts = nullptr)
    REJECT("inliers without cap", c.out.inlier_cap = 0)
    {
        // the header's order: of two things wrong, the earlier check speaks
        Call c;
        c.out.struct_size -= 8, c.n_pairs = -1;
        args.expect(c.says("struct_size"), "order: struct_size before pairs");
        c.out.struct_size += 8, c.prm.n_hypotheses = 0;
        args.expect(c.says("pairs"), "order: pairs before hypotheses");
        c.n_pairs = 3, c.prm.max_dist2 = 0.0;
        args.expect(c.says("hypotheses"), "order: hypotheses before max_dist2");
        c.prm.n_hypotheses = 512, c.prm.degenerate_den = 0;
        args.expect(c.says("max_dist2"), "order: max_dist2 before degenerate_den");
        c.prm.max_dist2 = 4.0, c.m = nullptr;
        args.expect(c.says("degenerate_den"), "order: degenerate_den before the inputs");
        c.prm.degenerate_den = 2, c.match_cap = 0;
        args.expect(c.says("null input"), "order: null input before the capacities");
        c.m = c.matches, c.out.models = nullptr;
        args.expect(c.says("capacity"), "order: capacities before the buffers");
        c.match_cap = 100, c.out.hypotheses_bytes = 0;
        args.expect(c.says("models is required"), "order: models before hypotheses");
        c.out.models = c.models, c.em = nullptr;
        args.expect(c.says("hypotheses buffer"), "order: hypotheses before the gate");
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
