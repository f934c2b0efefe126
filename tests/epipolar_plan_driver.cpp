// Host driver of tests/test_epipolar_cpu.py: the argument checks and the grid and scratch sizing of vslam_epipolar_dev
// (visualslam_amd/csrc/vslam_epipolar_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities,
// pair counts and hypothesis counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the
// record and hypothesis blocks cover the capacities, the split within 1 .. min(tiles, EPI_MAX_SPLIT), and every scratch size
// equal to its product computed in 128 bits (nothing wrapped).  Then every rejection of the ABI, over pointers it never follows.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_epipolar_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_epipolar_params prm{512, 1, 4.0};
    vslam_epipolar_out out{};
    uint32_t match_cap = 100, query_cap = 50, train_cap = 60;
    int n_pairs = 3;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const vslam_point *qp = points, *tp = points;
    const vslam_epipolar_params* p = &prm;
    const vslam_epipolar_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.models = reinterpret_cast<vslam_epipolar*>(matches);
        out.models_bytes = 3 * sizeof(vslam_epipolar);
        out.inlier_bits = reinterpret_cast<uint64_t*>(matches);
        out.inlier_bits_bytes = 3 * 2 * 8;
        out.inliers = matches;
        out.inliers_bytes = 3 * 10 * sizeof(vslam_match);
        out.inlier_counts = counts;
        out.inlier_counts_bytes = 3 * 4;
        out.inlier_cap = 10;
        out.hypotheses = reinterpret_cast<vslam_epipolar_hyp*>(matches);
        out.hypotheses_bytes = 3 * 512 * sizeof(vslam_epipolar_hyp);
    }
    bool valid() const { return epipolar_check_args(m, mc, match_cap, qp, query_cap, tp, train_cap, n_pairs, p, o) == nullptr; }
};
}  // namespace

int main() {
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 255, 256, 2047, 2048, 2049, 65534, 65535};
    const uint32_t hyps[] = {1, 2, 63, 64, 65, 255, 256, 257, 512, 2048, 65534, 65535};
    for (uint32_t cap : caps)
        for (int np : pairs)
            for (uint32_t H : hyps) {
                const EpipolarPlan p = epipolar_plan(cap, np, H);
                const unsigned __int128 c = cap, n = (unsigned)np, h = H;
                plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np, H);
                plan.expect((unsigned __int128)p.rec_blocks * 256 >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31), "rec_blocks", cap, np, H);
                plan.expect((unsigned __int128)p.model_blocks * EPI_MODEL_WG >= h && p.model_blocks >= 1 && (p.model_blocks - 1) * EPI_MODEL_WG < H, "model_blocks", cap, np, H);
                plan.expect((unsigned __int128)p.score_blocks * EPI_SCORE_WG >= h && p.score_blocks >= 1 && (p.score_blocks - 1) * EPI_SCORE_WG < H, "score_blocks", cap, np, H);
                plan.expect((unsigned __int128)p.tiles * EPI_TILE >= c && p.tiles >= 1, "tiles", cap, np, H);
                plan.expect(p.nsplit >= 1 && p.nsplit <= EPI_MAX_SPLIT && p.nsplit <= p.tiles && p.nsplit <= 65535, "nsplit", cap, np, H);
                plan.expect((unsigned __int128)p.coords_elems == n * c && (unsigned __int128)p.coords_elems * 32 < ((unsigned __int128)1 << 63), "coords", cap, np, H);
                plan.expect((unsigned __int128)p.hyp_elems == n * h && (unsigned __int128)p.hyp_elems * 80 < ((unsigned __int128)1 << 63), "hyp", cap, np, H);
                plan.expect((unsigned __int128)p.flag_words == n * p.fwords, "flag_words", cap, np, H);
            }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.n_pairs = 65535, c.match_cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.models_bytes = 65535 * sizeof(vslam_epipolar);
        c.out.inlier_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        c.out.inlier_cap = 0xffffffffu;
        c.out.inliers_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_match);
        c.out.inlier_counts_bytes = 65535 * 4;
        c.prm.n_hypotheses = 65535;
        c.out.hypotheses_bytes = (size_t)65535 * 65535 * sizeof(vslam_epipolar_hyp);
        args.expect(c.valid(), "largest");
        c.out.inliers_bytes -= 1;
        args.expect(!c.valid(), "largest inliers - 1");
        c.out.inliers_bytes += 1, c.out.inlier_bits_bytes -= 1;
        args.expect(!c.valid(), "largest bits - 1");
        c.out.inlier_bits_bytes += 1, c.out.hypotheses_bytes -= 1;
        args.expect(!c.valid(), "largest hypotheses - 1");
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
    REJECT("H 0", c.prm.n_hypotheses = 0)
    REJECT("H 65536", c.prm.n_hypotheses = 65536)
    REJECT("dist 0", c.prm.max_dist2 = 0.0)
    REJECT("dist < 0", c.prm.max_dist2 = -4.0)
    REJECT("dist nan", c.prm.max_dist2 = std::nan(""))
    REJECT("dist inf", c.prm.max_dist2 = HUGE_VAL)
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("query_cap 0", c.query_cap = 0)
    REJECT("train_cap 0", c.train_cap = 0)
    REJECT("no models", c.out.models = nullptr)
    REJECT("models small", c.out.models_bytes -= 1)
    REJECT("bits small", c.out.inlier_bits_bytes -= 1)
    REJECT("inliers small", c.out.inliers_bytes -= 1)
    REJECT("inliers without counts", c.out.inlier_counts = nullptr)
    REJECT("inlier_cap 0", c.out.inlier_cap = 0)
    REJECT("counts small", c.out.inlier_counts_bytes -= 1)
    REJECT("hypotheses small", c.out.hypotheses_bytes -= 1)
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
