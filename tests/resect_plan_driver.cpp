// Host driver of tests/test_resect_cpu.py: the argument checks and the grid and scratch sizing of vslam_resect_dev
// (visualslam_amd/csrc/vslam_resect_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities,
// pair counts and hypothesis counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the
// blocks cover the capacities, the tiles are dealt to 1 .. EPI_MAX_SPLIT workgroups, and every scratch size equal to its
// product computed in 128 bits (nothing wrapped).  Then every rejection of the ABI, over pointers it never follows, a buffer
// one record short for each output, and the order of the checks: of two things wrong, which one is reported.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_resect_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_pose poses[1];
    vslam_match matches[1];
    uint32_t counts[1];
    double points[3];
    uint64_t bits[1];
    vslam_point train[1];
    vslam_resect models[1];
    vslam_resect_params prm{512, 1, 4.0, {800.0, 800.0, 960.0, 540.0}};
    vslam_resect_out out{};
    uint32_t match_cap = 100, point_cap = 50, obs_cap = 70, train_cap = 60;
    int n_pairs = 3;
    const vslam_pose* ps = poses;
    const vslam_match *m = matches, *om = matches;
    const uint32_t *mc = counts, *oc = counts;
    const double* pt = points;
    const uint64_t* fb = bits;
    const vslam_point* tp = train;
    const vslam_resect_params* p = &prm;
    const vslam_resect_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.models = models;
        out.models_bytes = 3 * sizeof(vslam_resect);
        out.inlier_bits = bits;
        out.inlier_bits_bytes = 3 * 2 * 8;
        out.hypotheses = reinterpret_cast<vslam_resect_hyp*>(matches);
        out.hypotheses_bytes = (size_t)3 * 512 * sizeof(vslam_resect_hyp);
        out.correspondences = reinterpret_cast<vslam_resect_corr*>(matches);
        out.correspondences_bytes = (size_t)3 * 70 * sizeof(vslam_resect_corr);
        out.links = reinterpret_cast<int32_t*>(counts);
        out.links_bytes = (size_t)3 * 70 * sizeof(int32_t);
    }
    const char* why() const { return resect_check_args(ps, m, mc, match_cap, pt, fb, point_cap, om, oc, obs_cap, tp, train_cap, n_pairs, p, o); }
    bool valid() const { return why() == nullptr; }
    bool says(const char* word) const { return why() && std::strstr(why(), word); }
};
}  // namespace

int main() {
    static_assert(sizeof(vslam_resect_hyp) == 104 && sizeof(vslam_resect) == 120 && sizeof(vslam_resect_corr) == 48, "record layouts");
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    const uint32_t hyps[] = {1, 63, 64, 65, 255, 256, 257, 512, 65534, 65535};
    const uint32_t others[] = {1, 257, 0xffffffffu};  // the structure side's match_cap and point_cap, crossed with the observation capacity
    for (uint32_t cap : caps)
        for (int np : pairs)
            for (uint32_t nh : hyps)
                for (uint32_t oth : others) {
                    const ResectPlan p = resect_plan(oth, oth, cap, np, nh);
                    const unsigned __int128 c = cap, n = (unsigned)np, s = oth, lim = (unsigned __int128)1 << 63;
                    plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np, nh);
                    plan.expect((unsigned __int128)p.rec_blocks * TWOVIEW_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                                    ((unsigned __int128)p.rec_blocks - 1) * TWOVIEW_REC_WG < c, "rec_blocks", cap, np, nh);
                    plan.expect((unsigned __int128)p.struct_rec_blocks * TWOVIEW_REC_WG >= s && p.struct_rec_blocks >= 1 && p.struct_rec_blocks < (1u << 31) &&
                                    ((unsigned __int128)p.struct_rec_blocks - 1) * TWOVIEW_REC_WG < s, "struct_rec_blocks", oth, np, nh);
                    plan.expect((unsigned __int128)p.struct_fwords * 64 >= s && ((unsigned __int128)p.struct_fwords - 1) * 64 < s, "struct_fwords", oth, np, nh);
                    plan.expect(p.model_blocks >= 1 && p.model_blocks * RES_MODEL_WG >= nh && (p.model_blocks - 1) * RES_MODEL_WG < nh, "model_blocks", cap, np, nh);
                    plan.expect(p.score_blocks >= 1 && p.score_blocks * EPI_SCORE_WG >= nh && (p.score_blocks - 1) * EPI_SCORE_WG < nh, "score_blocks", cap, np, nh);
                    plan.expect((unsigned __int128)p.tiles * EPI_TILE >= c && ((unsigned __int128)p.tiles - 1) * EPI_TILE < c, "tiles", cap, np, nh);
                    plan.expect(p.nsplit >= 1 && p.nsplit <= EPI_MAX_SPLIT && p.nsplit <= p.tiles, "nsplit", cap, np, nh);
                    plan.expect(np <= 65535 && p.link_pairs == (unsigned)np - 1 && p.link_pairs <= 65534, "grid.y / grid.z", cap, np, nh);
                    plan.expect((unsigned __int128)p.table_elems == (n - 1) * s && (unsigned __int128)p.table_elems * 4 < lim, "table", oth, np, nh);
                    plan.expect((unsigned __int128)p.rec_elems == n * c && (unsigned __int128)p.rec_elems * sizeof(vslam_resect_corr) < lim, "records", cap, np, nh);
                    plan.expect((unsigned __int128)p.hyp_elems == n * nh && (unsigned __int128)p.hyp_elems * sizeof(vslam_resect_hyp) < lim, "hyp", cap, np, nh);
                    plan.expect((unsigned __int128)p.flag_words == n * p.fwords && (unsigned __int128)p.flag_words * 8 < lim, "flags", cap, np, nh);
                    plan.expect(p.pair_elems == (size_t)np, "pair_elems", cap, np, nh);
                }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.n_pairs = 1;
        args.expect(c.valid(), "one pair");
        c.n_pairs = 3;
        c.om = c.m, c.oc = c.mc;
        args.expect(c.valid(), "the observation list aliased onto the structure list");
        c.out.inlier_bits = nullptr, c.out.hypotheses = nullptr, c.out.correspondences = nullptr, c.out.links = nullptr;
        c.out.inlier_bits_bytes = c.out.hypotheses_bytes = c.out.correspondences_bytes = c.out.links_bytes = 0;
        args.expect(c.valid(), "models alone");
        c.prm.n_hypotheses = 1;
        args.expect(c.valid(), "1 hypothesis");
        c.prm.n_hypotheses = 65535;
        args.expect(c.valid(), "65535 hypotheses");
        c.prm.K.cx = -1e300, c.prm.K.cy = 0.0, c.prm.K.fx = 5e-324;
        args.expect(c.valid(), "extreme intrinsics");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = c.point_cap = c.obs_cap = c.train_cap = 0xffffffffu, c.prm.n_hypotheses = 65535;  // the largest call
        c.out.models_bytes = 65535 * sizeof(vslam_resect);
        c.out.inlier_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        c.out.hypotheses_bytes = (size_t)65535 * 65535 * sizeof(vslam_resect_hyp);
        c.out.correspondences_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_resect_corr);
        c.out.links_bytes = (size_t)65535 * 0xffffffffu * sizeof(int32_t);
        args.expect(c.valid(), "largest");
        c.out.correspondences_bytes -= 1;
        args.expect(!c.valid(), "largest correspondences - 1");
        c.out.correspondences_bytes += 1, c.out.inlier_bits_bytes -= 1;
        args.expect(!c.valid(), "largest bits - 1");
        c.out.inlier_bits_bytes += 1, c.out.hypotheses_bytes -= 1;
        args.expect(!c.valid(), "largest hypotheses - 1");
        c.out.hypotheses_bytes += 1, c.out.models_bytes -= 1;
        args.expect(!c.valid(), "largest models - 1");
        c.out.models_bytes += 1, c.out.links_bytes -= 1;
        args.expect(!c.valid(), "largest links - 1");
        c.out.links_bytes += 1;
        args.expect(c.valid(), "largest again");
    }
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("null poses", c.ps = nullptr)
    REJECT("null matches", c.m = nullptr)
    REJECT("null counts", c.mc = nullptr)
    REJECT("null points", c.pt = nullptr)
    REJECT("null bits", c.fb = nullptr)
    REJECT("null obs", c.om = nullptr)
    REJECT("null obs counts", c.oc = nullptr)
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
    REJECT("fx 0", c.prm.K.fx = 0.0)
    REJECT("fy < 0", c.prm.K.fy = -800.0)
    REJECT("fx nan", c.prm.K.fx = std::nan(""))
    REJECT("fy inf", c.prm.K.fy = HUGE_VAL)
    REJECT("cx nan", c.prm.K.cx = std::nan(""))
    REJECT("cy inf", c.prm.K.cy = -HUGE_VAL)
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("point_cap 0", c.point_cap = 0)
    REJECT("obs_cap 0", c.obs_cap = 0)
    REJECT("train_cap 0", c.train_cap = 0)
    REJECT("no models", c.out.models = nullptr)
    // a buffer one record short, for each output
    REJECT("models short", c.out.models_bytes -= sizeof(vslam_resect))
    REJECT("models small", c.out.models_bytes -= 1)
    REJECT("bits short", c.out.inlier_bits_bytes -= 8)
    REJECT("bits small", c.out.inlier_bits_bytes -= 1)
    REJECT("hypotheses short", c.out.hypotheses_bytes -= sizeof(vslam_resect_hyp))
    REJECT("hypotheses small", c.out.hypotheses_bytes -= 1)
    REJECT("correspondences short", c.out.correspondences_bytes -= sizeof(vslam_resect_corr))
    REJECT("correspondences small", c.out.correspondences_bytes -= 1)
    REJECT("links short", c.out.links_bytes -= sizeof(int32_t))
    REJECT("links small", c.out.links_bytes -= 1)
    {
        // the header's order: of two things wrong, the earlier check speaks
        Call c;
        c.out.struct_size -= 8, c.n_pairs = -1;
        args.expect(c.says("struct_size"), "order: struct_size before pairs");
        c.out.struct_size += 8, c.prm.n_hypotheses = 0;
        args.expect(c.says("pairs"), "order: pairs before hypotheses");
        c.n_pairs = 3, c.prm.max_dist2 = 0.0;
        args.expect(c.says("hypotheses"), "order: hypotheses before max_dist2");
        c.prm.n_hypotheses = 512, c.prm.K.cx = HUGE_VAL;
        args.expect(c.says("max_dist2"), "order: max_dist2 before the intrinsics");
        c.prm.max_dist2 = 4.0, c.prm.K.fx = 0.0;
        args.expect(c.says("not finite"), "order: finite before positive");
        c.prm.K.cx = 960.0, c.m = nullptr;
        args.expect(c.says("positive"), "order: the intrinsics before the inputs");
        c.prm.K.fx = 800.0, c.match_cap = 0;
        args.expect(c.says("null input"), "order: null input before the capacities");
        c.m = c.matches, c.om = nullptr;
        args.expect(c.says("capacity"), "order: the structure side before the observation side");
        c.match_cap = 100, c.obs_cap = 0;
        args.expect(c.says("null input"), "order: null observation input before its capacities");
        c.om = c.matches, c.out.models = nullptr;
        args.expect(c.says("capacity"), "order: capacities before the buffers");
        c.obs_cap = 70, c.out.inlier_bits_bytes = 0;
        args.expect(c.says("models is required"), "order: models before inlier_bits");
        c.out.models = c.models, c.out.hypotheses_bytes = 0;
        args.expect(c.says("inlier_bits buffer"), "order: inlier_bits before hypotheses");
        c.out.inlier_bits_bytes = 3 * 2 * 8, c.out.correspondences_bytes = 0;
        args.expect(c.says("hypotheses buffer"), "order: hypotheses before correspondences");
        c.out.hypotheses_bytes = (size_t)3 * 512 * sizeof(vslam_resect_hyp), c.out.links_bytes = 0;
        args.expect(c.says("correspondences buffer"), "order: correspondences before links");
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
