// Host driver of tests/test_pose_cpu.py: the argument checks and the grid and scratch sizing of vslam_pose_dev
// (visualslam_amd/csrc/vslam_pose_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities and
// pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the record and pair blocks
// cover the capacities, and every scratch size equal to its product computed in 128 bits (nothing wrapped).  Then every
// rejection of the ABI, over pointers it never follows.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_pose_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_epipolar models[1];
    vslam_pose_params prm{800.0, 800.0, 960.0, 540.0};
    vslam_pose_out out{};
    uint32_t match_cap = 100, query_cap = 50, train_cap = 60;
    int n_pairs = 3;
    const vslam_epipolar* md = models;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const vslam_point *qp = points, *tp = points;
    const vslam_pose_params* p = &prm;
    const vslam_pose_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.poses = reinterpret_cast<vslam_pose*>(matches);
        out.poses_bytes = 3 * sizeof(vslam_pose);
        out.candidates = reinterpret_cast<vslam_pose_cand*>(matches);
        out.candidates_bytes = 3 * 4 * sizeof(vslam_pose_cand);
        out.points = reinterpret_cast<double*>(matches);
        out.points_bytes = 3 * 100 * 3 * sizeof(double);
        out.front_bits = reinterpret_cast<uint64_t*>(matches);
        out.front_bits_bytes = 3 * 2 * 8;
    }
    bool valid() const { return pose_check_args(md, m, mc, match_cap, qp, query_cap, tp, train_cap, n_pairs, p, o) == nullptr; }
};
}  // namespace

int main() {
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t cap : caps)
        for (int np : pairs) {
            const PosePlan p = pose_plan(cap, np);
            const unsigned __int128 c = cap, n = (unsigned)np;
            plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np);
            plan.expect((unsigned __int128)p.rec_blocks * POSE_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                            ((unsigned __int128)p.rec_blocks - 1) * POSE_REC_WG < c, "rec_blocks", cap, np);
            plan.expect((unsigned __int128)p.pair_blocks * POSE_PAIR_WG >= n && p.pair_blocks >= 1 && (p.pair_blocks - 1) * POSE_PAIR_WG < (unsigned)np,
                        "pair_blocks", cap, np);
            plan.expect((unsigned __int128)p.coords_elems == n * c && (unsigned __int128)p.coords_elems * 32 < ((unsigned __int128)1 << 63), "coords", cap, np);
            plan.expect((unsigned __int128)p.cand_elems == n * 4 && (unsigned __int128)p.cand_elems * sizeof(vslam_pose_cand) < ((unsigned __int128)1 << 63),
                        "cand", cap, np);
            // the largest index k_pose_points forms, (np * cap) * 3 doubles, stays below 2^63 bytes
            plan.expect(n * c * 24 < ((unsigned __int128)1 << 63), "points", cap, np);
        }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.out.candidates = nullptr, c.out.points = nullptr, c.out.front_bits = nullptr;
        c.out.candidates_bytes = c.out.points_bytes = c.out.front_bits_bytes = 0;
        c.n_pairs = 3;
        args.expect(c.valid(), "poses alone");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.poses_bytes = 65535 * sizeof(vslam_pose);
        c.out.candidates_bytes = (size_t)65535 * 4 * sizeof(vslam_pose_cand);
        c.out.points_bytes = (size_t)65535 * 0xffffffffu * 24;
        c.out.front_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        args.expect(c.valid(), "largest");
        c.out.points_bytes -= 1;
        args.expect(!c.valid(), "largest points - 1");
        c.out.points_bytes += 1, c.out.front_bits_bytes -= 1;
        args.expect(!c.valid(), "largest bits - 1");
        c.out.front_bits_bytes += 1, c.out.candidates_bytes -= 1;
        args.expect(!c.valid(), "largest candidates - 1");
        c.out.candidates_bytes += 1, c.out.poses_bytes -= 1;
        args.expect(!c.valid(), "largest poses - 1");
    }
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("null models", c.md = nullptr)
    REJECT("null matches", c.m = nullptr)
    REJECT("null counts", c.mc = nullptr)
    REJECT("null query", c.qp = nullptr)
    REJECT("null train", c.tp = nullptr)
    REJECT("struct_size", c.out.struct_size -= 8)
    REJECT("pairs < 0", c.n_pairs = -1)
    REJECT("pairs > 65535", c.n_pairs = 65536)
    REJECT("fx 0", c.prm.fx = 0.0)
    REJECT("fx < 0", c.prm.fx = -800.0)
    REJECT("fy 0", c.prm.fy = 0.0)
    REJECT("fy < 0", c.prm.fy = -1.0)
    REJECT("fx nan", c.prm.fx = std::nan(""))
    REJECT("fy inf", c.prm.fy = HUGE_VAL)
    REJECT("cx nan", c.prm.cx = std::nan(""))
    REJECT("cx inf", c.prm.cx = -HUGE_VAL)
    REJECT("cy nan", c.prm.cy = std::nan(""))
    REJECT("cy inf", c.prm.cy = HUGE_VAL)
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("query_cap 0", c.query_cap = 0)
    REJECT("train_cap 0", c.train_cap = 0)
    REJECT("no poses", c.out.poses = nullptr)
    REJECT("poses small", c.out.poses_bytes -= 1)
    REJECT("candidates small", c.out.candidates_bytes -= 1)
    REJECT("points small", c.out.points_bytes -= 1)
    REJECT("bits small", c.out.front_bits_bytes -= 1)
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}
