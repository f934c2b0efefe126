// Host driver of tests/test_hpose_cpu.py: the argument checks and the grid and scratch sizing of vslam_hpose_dev
// (visualslam_amd/csrc/vslam_hpose_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities and
// pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the record and pair blocks
// cover the capacities, and every scratch size equal to its product computed in 128 bits (nothing wrapped).  Then every
// rejection of the ABI, over pointers it never follows, each buffer one record short, and the order of the checks; and the
// message of every check, one "msg <case>|<message>" line each ("-": the call is valid).
//   driver          "plan checked=N bad=B first=...", "args checked=N bad=B first=...", "order checked=N bad=B first=...", msg lines
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_hpose_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_point points[1];
    vslam_homography models[1];
    vslam_hpose_params prm{{800.0, 800.0, 960.0, 540.0}, 4.0, 0.03, 9, 10, 1, 0};
    vslam_hpose_out out{};
    uint32_t match_cap = 100, query_cap = 50, train_cap = 60;
    int n_pairs = 3;
    const vslam_homography* md = models;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const vslam_point *qp = points, *tp = points;
    const vslam_hpose_params* p = &prm;
    const vslam_hpose_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.poses = reinterpret_cast<vslam_pose*>(matches);
        out.poses_bytes = 3 * sizeof(vslam_pose);
        out.info = reinterpret_cast<vslam_hpose*>(matches);
        out.info_bytes = 3 * sizeof(vslam_hpose);
        out.candidates = reinterpret_cast<vslam_hpose_cand*>(matches);
        out.candidates_bytes = 3 * 4 * sizeof(vslam_hpose_cand);
        out.points = reinterpret_cast<double*>(matches);
        out.points_bytes = 3 * 100 * 3 * sizeof(double);
        out.front_bits = reinterpret_cast<uint64_t*>(matches);
        out.front_bits_bytes = 3 * 2 * 8;
    }
    const char* why() const { return hpose_check_args(md, m, mc, match_cap, qp, query_cap, tp, train_cap, n_pairs, p, o); }
    bool valid() const { return why() == nullptr; }
};
}  // namespace

// One change to a valid call and the message it gets.
#define MSG(what, stmt)                                            \
    {                                                              \
        Call c;                                                    \
        stmt;                                                      \
        const char* w = c.why();                                   \
        std::printf("msg %s|%s\n", what, w ? w : "-");             \
    }
// Two faults at once: the message is the one of the check that comes first.
#define FIRST(what, stmt, want)                                                \
    {                                                                          \
        Call c;                                                                \
        stmt;                                                                  \
        const char* w = c.why();                                               \
        order.expect(w && std::strcmp(w, want) == 0, what);                    \
    }

int main() {
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t cap : caps)
        for (int np : pairs) {
            const HposePlan p = hpose_plan(cap, np);
            const unsigned __int128 c = cap, n = (unsigned)np;
            plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np);
            plan.expect((unsigned __int128)p.rec_blocks * HPOSE_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                            ((unsigned __int128)p.rec_blocks - 1) * HPOSE_REC_WG < c, "rec_blocks", cap, np);
            plan.expect((unsigned __int128)p.pair_blocks * HPOSE_PAIR_WG >= n && p.pair_blocks >= 1 && (p.pair_blocks - 1) * HPOSE_PAIR_WG < (unsigned)np,
                        "pair_blocks", cap, np);
            plan.expect((unsigned __int128)p.coords_elems == n * c && (unsigned __int128)p.coords_elems * 32 < ((unsigned __int128)1 << 63), "coords", cap, np);
            plan.expect((unsigned __int128)p.cand_elems == n * 4 && (unsigned __int128)p.cand_elems * sizeof(vslam_hpose_cand) < ((unsigned __int128)1 << 63),
                        "cand", cap, np);
            plan.expect((unsigned __int128)p.invd_elems == n * 2, "invd", cap, np);
            // the largest index k_hpose_points forms, (np * cap) * 3 doubles, stays below 2^63 bytes
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
        args.expect(c.valid(), "poses and info alone");
        c.prm.only_degenerate = 0, c.prm.ambiguous_num = 0xffffffffu, c.prm.ambiguous_den = 0xffffffffu;
        args.expect(c.valid(), "every pair, largest ratio");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.poses_bytes = 65535 * sizeof(vslam_pose);
        c.out.info_bytes = 65535 * sizeof(vslam_hpose);
        c.out.candidates_bytes = (size_t)65535 * 4 * sizeof(vslam_hpose_cand);
        c.out.points_bytes = (size_t)65535 * 0xffffffffu * 24;
        c.out.front_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        args.expect(c.valid(), "largest");
        c.out.points_bytes -= 1;
        args.expect(!c.valid(), "largest points - 1");
        c.out.points_bytes += 1, c.out.front_bits_bytes -= 1;
        args.expect(!c.valid(), "largest bits - 1");
        c.out.front_bits_bytes += 1, c.out.candidates_bytes -= 1;
        args.expect(!c.valid(), "largest candidates - 1");
        c.out.candidates_bytes += 1, c.out.info_bytes -= 1;
        args.expect(!c.valid(), "largest info - 1");
        c.out.info_bytes += 1, c.out.poses_bytes -= 1;
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
    REJECT("fx 0", c.prm.K.fx = 0.0)
    REJECT("fx < 0", c.prm.K.fx = -800.0)
    REJECT("fy 0", c.prm.K.fy = 0.0)
    REJECT("fx nan", c.prm.K.fx = std::nan(""))
    REJECT("fy inf", c.prm.K.fy = HUGE_VAL)
    REJECT("cx nan", c.prm.K.cx = std::nan(""))
    REJECT("cy inf", c.prm.K.cy = HUGE_VAL)
    REJECT("max_dist2 0", c.prm.max_dist2 = 0.0)
    REJECT("max_dist2 nan", c.prm.max_dist2 = std::nan(""))
    REJECT("max_dist2 inf", c.prm.max_dist2 = HUGE_VAL)
    REJECT("min_spread 0", c.prm.min_spread = 0.0)
    REJECT("min_spread < 0", c.prm.min_spread = -1.0)
    REJECT("min_spread nan", c.prm.min_spread = std::nan(""))
    REJECT("min_spread inf", c.prm.min_spread = HUGE_VAL)
    REJECT("den 0", c.prm.ambiguous_den = 0)
    REJECT("only_degenerate 2", c.prm.only_degenerate = 2)
    REJECT("only_degenerate -1", c.prm.only_degenerate = -1)
    REJECT("reserved", c.prm.reserved = 1)
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("query_cap 0", c.query_cap = 0)
    REJECT("train_cap 0", c.train_cap = 0)
    REJECT("no poses", c.out.poses = nullptr)
    REJECT("no info", c.out.info = nullptr)
    // each buffer one record short
    REJECT("poses short", c.out.poses_bytes = 2 * sizeof(vslam_pose))
    REJECT("info short", c.out.info_bytes = 2 * sizeof(vslam_hpose))
    REJECT("candidates short", c.out.candidates_bytes = 11 * sizeof(vslam_hpose_cand))
    REJECT("points short", c.out.points_bytes = (3 * 100 - 1) * 24)
    REJECT("bits short", c.out.front_bits_bytes = 5 * 8)
    REJECT("poses one byte", c.out.poses_bytes -= 1)
    REJECT("info one byte", c.out.info_bytes -= 1)
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);

    // the order: null, struct_size, n_pairs, the parameters (K, max_dist2, min_spread, den, only_degenerate, reserved), the inputs, the buffers
    Tally order;
    FIRST("struct_size before pairs", (c.out.struct_size = 0, c.n_pairs = -1), "out->struct_size is not sizeof(vslam_hpose_out)")
    FIRST("pairs before K", (c.n_pairs = 65536, c.prm.K.fx = 0.0), "0 .. 65535 pairs per call")
    FIRST("K finite before positive", (c.prm.K.fx = 0.0, c.prm.K.cy = HUGE_VAL), "the intrinsics must be finite")
    FIRST("K before max_dist2", (c.prm.K.fy = -1.0, c.prm.max_dist2 = 0.0), "fx and fy must be positive")
    FIRST("max_dist2 before min_spread", (c.prm.max_dist2 = 0.0, c.prm.min_spread = 0.0), "max_dist2 must be finite and positive")
    FIRST("min_spread before den", (c.prm.min_spread = 0.0, c.prm.ambiguous_den = 0), "min_spread must be finite and positive")
    FIRST("den before only_degenerate", (c.prm.ambiguous_den = 0, c.prm.only_degenerate = 2), "ambiguous_den must be positive")
    FIRST("only_degenerate before reserved", (c.prm.only_degenerate = 2, c.prm.reserved = 7), "only_degenerate must be 0 or 1")
    FIRST("reserved before inputs", (c.prm.reserved = 7, c.md = nullptr), "reserved must be 0")
    FIRST("null input before capacity", (c.m = nullptr, c.match_cap = 0), "null input")
    FIRST("capacity before buffers", (c.train_cap = 0, c.out.poses = nullptr), "a capacity is zero")
    FIRST("poses before info", (c.out.poses = nullptr, c.out.info = nullptr), "poses is required")
    FIRST("poses size before info", (c.out.poses_bytes = 0, c.out.info = nullptr), "poses buffer too small")
    FIRST("info before candidates", (c.out.info_bytes = 0, c.out.candidates_bytes = 0), "info buffer too small")
    FIRST("candidates before points", (c.out.candidates_bytes = 0, c.out.points_bytes = 0), "candidates buffer too small")
    FIRST("points before bits", (c.out.points_bytes = 0, c.out.front_bits_bytes = 0), "points buffer too small")
    std::printf("order checked=%ld bad=%ld first=%s\n", order.checked, order.bad, order.first);

    MSG("valid", (void)0)
    MSG("null params", c.p = nullptr)
    MSG("null out", c.o = nullptr)
    MSG("struct_size", c.out.struct_size -= 8)
    MSG("pairs < 0", c.n_pairs = -1)
    MSG("pairs > 65535", c.n_pairs = 65536)
    MSG("fx nan", c.prm.K.fx = std::nan(""))
    MSG("cy inf", c.prm.K.cy = HUGE_VAL)
    MSG("fx zero", c.prm.K.fx = 0.0)
    MSG("fy negative", c.prm.K.fy = -1.0)
    MSG("max_dist2 nan", c.prm.max_dist2 = std::nan(""))
    MSG("max_dist2 zero", c.prm.max_dist2 = 0.0)
    MSG("min_spread nan", c.prm.min_spread = std::nan(""))
    MSG("min_spread zero", c.prm.min_spread = 0.0)
    MSG("den zero", c.prm.ambiguous_den = 0)
    MSG("only_degenerate 2", c.prm.only_degenerate = 2)
    MSG("reserved", c.prm.reserved = 1)
    MSG("null models", c.md = nullptr)
    MSG("null train", c.tp = nullptr)
    MSG("query_cap 0", c.query_cap = 0)
    MSG("null poses", c.out.poses = nullptr)
    MSG("poses short", c.out.poses_bytes -= 1)
    MSG("null info", c.out.info = nullptr)
    MSG("info short", c.out.info_bytes -= 1)
    MSG("candidates short", c.out.candidates_bytes -= 1)
    MSG("points short", c.out.points_bytes -= 1)
    MSG("front_bits short", c.out.front_bits_bytes -= 1)
    MSG("poses and info alone", (c.out.candidates = nullptr, c.out.points = nullptr, c.out.front_bits = nullptr))
    return plan.bad || args.bad || order.bad ? 1 : 0;
}
