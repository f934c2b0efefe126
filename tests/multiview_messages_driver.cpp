// Host driver of tests/test_multiview_messages_cpu.py: the message of every rejection of the five multi-view *_check_args
// (vslam_chain_plan.h, vslam_resect_plan.h, vslam_resect_refine_plan.h, vslam_tracks_plan.h, vslam_bundle_plan.h) without a
// GPU, built with -fsanitize=address,undefined.  One valid call per stage over pointers the checks never follow, one field of
// it broken per case, and the whole message printed: the test holds the table of what each must say, byte for byte.
//   driver          one line per case: "<stage>|<case>|<message, or - for a call that is valid>"
#include <cstdio>

#include "vslam_bundle_plan.h"
#include "vslam_chain_plan.h"
#include "vslam_resect_plan.h"

using namespace vslam;

namespace {
// what the pointers of the valid calls point at: never read
vslam_pose poses[1];
vslam_match matches[1];
uint32_t counts[1];
double points[3];
uint64_t bits[1];
vslam_point frames[1];
vslam_chain chains[1];
vslam_track rows[1];
vslam_track_ref refs[1];
alignas(16) vslam_resect_corr corrs[2];
vslam_resect models[8];  // (the refinement compares the addresses of models_in and models)
const vslam_pose_params K{800.0, 800.0, 960.0, 540.0};

struct Common {  // 3 pairs, the structure side's lists and capacities
    uint32_t match_cap = 100, point_cap = 50;
    int n_pairs = 3;
    const vslam_pose* ps = poses;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const uint64_t* fb = bits;
};

struct Chain : Common {
    vslam_chain_params prm{16};
    vslam_chain_out out{sizeof(vslam_chain_out), chains, 3 * 176, points, 3 * 100 * 24, reinterpret_cast<int32_t*>(counts), 3 * 100 * 4, points, 3 * 100 * 8};
    const double* pt = points;
    const vslam_chain_params* p = &prm;
    const vslam_chain_out* o = &out;
    const char* why() const { return chain_check_args(ps, m, mc, match_cap, pt, fb, point_cap, n_pairs, p, o); }
};

struct Resect : Common {
    vslam_resect_params prm{512, 1, 4.0, K};
    vslam_resect_out out{sizeof(vslam_resect_out), models, 3 * 120, bits, 3 * 2 * 8, reinterpret_cast<vslam_resect_hyp*>(matches), 3 * 512 * 104, corrs, 3 * 70 * 48,
                         reinterpret_cast<int32_t*>(counts), 3 * 70 * 4};
    uint32_t obs_cap = 70, train_cap = 60;
    const double* pt = points;
    const vslam_match* om = matches;
    const uint32_t* oc = counts;
    const vslam_point* tp = frames;
    const vslam_resect_params* p = &prm;
    const vslam_resect_out* o = &out;
    const char* why() const { return resect_check_args(ps, m, mc, match_cap, pt, fb, point_cap, om, oc, obs_cap, tp, train_cap, n_pairs, p, o); }
};

struct Refine {
    vslam_resect_refine_params prm{4, 4.0, K};
    vslam_resect_refine_out out{sizeof(vslam_resect_refine_out), models, 3 * 120, reinterpret_cast<vslam_resect_refine*>(points), 3 * 32, bits, 3 * 2 * 8};
    uint32_t obs_cap = 70;
    int n_pairs = 3;
    bool aligned = true;
    const vslam_resect* mi = models;
    const vslam_resect_corr* cs = corrs;
    const vslam_resect_refine_params* p = &prm;
    const vslam_resect_refine_out* o = &out;
    const char* why() const { return resect_refine_check_args(mi, cs, obs_cap, n_pairs, p, o, aligned); }
};

struct Tracks : Common {
    vslam_tracks_params prm{K, 4.0, 2, 0};
    vslam_tracks_out out{sizeof(vslam_tracks_out), rows, 3 * 100 * 48, refs, 3 * 100 * 8, bits, 3 * 2 * 8, reinterpret_cast<vslam_track_summary*>(points), 3 * 16};
    const vslam_chain* ch = chains;
    const vslam_point* fp = frames;
    const vslam_tracks_params* p = &prm;
    const vslam_tracks_out* o = &out;
    const char* why() const { return tracks_check_args(ps, m, mc, match_cap, fb, point_cap, n_pairs, ch, fp, p, o); }
};

struct Bundle : Common {
    vslam_bundle_params prm{K, 4.0, 2, 4};
    vslam_bundle_out out{sizeof(vslam_bundle_out), rows, 3 * 100 * 48, reinterpret_cast<vslam_bundle_cam*>(points), 3 * 160, reinterpret_cast<vslam_bundle_point*>(points),
                         3 * 100 * 40, bits, 3 * 2 * 2 * 8};
    const vslam_chain* ch = chains;
    const vslam_point* fp = frames;
    const vslam_track* ti = rows;
    const vslam_track_ref* rf = refs;
    const vslam_bundle_params* p = &prm;
    const vslam_bundle_out* o = &out;
    const char* why() const { return bundle_check_args(ps, m, mc, match_cap, fb, point_cap, n_pairs, ch, fp, ti, rf, p, o); }
};
}  // namespace

// A valid call of `Stage`, one change to it, and what the checks say then.
#define SAY(Stage, stage, what, stmt)                           \
    {                                                           \
        Stage c;                                                \
        stmt;                                                   \
        const char* why = c.why();                              \
        std::printf("%s|%s|%s\n", stage, what, why ? why : "-"); \
    }
#define COMMON(Stage, stage)                                  \
    SAY(Stage, stage, "valid", (void)0)                       \
    SAY(Stage, stage, "null params", c.p = nullptr)           \
    SAY(Stage, stage, "null out", c.o = nullptr)              \
    SAY(Stage, stage, "struct_size", c.out.struct_size -= 8)  \
    SAY(Stage, stage, "pairs < 0", c.n_pairs = -1)            \
    SAY(Stage, stage, "pairs > 65535", c.n_pairs = 65536)
#define INTRINSICS(Stage, stage)                              \
    SAY(Stage, stage, "fx nan", c.prm.K.fx = NAN)             \
    SAY(Stage, stage, "cy inf", c.prm.K.cy = INFINITY)        \
    SAY(Stage, stage, "fx zero", c.prm.K.fx = 0.0)            \
    SAY(Stage, stage, "fy negative", c.prm.K.fy = -800.0)
#define MAX_DIST2(Stage, stage)                               \
    SAY(Stage, stage, "max_dist2 nan", c.prm.max_dist2 = NAN) \
    SAY(Stage, stage, "max_dist2 zero", c.prm.max_dist2 = 0.0)

int main() {
    COMMON(Chain, "chain")
    SAY(Chain, "chain", "min_links 0", c.prm.min_links = 0)
    SAY(Chain, "chain", "null points", c.pt = nullptr)
    SAY(Chain, "chain", "match_cap 0", c.match_cap = 0)
    SAY(Chain, "chain", "null chain", c.out.chain = nullptr)
    SAY(Chain, "chain", "chain short", c.out.chain_bytes -= 1)
    SAY(Chain, "chain", "map short", c.out.map_bytes -= 1)
    SAY(Chain, "chain", "links short", c.out.links_bytes -= 1)
    SAY(Chain, "chain", "ratios short", c.out.ratios_bytes -= 1)
    SAY(Chain, "chain", "chain alone", (c.out.map = nullptr, c.out.links = nullptr, c.out.ratios = nullptr, c.out.map_bytes = c.out.links_bytes = c.out.ratios_bytes = 0))

    COMMON(Resect, "resect")
    SAY(Resect, "resect", "hypotheses 0", c.prm.n_hypotheses = 0)
    MAX_DIST2(Resect, "resect")
    INTRINSICS(Resect, "resect")
    SAY(Resect, "resect", "null poses", c.ps = nullptr)
    SAY(Resect, "resect", "point_cap 0", c.point_cap = 0)
    SAY(Resect, "resect", "null obs_counts", c.oc = nullptr)
    SAY(Resect, "resect", "train_cap 0", c.train_cap = 0)
    SAY(Resect, "resect", "null models", c.out.models = nullptr)
    SAY(Resect, "resect", "models short", c.out.models_bytes -= 1)
    SAY(Resect, "resect", "inlier_bits short", c.out.inlier_bits_bytes -= 1)
    SAY(Resect, "resect", "hypotheses short", c.out.hypotheses_bytes -= 1)
    SAY(Resect, "resect", "correspondences short", c.out.correspondences_bytes -= 1)
    SAY(Resect, "resect", "links short", c.out.links_bytes -= 1)

    COMMON(Refine, "resect_refine")
    SAY(Refine, "resect_refine", "rounds 0", c.prm.rounds = 0)
    SAY(Refine, "resect_refine", "rounds 9", c.prm.rounds = 9)
    MAX_DIST2(Refine, "resect_refine")
    INTRINSICS(Refine, "resect_refine")
    SAY(Refine, "resect_refine", "null models_in", c.mi = nullptr)
    SAY(Refine, "resect_refine", "obs_cap 0", c.obs_cap = 0)
    SAY(Refine, "resect_refine", "unaligned", c.cs = reinterpret_cast<const vslam_resect_corr*>(reinterpret_cast<const char*>(corrs) + 8))
    SAY(Refine, "resect_refine", "unaligned, host", (c.cs = reinterpret_cast<const vslam_resect_corr*>(reinterpret_cast<const char*>(corrs) + 8), c.aligned = false))
    SAY(Refine, "resect_refine", "null models", c.out.models = nullptr)
    SAY(Refine, "resect_refine", "models short", c.out.models_bytes -= 1)
    SAY(Refine, "resect_refine", "info short", c.out.info_bytes -= 1)
    SAY(Refine, "resect_refine", "inlier_bits short", c.out.inlier_bits_bytes -= 1)
    SAY(Refine, "resect_refine", "models one row behind models_in", c.mi = models + 1)

    COMMON(Tracks, "tracks")
    INTRINSICS(Tracks, "tracks")
    MAX_DIST2(Tracks, "tracks")
    SAY(Tracks, "tracks", "min_views 1", c.prm.min_views = 1)
    SAY(Tracks, "tracks", "null chain", c.ch = nullptr)
    SAY(Tracks, "tracks", "point_cap 0", c.point_cap = 0)
    SAY(Tracks, "tracks", "null tracks", c.out.tracks = nullptr)
    SAY(Tracks, "tracks", "tracks short", c.out.tracks_bytes -= 1)
    SAY(Tracks, "tracks", "refs short", c.out.refs_bytes -= 1)
    SAY(Tracks, "tracks", "good_bits short", c.out.good_bits_bytes -= 1)
    SAY(Tracks, "tracks", "summary short", c.out.summary_bytes -= 1)

    COMMON(Bundle, "bundle")
    SAY(Bundle, "bundle", "sweeps 0", c.prm.sweeps = 0)
    SAY(Bundle, "bundle", "sweeps 65", c.prm.sweeps = 65)
    SAY(Bundle, "bundle", "min_views 1", c.prm.min_views = 1)
    MAX_DIST2(Bundle, "bundle")
    INTRINSICS(Bundle, "bundle")
    SAY(Bundle, "bundle", "null refs", c.rf = nullptr)
    SAY(Bundle, "bundle", "match_cap 0", c.match_cap = 0)
    SAY(Bundle, "bundle", "null tracks", c.out.tracks = nullptr)
    SAY(Bundle, "bundle", "tracks short", c.out.tracks_bytes -= 1)
    SAY(Bundle, "bundle", "null cams", c.out.cams = nullptr)
    SAY(Bundle, "bundle", "cams short", c.out.cams_bytes -= 1)
    SAY(Bundle, "bundle", "point_info short", c.out.point_info_bytes -= 1)
    SAY(Bundle, "bundle", "member_bits short", c.out.member_bits_bytes -= 1)
    SAY(Bundle, "bundle", "tracks one row behind tracks_in", c.ti = rows + 1)
    return 0;
}
