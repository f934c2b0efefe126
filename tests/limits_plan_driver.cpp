// Host driver of tests/test_geometry_limits_cpu.py: the grids the plan headers (visualslam_amd/csrc/vslam_*_plan.h) give the calls
// of tests/limitcases.py, without a GPU, built with -fsanitize=address,undefined.  It reads lines
//   stage match_cap/obs_cap point_cap n_pairs n_hypotheses
// (stage: homography, pose, refit, resect, resect_refine, chain, tracks; a field a stage does not take is ignored) and prints
// one line per call: the stage and the plan's fields, name=value - of tiles, nsplit, score_blocks, model_blocks, rec_blocks,
// sum_blocks, pair_blocks, fwords and link_pairs those the stage's plan has.  An unknown stage or a short line: exit status 2.
#include <cstdio>
#include <cstring>

#include "vslam_chain_plan.h"
#include "vslam_homography_plan.h"
#include "vslam_pose_plan.h"
#include "vslam_refit_plan.h"
#include "vslam_resect_plan.h"
#include "vslam_resect_refine_plan.h"
#include "vslam_tracks_plan.h"

using namespace vslam;

namespace {
void score_fields(const EpipolarPlan& p) {
    std::printf(" tiles=%u nsplit=%u score_blocks=%u model_blocks=%u rec_blocks=%u fwords=%u", p.tiles, p.nsplit, p.score_blocks, p.model_blocks, p.rec_blocks,
                p.fwords);
}
}  // namespace

int main() {
    char stage[32];
    unsigned long long cap, pcap, np, nh;
    int got;
    while ((got = std::scanf("%31s %llu %llu %llu %llu", stage, &cap, &pcap, &np, &nh)) == 5) {
        if (cap < 1 || cap > 0xffffffffull || pcap > 0xffffffffull || np < 1 || np > 65535 || nh > 65535) return 2;
        const uint32_t c = (uint32_t)cap, pc = (uint32_t)pcap, h = (uint32_t)nh;
        const int n = (int)np;
        std::printf("%s", stage);
        if (!std::strcmp(stage, "homography")) {
            const HomographyPlan p = homography_plan(c, n, h);
            score_fields(p);
            std::printf(" pair_blocks=%u", p.pair_blocks);
        } else if (!std::strcmp(stage, "pose")) {
            const PosePlan p = pose_plan(c, n);
            std::printf(" rec_blocks=%u fwords=%u pair_blocks=%u", p.rec_blocks, p.fwords, p.pair_blocks);
        } else if (!std::strcmp(stage, "refit")) {
            const RefitPlan p = refit_plan(c, n);
            std::printf(" rec_blocks=%u fwords=%u sum_blocks=%u pair_blocks=%u", p.rec_blocks, p.fwords, p.sum_blocks, p.pair_blocks);
        } else if (!std::strcmp(stage, "resect")) {
            const ResectPlan p = resect_plan(c, pc, c, n, h);  // the structure side at the observation side's capacity
            score_fields(p);
            std::printf(" link_pairs=%u", p.link_pairs);
        } else if (!std::strcmp(stage, "resect_refine")) {
            const ResectRefinePlan p = resect_refine_plan(c, n);
            std::printf(" fwords=%u sum_blocks=%u pair_blocks=%u", p.fwords, p.sum_blocks, p.pair_blocks);
        } else if (!std::strcmp(stage, "chain")) {
            const ChainPlan p = chain_plan(c, pc, n);
            std::printf(" rec_blocks=%u fwords=%u link_pairs=%u", p.rec_blocks, p.fwords, p.link_pairs);
        } else if (!std::strcmp(stage, "tracks")) {
            const TracksPlan p = tracks_plan(c, pc, n);
            std::printf(" rec_blocks=%u fwords=%u link_pairs=%u", p.rec_blocks, p.fwords, p.link_pairs);
        } else {
            std::printf(" unknown\n");
            return 2;
        }
        std::printf("\n");
    }
    return got == EOF ? 0 : 2;
}
