// Two-view geometry of the C ABI (include/vslam.h): argument checks and sizing (vslam_epipolar_plan.h), scratch and launches
// of kernels_epipolar.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_epipolar.hip.h"
#include "vslam_ctx.h"
#include "vslam_epipolar_plan.h"
#include "vslam_launch.h"

using namespace vslam;

int vslam::enqueue_epi_coords(vslam_ctx* c, const vslam_match* matches, const unsigned int* match_counts, unsigned int match_cap,
                              const vslam_point* query_points, unsigned int query_cap, const vslam_point* train_points, unsigned int train_cap,
                              int n_pairs, EpiXY* xy) {
    LAUNCH(c, "k_epi_coords", k_epi_coords, dim3(twoview_plan(match_cap, n_pairs).rec_blocks, n_pairs), dim3(TWOVIEW_REC_WG), matches, match_counts,
           match_cap, query_points, query_cap, train_points, train_cap, xy);
    return VSLAM_OK;
}

int vslam::enqueue_epi_flags(vslam_ctx* c, const EpiXY* xy, const unsigned int* match_counts, unsigned int match_cap, const vslam_epipolar* models,
                             double max_dist2, int n_pairs, unsigned long long* flags) {
    const TwoViewPlan pl = twoview_plan(match_cap, n_pairs);
    LAUNCH(c, "k_epi_flags", k_epi_flags, dim3(pl.rec_blocks, n_pairs), dim3(TWOVIEW_REC_WG), xy, match_counts, match_cap, models, max_dist2, flags,
           pl.fwords);
    return VSLAM_OK;
}

extern "C" {

int vslam_epipolar_dev(vslam_ctx* c, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                       const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                       const vslam_epipolar_params* prm, const vslam_epipolar_out* out) {
    static_assert(sizeof(vslam_epipolar_hyp) == 80 && sizeof(vslam_epipolar) == 88 && sizeof(EpiXY) == 32, "record layouts");
    if (const char* why = epipolar_check_args(matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("epipolar: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const unsigned int H = prm->n_hypotheses;
    const EpipolarPlan pl = epipolar_plan(match_cap, n_pairs, H);
    EpiXY* xy = nullptr;
    vslam_epipolar_hyp* hyp_ws = nullptr;
    ListOut<vslam_epipolar_out> lists{out, pl.fwords, pl.flag_words, n_pairs};
    WsPlan ws;
    ws.add(xy, pl.coords_elems);
    if (!out->hypotheses) ws.add(hyp_ws, pl.hyp_elems);
    lists.add(ws);
    TRY(ws.commit(c));
    vslam_epipolar_hyp* hyp = out->hypotheses ? out->hypotheses : hyp_ws;

    TRY(enqueue_epi_coords(c, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, xy));
    LAUNCH(c, "k_epi_models", k_epi_models, dim3(pl.model_blocks, n_pairs), dim3(EPI_MODEL_WG), xy, match_counts, match_cap, H, prm->seed, hyp);
    LAUNCH(c, "k_epi_score", k_epi_score, dim3(pl.score_blocks, pl.nsplit, n_pairs), dim3(EPI_SCORE_WG), xy, match_counts, match_cap, H,
           prm->max_dist2, hyp);
    LAUNCH(c, "k_epi_select", k_epi_select, dim3(n_pairs), dim3(256), hyp, match_counts, match_cap, H, out->models);
    if (lists.wanted()) TRY(enqueue_epi_flags(c, xy, match_counts, match_cap, out->models, prm->max_dist2, n_pairs, lists.flags()));
    return lists.list(c, matches, match_counts, match_cap);
}

int vslam_epipolar_host(vslam_ctx* c, const vslam_match* matches, size_t n_matches, const vslam_point* query_points, size_t n_query,
                        const vslam_point* train_points, size_t n_train, const vslam_epipolar_params* prm, vslam_epipolar* model,
                        uint64_t* inlier_bits, vslam_match* inliers, size_t inlier_cap, size_t* n_inliers, vslam_epipolar_hyp* hypotheses) {
    ARGCHK(c, prm && model, "epipolar_host: null argument");
    ARGCHK(c, prm->n_hypotheses >= 1 && prm->n_hypotheses <= 65535, "epipolar_host: 1 .. 65535 hypotheses");
    ARGCHK(c, std::isfinite(prm->max_dist2) && prm->max_dist2 > 0.0, "epipolar_host: max_dist2 must be finite and positive");
    HostPair in{matches, query_points, train_points, n_matches, n_query, n_train};
    TRY(in.check(c, "epipolar_host", inlier_cap, !inliers || (n_inliers && inlier_cap > 0) ? nullptr : "inliers needs n_inliers and an inlier_cap"));
    TRY(usable_ctx(c));

    DevBufs dev;
    TRY(in.upload(c, dev));
    vslam_epipolar_out out{};
    out.struct_size = sizeof(out);
    TRY(dev.get(c, out.models, 1));
    out.models_bytes = sizeof(vslam_epipolar);
    TRY(in.lists(c, dev, out, inlier_bits, inliers, inlier_cap, n_inliers));
    if (hypotheses) {
        TRY(dev.get(c, out.hypotheses, prm->n_hypotheses));
        out.hypotheses_bytes = (size_t)prm->n_hypotheses * sizeof(vslam_epipolar_hyp);
    }
    TRY(vslam_epipolar_dev(c, in.d_matches, in.d_cnt, in.mcap, in.d_q, in.qcap, in.d_t, in.tcap, 1, prm, &out));
    HIPCHK(c, hipMemcpyAsync(model, out.models, sizeof(vslam_epipolar), hipMemcpyDeviceToHost, c->stream));
    if (hypotheses) HIPCHK(c, hipMemcpyAsync(hypotheses, out.hypotheses, out.hypotheses_bytes, hipMemcpyDeviceToHost, c->stream));
    return in.download(c, out);
}

}  // extern "C"
