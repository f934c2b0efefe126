// Homography and the degeneracy verdict of the C ABI (include/vslam.h): argument checks and sizing
// (vslam_homography_plan.h), scratch and launches of kernels_homography.hip.h.  The coordinate scratch and the inlier list
// are the two-view geometry's (enqueue_epi_coords, enqueue_inlier_list).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_homography.hip.h"
#include "vslam_ctx.h"
#include "vslam_homography_plan.h"
#include "vslam_launch.h"

using namespace vslam;

int vslam::enqueue_hom_flags(vslam_ctx* c, const EpiXY* xy, const unsigned int* match_counts, unsigned int match_cap, const vslam_homography* models,
                             double max_dist2, int n_pairs, unsigned long long* flags) {
    const TwoViewPlan pl = twoview_plan(match_cap, n_pairs);
    LAUNCH(c, "k_hom_flags", k_hom_flags, dim3(pl.rec_blocks, n_pairs), dim3(TWOVIEW_REC_WG), xy, match_counts, match_cap, models, max_dist2, flags,
           pl.fwords);
    return VSLAM_OK;
}

int vslam::enqueue_hom_verdict(vslam_ctx* c, const vslam_epipolar* epi, int n_pairs, unsigned int num, unsigned int den, unsigned int min_inliers,
                               vslam_homography* models, vslam_epipolar* gated) {
    LAUNCH(c, "k_hom_verdict", k_hom_verdict, dim3(hom_pair_blocks(n_pairs)), dim3(HOM_PAIR_WG), epi, n_pairs, num,
           den, min_inliers, models, gated);
    return VSLAM_OK;
}

extern "C" {

int vslam_homography_dev(vslam_ctx* c, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                         const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                         const vslam_epipolar* epipolar_models, const vslam_homography_params* prm, const vslam_homography_out* out) {
    static_assert(sizeof(vslam_homography_hyp) == 152 && sizeof(vslam_homography) == 168 && sizeof(vslam_epipolar) == 88 && sizeof(EpiXY) == 32,
                  "record layouts");
    if (const char* why = homography_check_args(matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs,
                                                epipolar_models, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("homography: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const unsigned int H = prm->n_hypotheses;
    const HomographyPlan pl = homography_plan(match_cap, n_pairs, H);
    EpiXY* xy = nullptr;
    vslam_homography_hyp* hyp_ws = nullptr;
    ListOut<vslam_homography_out> lists{out, pl.fwords, pl.flag_words, n_pairs};
    WsPlan ws;
    ws.add(xy, pl.coords_elems);
    if (!out->hypotheses) ws.add(hyp_ws, pl.hyp_elems);
    lists.add(ws);
    TRY(ws.commit(c));
    vslam_homography_hyp* hyp = out->hypotheses ? out->hypotheses : hyp_ws;

    TRY(enqueue_epi_coords(c, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, xy));
    LAUNCH(c, "k_hom_models", k_hom_models, dim3(pl.model_blocks, n_pairs), dim3(HOM_MODEL_WG), xy, match_counts, match_cap, H, prm->seed, hyp);
    LAUNCH(c, "k_hom_score", k_hom_score, dim3(pl.score_blocks, pl.nsplit, n_pairs), dim3(EPI_SCORE_WG), xy, match_counts, match_cap, H,
           prm->max_dist2, hyp);
    LAUNCH(c, "k_hom_select", k_hom_select, dim3(n_pairs), dim3(256), hyp, match_counts, match_cap, H, out->models);
    if (epipolar_models)
        TRY(enqueue_hom_verdict(c, epipolar_models, n_pairs, prm->degenerate_num, prm->degenerate_den, prm->min_inliers, out->models, out->gated_models));
    if (lists.wanted()) TRY(enqueue_hom_flags(c, xy, match_counts, match_cap, out->models, prm->max_dist2, n_pairs, lists.flags()));
    return lists.list(c, matches, match_counts, match_cap);
}

int vslam_homography_host(vslam_ctx* c, const vslam_match* matches, size_t n_matches, const vslam_point* query_points, size_t n_query,
                          const vslam_point* train_points, size_t n_train, const vslam_epipolar* epipolar_model,
                          const vslam_homography_params* prm, vslam_homography* model, uint64_t* inlier_bits, vslam_match* inliers,
                          size_t inlier_cap, size_t* n_inliers, vslam_homography_hyp* hypotheses, vslam_epipolar* gated_model) {
    ARGCHK(c, prm && model, "homography_host: null argument");
    ARGCHK(c, prm->n_hypotheses >= 1 && prm->n_hypotheses <= 65535, "homography_host: 1 .. 65535 hypotheses");
    ARGCHK(c, std::isfinite(prm->max_dist2) && prm->max_dist2 > 0.0, "homography_host: max_dist2 must be finite and positive");
    ARGCHK(c, prm->degenerate_den > 0, "homography_host: degenerate_den must be positive");
    HostPair in{matches, query_points, train_points, n_matches, n_query, n_train};
    TRY(in.check(c, "homography_host", inlier_cap,
                 inliers && !(n_inliers && inlier_cap > 0) ? "inliers needs n_inliers and an inlier_cap"
                 : gated_model && !epipolar_model          ? "gated_model needs epipolar_model"
                                                           : nullptr));
    TRY(usable_ctx(c));

    DevBufs dev;
    TRY(in.upload(c, dev));
    vslam_epipolar* d_epi = nullptr;
    if (epipolar_model) TRY(dev.put(c, d_epi, epipolar_model, 1));
    vslam_homography_out out{};
    out.struct_size = sizeof(out);
    TRY(dev.get(c, out.models, 1));
    out.models_bytes = sizeof(vslam_homography);
    TRY(in.lists(c, dev, out, inlier_bits, inliers, inlier_cap, n_inliers));
    if (hypotheses) {
        TRY(dev.get(c, out.hypotheses, prm->n_hypotheses));
        out.hypotheses_bytes = (size_t)prm->n_hypotheses * sizeof(vslam_homography_hyp);
    }
    if (gated_model) {
        out.gated_models = d_epi;  // in place: the ABI allows the very pointer
        out.gated_models_bytes = sizeof(vslam_epipolar);
    }
    TRY(vslam_homography_dev(c, in.d_matches, in.d_cnt, in.mcap, in.d_q, in.qcap, in.d_t, in.tcap, 1, d_epi, prm, &out));
    HIPCHK(c, hipMemcpyAsync(model, out.models, sizeof(vslam_homography), hipMemcpyDeviceToHost, c->stream));
    if (hypotheses) HIPCHK(c, hipMemcpyAsync(hypotheses, out.hypotheses, out.hypotheses_bytes, hipMemcpyDeviceToHost, c->stream));
    if (gated_model) HIPCHK(c, hipMemcpyAsync(gated_model, out.gated_models, sizeof(vslam_epipolar), hipMemcpyDeviceToHost, c->stream));
    return in.download(c, out);
}

}  // extern "C"
