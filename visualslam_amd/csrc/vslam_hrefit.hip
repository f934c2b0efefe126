// Least-squares refit of the homography of the C ABI (include/vslam.h): argument checks and sizing (vslam_hrefit_plan.h),
// scratch and launches of kernels_hrefit.hip.h.  The number of launches depends on `rounds` alone: a pair that stops early
// costs its workgroups one read of its state.  The verdict, the ballot words and the list are the homography stage's
// (enqueue_hom_verdict, enqueue_hom_flags, enqueue_inlier_list).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_hrefit.hip.h"
#include "vslam_ctx.h"
#include "vslam_hrefit_plan.h"
#include "vslam_launch.h"

using namespace vslam;

extern "C" {

int vslam_hrefit_dev(vslam_ctx* c, const vslam_homography* models_in, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                     const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                     const vslam_epipolar* epipolar_models, const vslam_hrefit_params* prm, const vslam_hrefit_out* out) {
    static_assert(sizeof(vslam_hrefit) == 16 && sizeof(vslam_homography) == 168 && sizeof(vslam_epipolar) == 88 && sizeof(EpiXY) == 32 &&
                      sizeof(HRefitState) == 520,
                  "record layouts");
    if (const char* why = hrefit_check_args(models_in, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs,
                                            epipolar_models, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("hrefit: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const HRefitPlan pl = hrefit_plan(match_cap, n_pairs);
    EpiXY* xy = nullptr;
    HRefitState* state = nullptr;
    double* partial = nullptr;
    ListOut<vslam_hrefit_out> lists{out, pl.fwords, pl.flag_words, n_pairs};
    WsPlan ws;
    ws.add(xy, pl.coords_elems);
    ws.add(state, pl.state_elems);
    ws.add(partial, pl.partial_elems);
    lists.add(ws);
    TRY(ws.commit(c));

    const dim3 stream_grid(pl.sum_blocks, n_pairs), pair_grid(pl.pair_blocks);
    const double d2 = prm->max_dist2;
    TRY(enqueue_epi_coords(c, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, xy));
    LAUNCH(c, "k_hrefit_init", k_hrefit_init, pair_grid, dim3(REFIT_PAIR_WG), models_in, n_pairs, state);
    for (unsigned int r = 0; r <= prm->rounds; ++r) {
        LAUNCH(c, "k_hrefit_count", k_hrefit_count, stream_grid, dim3(REFIT_WG), xy, match_counts, match_cap, state, d2, partial, pl.sum_blocks);
        LAUNCH(c, "k_hrefit_begin", k_hrefit_begin, pair_grid, dim3(REFIT_PAIR_WG), partial, pl.sum_blocks, match_counts, match_cap, n_pairs, r,
               prm->rounds, state, out->models, out->info);
        if (r == prm->rounds) break;
        LAUNCH(c, "k_hrefit_dist", k_hrefit_dist, stream_grid, dim3(REFIT_WG), xy, match_counts, match_cap, state, d2, partial, pl.sum_blocks);
        LAUNCH(c, "k_hrefit_scale", k_hrefit_scale, pair_grid, dim3(REFIT_PAIR_WG), partial, pl.sum_blocks, match_counts, match_cap, n_pairs, state);
        LAUNCH(c, "k_hrefit_moments", k_hrefit_moments, stream_grid, dim3(REFIT_WG), xy, match_counts, match_cap, state, d2, partial, pl.sum_blocks);
        LAUNCH(c, "k_hrefit_solve", k_hrefit_solve, pair_grid, dim3(REFIT_PAIR_WG), partial, pl.sum_blocks, match_counts, match_cap, n_pairs, state);
    }
    if (epipolar_models)
        TRY(enqueue_hom_verdict(c, epipolar_models, n_pairs, prm->degenerate_num, prm->degenerate_den, prm->min_inliers, out->models, out->gated_models));
    if (lists.wanted()) TRY(enqueue_hom_flags(c, xy, match_counts, match_cap, out->models, d2, n_pairs, lists.flags()));
    return lists.list(c, matches, match_counts, match_cap);
}

int vslam_hrefit_host(vslam_ctx* c, const vslam_homography* model_in, const vslam_match* matches, size_t n_matches, const vslam_point* query_points,
                      size_t n_query, const vslam_point* train_points, size_t n_train, const vslam_epipolar* epipolar_model,
                      const vslam_hrefit_params* prm, vslam_homography* model, vslam_hrefit* info, uint64_t* inlier_bits, vslam_match* inliers,
                      size_t inlier_cap, size_t* n_inliers, vslam_epipolar* gated_model) {
    ARGCHK(c, prm && model_in && model, "hrefit_host: null argument");
    ARGCHK(c, prm->rounds >= 1 && prm->rounds <= 8, "hrefit_host: 1 .. 8 rounds");
    ARGCHK(c, std::isfinite(prm->max_dist2) && prm->max_dist2 > 0.0, "hrefit_host: max_dist2 must be finite and positive");
    ARGCHK(c, !epipolar_model || prm->degenerate_den > 0, "hrefit_host: degenerate_den must be positive");
    HostPair in{matches, query_points, train_points, n_matches, n_query, n_train};
    TRY(in.check(c, "hrefit_host", inlier_cap,
                 inliers && !(n_inliers && inlier_cap > 0) ? "inliers needs n_inliers and an inlier_cap"
                 : gated_model && !epipolar_model          ? "gated_model needs epipolar_model"
                                                           : nullptr));
    TRY(usable_ctx(c));

    DevBufs dev;
    vslam_homography* d_model = nullptr;
    vslam_epipolar* d_epi = nullptr;
    TRY(dev.put(c, d_model, model_in, 1));
    if (epipolar_model) TRY(dev.put(c, d_epi, epipolar_model, 1));
    TRY(in.upload(c, dev));
    vslam_hrefit_out out{};
    out.struct_size = sizeof(out);
    out.models = d_model;  // in place: the ABI allows the very pointer
    out.models_bytes = sizeof(vslam_homography);
    if (info) {
        TRY(dev.get(c, out.info, 1));
        out.info_bytes = sizeof(vslam_hrefit);
    }
    TRY(in.lists(c, dev, out, inlier_bits, inliers, inlier_cap, n_inliers));
    if (gated_model) {
        out.gated_models = d_epi;  // in place: the ABI allows the very pointer
        out.gated_models_bytes = sizeof(vslam_epipolar);
    }
    TRY(vslam_hrefit_dev(c, d_model, in.d_matches, in.d_cnt, in.mcap, in.d_q, in.qcap, in.d_t, in.tcap, 1, d_epi, prm, &out));
    HIPCHK(c, hipMemcpyAsync(model, out.models, sizeof(vslam_homography), hipMemcpyDeviceToHost, c->stream));
    if (info) HIPCHK(c, hipMemcpyAsync(info, out.info, sizeof(vslam_hrefit), hipMemcpyDeviceToHost, c->stream));
    if (gated_model) HIPCHK(c, hipMemcpyAsync(gated_model, out.gated_models, sizeof(vslam_epipolar), hipMemcpyDeviceToHost, c->stream));
    return in.download(c, out);
}

}  // extern "C"
