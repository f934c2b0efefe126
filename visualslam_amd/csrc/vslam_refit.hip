// Least-squares refit of the fundamental matrix of the C ABI (include/vslam.h): argument checks and sizing
// (vslam_refit_plan.h), scratch and launches of kernels_refit.hip.h.  The number of launches depends on `rounds` alone: a
// pair that stops early costs its workgroups one read of its state.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_refit.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_refit_plan.h"

using namespace vslam;

extern "C" {

int vslam_refit_dev(vslam_ctx* c, const vslam_epipolar* models_in, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                    const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                    const vslam_refit_params* prm, const vslam_refit_out* out) {
    static_assert(sizeof(vslam_refit) == 16 && sizeof(vslam_epipolar) == 88 && sizeof(EpiXY) == 32, "record layouts");
    if (const char* why = refit_check_args(models_in, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("refit: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const RefitPlan pl = refit_plan(match_cap, n_pairs);
    EpiXY* xy = nullptr;
    RefitState* state = nullptr;
    double* partial = nullptr;
    ListOut<vslam_refit_out> lists{out, pl.fwords, pl.flag_words, n_pairs};
    WsPlan ws;
    ws.add(xy, pl.coords_elems);
    ws.add(state, pl.state_elems);
    ws.add(partial, pl.partial_elems);
    lists.add(ws);
    TRY(ws.commit(c));

    const dim3 stream_grid(pl.sum_blocks, n_pairs), pair_grid(pl.pair_blocks);
    const double d2 = prm->max_dist2;
    TRY(enqueue_epi_coords(c, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, xy));
    LAUNCH(c, "k_refit_init", k_refit_init, pair_grid, dim3(REFIT_PAIR_WG), models_in, n_pairs, state);
    for (unsigned int r = 0; r <= prm->rounds; ++r) {
        LAUNCH(c, "k_refit_count", k_refit_count, stream_grid, dim3(REFIT_WG), xy, match_counts, match_cap, state, d2, partial, pl.sum_blocks);
        LAUNCH(c, "k_refit_begin", k_refit_begin, pair_grid, dim3(REFIT_PAIR_WG), partial, pl.sum_blocks, match_counts, match_cap, n_pairs, r,
               prm->rounds, state, out->models, out->info);
        if (r == prm->rounds) break;
        LAUNCH(c, "k_refit_dist", k_refit_dist, stream_grid, dim3(REFIT_WG), xy, match_counts, match_cap, state, d2, partial, pl.sum_blocks);
        LAUNCH(c, "k_refit_scale", k_refit_scale, pair_grid, dim3(REFIT_PAIR_WG), partial, pl.sum_blocks, match_counts, match_cap, n_pairs, state);
        LAUNCH(c, "k_refit_moments", k_refit_moments, stream_grid, dim3(REFIT_WG), xy, match_counts, match_cap, state, d2, partial, pl.sum_blocks);
        LAUNCH(c, "k_refit_solve", k_refit_solve, pair_grid, dim3(REFIT_PAIR_WG), partial, pl.sum_blocks, match_counts, match_cap, n_pairs, state);
    }
    if (lists.wanted()) TRY(enqueue_epi_flags(c, xy, match_counts, match_cap, out->models, d2, n_pairs, lists.flags()));
    return lists.list(c, matches, match_counts, match_cap);
}

int vslam_refit_host(vslam_ctx* c, const vslam_epipolar* model_in, const vslam_match* matches, size_t n_matches, const vslam_point* query_points,
                     size_t n_query, const vslam_point* train_points, size_t n_train, const vslam_refit_params* prm, vslam_epipolar* model,
                     vslam_refit* info, uint64_t* inlier_bits, vslam_match* inliers, size_t inlier_cap, size_t* n_inliers) {
    ARGCHK(c, prm && model_in && model, "refit_host: null argument");
    ARGCHK(c, prm->rounds >= 1 && prm->rounds <= 8, "refit_host: 1 .. 8 rounds");
    ARGCHK(c, std::isfinite(prm->max_dist2) && prm->max_dist2 > 0.0, "refit_host: max_dist2 must be finite and positive");
    HostPair in{matches, query_points, train_points, n_matches, n_query, n_train};
    TRY(in.check(c, "refit_host", inlier_cap, !inliers || (n_inliers && inlier_cap > 0) ? nullptr : "inliers needs n_inliers and an inlier_cap"));
    TRY(usable_ctx(c));

    DevBufs dev;
    vslam_epipolar* d_model = nullptr;
    TRY(dev.put(c, d_model, model_in, 1));
    TRY(in.upload(c, dev));
    vslam_refit_out out{};
    out.struct_size = sizeof(out);
    out.models = d_model;  // in place: the ABI allows the very pointer
    out.models_bytes = sizeof(vslam_epipolar);
    if (info) {
        TRY(dev.get(c, out.info, 1));
        out.info_bytes = sizeof(vslam_refit);
    }
    TRY(in.lists(c, dev, out, inlier_bits, inliers, inlier_cap, n_inliers));
    TRY(vslam_refit_dev(c, d_model, in.d_matches, in.d_cnt, in.mcap, in.d_q, in.qcap, in.d_t, in.tcap, 1, prm, &out));
    HIPCHK(c, hipMemcpyAsync(model, out.models, sizeof(vslam_epipolar), hipMemcpyDeviceToHost, c->stream));
    if (info) HIPCHK(c, hipMemcpyAsync(info, out.info, sizeof(vslam_refit), hipMemcpyDeviceToHost, c->stream));
    return in.download(c, out);
}

}  // extern "C"
