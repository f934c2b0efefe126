// The refinement of the resected pose of the C ABI (include/vslam.h, "resection: Gauss-Newton refinement over all inliers"):
// argument checks and sizing (vslam_resect_refine_plan.h), scratch and launches of kernels_resect_refine.hip.h.  The number of
// launches depends on `rounds` alone: a pair that stops early costs its workgroups one read of its state.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_resect_refine.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_resect_refine_plan.h"

using namespace vslam;

extern "C" {

int vslam_resect_refine_dev(vslam_ctx* c, const vslam_resect* models_in, const vslam_resect_corr* corr, uint32_t obs_cap, int n_pairs,
                            const vslam_resect_refine_params* prm, const vslam_resect_refine_out* out) {
    static_assert(sizeof(vslam_resect_refine) == 32 && sizeof(vslam_resect) == 120 && sizeof(vslam_resect_corr) == 48, "record layouts");
    if (const char* why = resect_refine_check_args(models_in, corr, obs_cap, n_pairs, prm, out, true))
        return fail(c, VSLAM_ERR_INVALID, std::string("resect_refine: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const ResectRefinePlan pl = resect_refine_plan(obs_cap, n_pairs);
    RrState* state = nullptr;
    double* partial = nullptr;
    WsPlan ws;
    ws.add(state, pl.state_elems);
    ws.add(partial, pl.partial_elems);
    TRY(ws.commit(c));

    const dim3 stream_grid(pl.sum_blocks, n_pairs), pair_grid(pl.pair_blocks);
    const double fx = prm->K.fx, fy = prm->K.fy, d2 = prm->max_dist2;
    LAUNCH(c, "k_rr_init", k_rr_init, pair_grid, dim3(RR_PAIR_WG), models_in, n_pairs, state);
    for (unsigned int r = 0; r <= prm->rounds; ++r) {
        LAUNCH(c, "k_rr_pass", k_rr_pass, stream_grid, dim3(REFIT_WG), corr, obs_cap, state, fx, fy, d2, partial, pl.sum_blocks);
        LAUNCH(c, "k_rr_step", k_rr_step, pair_grid, dim3(RR_PAIR_WG), partial, pl.sum_blocks, obs_cap, n_pairs, r, prm->rounds, state, out->models,
               out->info);
    }
    if (out->inlier_bits) {
        unsigned long long* flags = reinterpret_cast<unsigned long long*>(out->inlier_bits);
        LAUNCH(c, "k_rr_flags_zero", k_rr_flags_zero, dim3((pl.fwords + REFIT_WG - 1) / REFIT_WG, n_pairs), dim3(REFIT_WG), out->models, obs_cap, flags,
               pl.fwords);
        LAUNCH(c, "k_rr_flags", k_rr_flags, dim3(pl.row_blocks, n_pairs), dim3(REFIT_WG), corr, obs_cap, out->models, fx, fy, d2, flags, pl.fwords);
    }
    return VSLAM_OK;
}

int vslam_resect_refine_host(vslam_ctx* c, const vslam_resect* models_in, const vslam_resect_corr* corr, uint32_t obs_cap, int n_pairs,
                             const vslam_resect_refine_params* prm, const vslam_resect_refine_out* out) {
    if (const char* why = resect_refine_check_args(models_in, corr, obs_cap, n_pairs, prm, out, false))
        return fail(c, VSLAM_ERR_INVALID, std::string("resect_refine_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs, rows = np * obs_cap, words = np * twoview_fwords(obs_cap);
    HostMirror m(c);
    const auto d_models = m.in(models_in, np);
    const auto d_corr = m.in(corr, rows);
    vslam_resect_refine_out d{};
    d.struct_size = sizeof(d);
    d.models = d_models;  // in place: the ABI allows the very pointer
    m.out(d.models, d.models_bytes, out->models, np, false);
    m.out(d.info, d.info_bytes, out->info, np, false);
    m.out(d.inlier_bits, d.inlier_bits_bytes, out->inlier_bits, words, true);
    TRY(m.status());
    TRY(vslam_resect_refine_dev(c, d_models, d_corr, obs_cap, n_pairs, prm, &d));
    return m.finish();
}

}  // extern "C"
