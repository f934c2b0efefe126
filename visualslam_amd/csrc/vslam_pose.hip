// Relative pose and triangulation of the C ABI (include/vslam.h): argument checks and sizing (vslam_pose_plan.h), scratch and
// launches of kernels_pose.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_pose.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_pose_plan.h"

using namespace vslam;

extern "C" {

int vslam_pose_dev(vslam_ctx* c, const vslam_epipolar* models, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                   const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                   const vslam_pose_params* prm, const vslam_pose_out* out) {
    static_assert(sizeof(vslam_pose_cand) == 104 && sizeof(vslam_pose) == 112 && sizeof(EpiXY) == 32, "record layouts");
    if (const char* why = pose_check_args(models, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("pose: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const PosePlan pl = pose_plan(match_cap, n_pairs);
    EpiXY* xy = nullptr;
    vslam_pose_cand* cand_ws = nullptr;
    WsPlan ws;
    ws.add(xy, pl.coords_elems);
    if (!out->candidates) ws.add(cand_ws, pl.cand_elems);
    TRY(ws.commit(c));
    vslam_pose_cand* cand = out->candidates ? out->candidates : cand_ws;

    TRY(enqueue_epi_coords(c, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, xy));
    LAUNCH(c, "k_pose_candidates", k_pose_candidates, dim3(pl.pair_blocks), dim3(POSE_PAIR_WG), models, *prm, n_pairs, cand);
    LAUNCH(c, "k_pose_vote", k_pose_vote, dim3(pl.rec_blocks, n_pairs), dim3(POSE_REC_WG), xy, match_counts, match_cap, *prm, cand);
    LAUNCH(c, "k_pose_select", k_pose_select, dim3(pl.pair_blocks), dim3(POSE_PAIR_WG), cand, match_counts, match_cap, n_pairs, out->poses);
    if (out->points || out->front_bits)
        LAUNCH(c, "k_pose_points", k_pose_points, dim3(pl.rec_blocks, n_pairs), dim3(POSE_REC_WG), xy, match_counts, match_cap, out->poses, *prm,
               out->points, reinterpret_cast<unsigned long long*>(out->front_bits), pl.fwords);
    return VSLAM_OK;
}

int vslam_pose_host(vslam_ctx* c, const vslam_epipolar* model, const vslam_match* matches, size_t n_matches, const vslam_point* query_points,
                    size_t n_query, const vslam_point* train_points, size_t n_train, const vslam_pose_params* prm, vslam_pose* pose,
                    vslam_pose_cand* candidates, double* points, uint64_t* front_bits) {
    ARGCHK(c, prm && model && pose, "pose_host: null argument");
    if (const char* why = check_intrinsics(*prm)) return fail(c, VSLAM_ERR_INVALID, std::string("pose_host: ") + why);
    HostPair in{matches, query_points, train_points, n_matches, n_query, n_train};
    TRY(in.check(c, "pose_host"));
    TRY(usable_ctx(c));

    DevBufs dev;
    vslam_epipolar* d_model = nullptr;
    TRY(dev.put(c, d_model, model, 1));
    TRY(in.upload(c, dev));
    vslam_pose_out out{};
    out.struct_size = sizeof(out);
    TRY(dev.get(c, out.poses, 1));
    out.poses_bytes = sizeof(vslam_pose);
    if (candidates) {
        TRY(dev.get(c, out.candidates, 4));
        out.candidates_bytes = 4 * sizeof(vslam_pose_cand);
    }
    if (points) {
        TRY(dev.get(c, out.points, (size_t)in.mcap * 3));
        out.points_bytes = (size_t)in.mcap * 3 * sizeof(double);
    }
    if (front_bits) {
        TRY(dev.get(c, out.front_bits, in.fwords));
        out.front_bits_bytes = in.fwords * sizeof(uint64_t);
    }
    TRY(vslam_pose_dev(c, d_model, in.d_matches, in.d_cnt, in.mcap, in.d_q, in.qcap, in.d_t, in.tcap, 1, prm, &out));
    HIPCHK(c, hipMemcpyAsync(pose, out.poses, sizeof(vslam_pose), hipMemcpyDeviceToHost, c->stream));
    if (candidates) HIPCHK(c, hipMemcpyAsync(candidates, out.candidates, 4 * sizeof(vslam_pose_cand), hipMemcpyDeviceToHost, c->stream));
    if (front_bits && in.used_words) HIPCHK(c, hipMemcpyAsync(front_bits, out.front_bits, in.used_words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the point rows of a pair without a winner are not written: the caller's stay as they are
    if (points && n_matches && pose->best >= 0) HIPCHK(c, hipMemcpy(points, out.points, n_matches * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return VSLAM_OK;
}

}  // extern "C"
