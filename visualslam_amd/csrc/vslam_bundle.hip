// The bundle adjustment of the C ABI (include/vslam.h, "bundle adjustment"): argument checks and sizing (vslam_bundle_plan.h),
// scratch and launches of kernels_bundle.hip.h.  The tables are the trajectory's and the tracks stage's (enqueue_chain_link,
// enqueue_trk_next).  The number of launches depends on `sweeps` alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_bundle.hip.h"
#include "vslam_bundle_plan.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"

using namespace vslam;

extern "C" {

int vslam_bundle_dev(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                     const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain, const vslam_point* frame_points,
                     const vslam_track* tracks_in, const vslam_track_ref* refs, const vslam_bundle_cam* cams_in, const vslam_bundle_params* prm,
                     const vslam_bundle_out* out) {
    static_assert(sizeof(vslam_bundle_cam) == 160 && sizeof(vslam_bundle_point) == 40 && sizeof(vslam_bundle_params) == 48, "record layouts");
    if (const char* why = bundle_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, frame_points, tracks_in, refs,
                                            prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("bundle: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const BundlePlan pl = bundle_plan(match_cap, point_cap, n_pairs);
    unsigned int *prev = nullptr, *next = nullptr;
    BaCam* state = nullptr;
    double* partial = nullptr;
    WsPlan ws;
    ws.add(prev, pl.trk.prev_elems);
    ws.add(next, pl.trk.next_elems);
    ws.add(state, pl.state_elems);
    ws.add(partial, pl.partial_elems);
    TRY(ws.commit(c));

    const TrkIn in{poses,     matches,      match_counts, reinterpret_cast<const unsigned long long*>(front_bits), chain, frame_points, match_cap,
                   pl.trk.fwords, point_cap, n_pairs};
    const dim3 records(pl.trk.rec_blocks, n_pairs), rows(pl.sum_blocks, n_pairs), pairs(pl.pair_blocks);
    if (pl.trk.link_pairs) {
        TRY(enqueue_chain_link(c, poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, prev));
        TRY(enqueue_trk_next(c, poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, prev, next));
    }
    LAUNCH(c, "k_ba_init", k_ba_init, records, dim3(TRK_REC_WG), in, *prm, prev, next, tracks_in, cams_in, out->tracks, out->point_info, state);
    for (unsigned int sweep = 0; sweep < prm->sweeps; ++sweep) {
        LAUNCH(c, "k_ba_points", k_ba_points, records, dim3(TRK_REC_WG), in, *prm, prev, next, state, out->tracks, out->point_info, sweep);
        for (int which : {BA_CUR, BA_CAND}) {
            LAUNCH(c, "k_ba_cam_pass", k_ba_cam_pass, rows, dim3(REFIT_WG), in, *prm, refs, out->tracks, state, which, partial, pl.sum_blocks);
            LAUNCH(c, "k_ba_cam_step", k_ba_cam_step, pairs, dim3(RR_PAIR_WG), in, partial, pl.sum_blocks, which, sweep, prm->sweeps, state, out->cams);
        }
    }
    LAUNCH(c, "k_ba_cam_pass", k_ba_cam_pass, rows, dim3(REFIT_WG), in, *prm, refs, out->tracks, state, BA_FINAL, partial, pl.sum_blocks);
    LAUNCH(c, "k_ba_cam_step", k_ba_cam_step, pairs, dim3(RR_PAIR_WG), in, partial, pl.sum_blocks, BA_FINAL, prm->sweeps, prm->sweeps, state, out->cams);
    if (out->member_bits)
        LAUNCH(c, "k_ba_member_bits", k_ba_member_bits, records, dim3(TRK_REC_WG), in, *prm, refs, out->tracks, state,
               reinterpret_cast<unsigned long long*>(out->member_bits));
    LAUNCH(c, "k_ba_points_final", k_ba_points_final, records, dim3(TRK_REC_WG), in, *prm, prev, next, state, out->tracks, out->point_info);
    return VSLAM_OK;
}

int vslam_bundle_host(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                      const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain, const vslam_point* frame_points,
                      const vslam_track* tracks_in, const vslam_track_ref* refs, const vslam_bundle_cam* cams_in, const vslam_bundle_params* prm,
                      const vslam_bundle_out* out) {
    if (const char* why = bundle_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, frame_points, tracks_in, refs,
                                            prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("bundle_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs, recs = np * match_cap, words = np * twoview_fwords(match_cap);
    DevBufs dev;
    vslam_pose* d_poses = nullptr;
    vslam_match* d_matches = nullptr;
    uint32_t* d_counts = nullptr;
    uint64_t* d_bits = nullptr;
    vslam_chain* d_chain = nullptr;
    vslam_point* d_frames = nullptr;
    vslam_track* d_tracks_in = nullptr;
    vslam_track_ref* d_refs = nullptr;
    vslam_bundle_cam* d_cams_in = nullptr;
    TRY(dev.put(c, d_poses, poses, np));
    TRY(dev.put(c, d_matches, matches, recs));
    TRY(dev.put(c, d_counts, match_counts, np));
    TRY(dev.put(c, d_bits, front_bits, words));
    TRY(dev.put(c, d_chain, chain, np));
    TRY(dev.put(c, d_frames, frame_points, (np + 1) * point_cap));
    TRY(dev.put(c, d_tracks_in, tracks_in, recs));
    TRY(dev.put(c, d_refs, refs, recs));
    if (cams_in) TRY(dev.put(c, d_cams_in, cams_in, np));
    // the outputs go up first: the rows and words the call leaves untouched come back as the caller had them
    vslam_bundle_out d{};
    d.struct_size = sizeof(d);
    TRY(dev.put(c, d.tracks, static_cast<const vslam_track*>(out->tracks), recs));
    d.tracks_bytes = recs * sizeof(vslam_track);
    TRY(dev.get(c, d.cams, np));
    d.cams_bytes = np * sizeof(vslam_bundle_cam);
    if (out->point_info) {
        TRY(dev.put(c, d.point_info, static_cast<const vslam_bundle_point*>(out->point_info), recs));
        d.point_info_bytes = recs * sizeof(vslam_bundle_point);
    }
    if (out->member_bits) {
        TRY(dev.put(c, d.member_bits, static_cast<const uint64_t*>(out->member_bits), 2 * words));
        d.member_bits_bytes = 2 * words * sizeof(uint64_t);
    }
    TRY(vslam_bundle_dev(c, d_poses, d_matches, d_counts, match_cap, d_bits, point_cap, n_pairs, d_chain, d_frames, d_tracks_in, d_refs, d_cams_in, prm, &d));
    HIPCHK(c, hipMemcpyAsync(out->tracks, d.tracks, recs * sizeof(vslam_track), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out->cams, d.cams, np * sizeof(vslam_bundle_cam), hipMemcpyDeviceToHost, c->stream));
    if (out->point_info) HIPCHK(c, hipMemcpyAsync(out->point_info, d.point_info, d.point_info_bytes, hipMemcpyDeviceToHost, c->stream));
    if (out->member_bits) HIPCHK(c, hipMemcpyAsync(out->member_bits, d.member_bits, d.member_bits_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

}  // extern "C"
