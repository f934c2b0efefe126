// The tracks step of the C ABI (include/vslam.h, "tracks"): argument checks and sizing (vslam_tracks_plan.h), scratch and
// launches of kernels_tracks.hip.h.  The link table is the trajectory's (enqueue_chain_link); the continuation table is filled
// by enqueue_trk_next, which vslam_bundle_dev calls too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_tracks.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_tracks_plan.h"

using namespace vslam;

int vslam::enqueue_trk_next(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const unsigned int* match_counts, unsigned int match_cap,
                            const uint64_t* front_bits, unsigned int point_cap, int n_pairs, const vslam_chain* chain, const unsigned int* prev,
                            unsigned int* next) {
    const TracksPlan pl = tracks_plan(match_cap, point_cap, n_pairs);
    const TrkIn in{poses, matches, match_counts, reinterpret_cast<const unsigned long long*>(front_bits), chain, nullptr, match_cap, pl.fwords, point_cap, n_pairs};
    HIPCHK(c, hipMemsetAsync(next, 0xff, pl.next_elems * sizeof(unsigned int), c->stream));
    LAUNCH(c, "k_trk_next", k_trk_next, dim3(pl.rec_blocks, pl.link_pairs), dim3(TRK_REC_WG), in, prev, next);
    return VSLAM_OK;
}

extern "C" {

int vslam_tracks_dev(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                     const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain, const vslam_point* frame_points,
                     const vslam_tracks_params* prm, const vslam_tracks_out* out) {
    static_assert(sizeof(vslam_track) == 48 && sizeof(vslam_track_ref) == 8 && sizeof(vslam_track_summary) == 16 && sizeof(vslam_tracks_params) == 48,
                  "record layouts");
    if (const char* why = tracks_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, frame_points, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("tracks: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const TracksPlan pl = tracks_plan(match_cap, point_cap, n_pairs);
    unsigned int *prev = nullptr, *next = nullptr;
    WsPlan ws;
    ws.add(prev, pl.prev_elems);
    ws.add(next, pl.next_elems);
    TRY(ws.commit(c));

    const TrkIn in{poses, matches, match_counts, reinterpret_cast<const unsigned long long*>(front_bits), chain, frame_points, match_cap, pl.fwords, point_cap,
                   n_pairs};
    const dim3 records(pl.rec_blocks, n_pairs);
    if (out->summary) HIPCHK(c, hipMemsetAsync(out->summary, 0, (size_t)n_pairs * sizeof(vslam_track_summary), c->stream));
    if (pl.link_pairs) {
        TRY(enqueue_chain_link(c, poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, prev));
        TRY(enqueue_trk_next(c, poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, prev, next));
    }
    LAUNCH(c, "k_trk_walk", k_trk_walk, records, dim3(TRK_REC_WG), in, *prm, prev, next, out->tracks, out->refs, out->summary);
    LAUNCH(c, "k_trk_rows", k_trk_rows, records, dim3(TRK_REC_WG), in, prev, next, out->tracks, out->refs,
           reinterpret_cast<unsigned long long*>(out->good_bits));
    return VSLAM_OK;
}

int vslam_tracks_host(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                      const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain, const vslam_point* frame_points,
                      const vslam_tracks_params* prm, const vslam_tracks_out* out) {
    if (const char* why = tracks_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, frame_points, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("tracks_host: ") + why);
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
    TRY(dev.put(c, d_poses, poses, np));
    TRY(dev.put(c, d_matches, matches, recs));
    TRY(dev.put(c, d_counts, match_counts, np));
    TRY(dev.put(c, d_bits, front_bits, words));
    TRY(dev.put(c, d_chain, chain, np));
    TRY(dev.put(c, d_frames, frame_points, (np + 1) * point_cap));
    // the outputs go up first: the rows the call leaves untouched come back as the caller had them
    vslam_tracks_out d{};
    d.struct_size = sizeof(d);
    TRY(dev.put(c, d.tracks, static_cast<const vslam_track*>(out->tracks), recs));
    d.tracks_bytes = recs * sizeof(vslam_track);
    if (out->refs) {
        TRY(dev.put(c, d.refs, static_cast<const vslam_track_ref*>(out->refs), recs));
        d.refs_bytes = recs * sizeof(vslam_track_ref);
    }
    if (out->good_bits) {
        TRY(dev.put(c, d.good_bits, static_cast<const uint64_t*>(out->good_bits), words));
        d.good_bits_bytes = words * sizeof(uint64_t);
    }
    if (out->summary) {
        TRY(dev.get(c, d.summary, np));
        d.summary_bytes = np * sizeof(vslam_track_summary);
    }
    TRY(vslam_tracks_dev(c, d_poses, d_matches, d_counts, match_cap, d_bits, point_cap, n_pairs, d_chain, d_frames, prm, &d));
    HIPCHK(c, hipMemcpyAsync(out->tracks, d.tracks, recs * sizeof(vslam_track), hipMemcpyDeviceToHost, c->stream));
    if (out->refs) HIPCHK(c, hipMemcpyAsync(out->refs, d.refs, recs * sizeof(vslam_track_ref), hipMemcpyDeviceToHost, c->stream));
    if (out->good_bits) HIPCHK(c, hipMemcpyAsync(out->good_bits, d.good_bits, words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (out->summary) HIPCHK(c, hipMemcpyAsync(out->summary, d.summary, np * sizeof(vslam_track_summary), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

}  // extern "C"
