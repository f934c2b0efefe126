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

int vslam::enqueue_trk_next(vslam_ctx* c, const StructLists& L, const vslam_chain* chain, const unsigned int* prev, unsigned int* next) {
    const TracksPlan pl = tracks_plan(L.match_cap, L.point_cap, L.n_pairs);
    const TrkIn in{L.poses,     L.matches, L.match_counts, reinterpret_cast<const unsigned long long*>(L.front_bits), chain, nullptr, L.match_cap,
                   pl.fwords, L.point_cap, L.n_pairs};
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
        const StructLists L{poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs};
        TRY(enqueue_chain_link(c, L, prev));
        TRY(enqueue_trk_next(c, L, chain, prev, next));
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
    HostMirror m(c);
    const auto d_poses = m.in(poses, np);
    const auto d_matches = m.in(matches, recs);
    const auto d_counts = m.in(match_counts, np);
    const auto d_bits = m.in(front_bits, words);
    const auto d_chain = m.in(chain, np);
    const auto d_frames = m.in(frame_points, (np + 1) * point_cap);
    vslam_tracks_out d{};
    d.struct_size = sizeof(d);
    m.out(d.tracks, d.tracks_bytes, out->tracks, recs, true);
    m.out(d.refs, d.refs_bytes, out->refs, recs, true);
    m.out(d.good_bits, d.good_bits_bytes, out->good_bits, words, true);
    m.out(d.summary, d.summary_bytes, out->summary, np, false);
    TRY(m.status());
    TRY(vslam_tracks_dev(c, d_poses, d_matches, d_counts, match_cap, d_bits, point_cap, n_pairs, d_chain, d_frames, prm, &d));
    return m.finish();
}

}  // extern "C"
