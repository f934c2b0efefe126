// C ABI (include/vslam.h) over the hand-written gfx950 kernels.  Host code here only
// validates arguments, sizes the workspace and enqueues kernels on the context's stream;
// there is no CPU compute path: if HIP is unavailable every compute entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <string>
#include <set>
#include <memory>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_generic.hip.h"
#include "kernels_pyramid.hip.h"
#include "kernels_strip.hip.h"
#include "kernels_hdiff.hip.h"
#include "kernels_aux.hip.h"
#include "kernels_harris_strip.hip.h"
#include "kernels_orient.hip.h"
#include "kernels_orient_batch.hip.h"
#include "kernels_orient_pk.hip.h"
#include "kernels_compact.hip.h"
#include "kernels_sift.hip.h"
#include "kernels_extrema_dense.hip.h"
#include "vslam_batch_plan.h"
#include "vslam_internal.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_mx.h"
#include "vslam_octave_launch.h"

using namespace vslam;


struct vslam_pyramid {
    vslam_ctx* ctx = nullptr;
    vslam_params params{};
    vslam_batch_layout layout{};
    vslam_pyramid_info info{};
    uint8_t* d_block = nullptr;  // one pyramid frame block (layout.pyramid_frame_bytes)
    uint8_t* d_bases = nullptr;  // octave bases, octave o at base_off[o]
    size_t block_cap = 0, bases_cap = 0;
    size_t base_off[VSLAM_MAX_OCTAVES] = {};
};


static const char* const kKernelNames =
    "k_resize_linear2x\nk_blur_h_generic\nk_blur_v_generic\n"
    "k_dog5\nk_resize_nearest_half\nk_extrema\nk_pyr_octave\nk_pyr_octave_mx\n"
    "k_gauss_v_strip\nk_gauss_h_strip\nk_gauss_h_diff\nk_resize_linear2x_slide\nk_resize_nearest_half_v4\nk_extrema_w3\nk_extrema_dense\nk_localize_points\nk_orient_keypoints\nk_edge_response_windows\nk_level_gradients\nk_pack_rows\nk_edge_flags\nk_survivor_ranges\nk_orient_survivors\n"
    "k_extrema_pack\nk_harris_strip\nk_flag_count\nk_chunk_scan\nk_flag_scatter\nk_level_gradients\nk_sift_descriptors\nk_pack_offsets\nk_pack_copy\nk_count_totals\n"
    "k_desc_norms\nk_match_nn2\nk_match_merge\n"
    "k_guided_rows\nk_match_guided\nk_match_guided_merge\n"
    "k_guided_hf_rows\nk_guided_hf_kinds\nk_match_guided_hf\n"
    "k_match_nn2_mutual\nk_match_mutual_merge\nk_match_rnn_write\n"
    "k_epi_coords\nk_epi_models\nk_epi_score\nk_epi_select\nk_epi_flags\n"
    "k_refit_init\nk_refit_count\nk_refit_begin\nk_refit_dist\nk_refit_scale\nk_refit_moments\nk_refit_solve\n"
    "k_hom_models\nk_hom_score\nk_hom_select\nk_hom_flags\nk_hom_verdict\n"
    "k_hrefit_init\nk_hrefit_count\nk_hrefit_begin\nk_hrefit_dist\nk_hrefit_scale\nk_hrefit_moments\nk_hrefit_solve\n"
    "k_pose_candidates\nk_pose_vote\nk_pose_select\nk_pose_points\n"
    "k_hpose_candidates\nk_hpose_vote\nk_hpose_select\nk_hpose_points\n"
    "k_chain_link\nk_chain_ratio\nk_chain_median\nk_chain_walk\nk_chain_map\n"
    "k_res_corr\nk_res_gather\nk_res_models\nk_res_score\nk_res_select\nk_res_flags\n"
    "k_rr_init\nk_rr_pass\nk_rr_step\nk_rr_flags_zero\nk_rr_flags\n"
    "k_trk_next\nk_trk_walk\nk_trk_rows\n"
    "k_ba_init\nk_ba_points\nk_ba_cam_pass\nk_ba_cam_step\nk_ba_member_bits\nk_ba_points_final\n"
    "k_vocab_gather\nk_words_nn\nk_words_merge\n"
    "k_place_df\nk_place_self\nk_place_score\nk_place_top\n"
    "k_kmeans_init\nk_kmeans_count\nk_kmeans_columns\nk_kmeans_scan\nk_kmeans_members\nk_kmeans_block_sums\nk_kmeans_update\n"
    "k_loop_pairs\nk_match_nn2_pairs\nk_match_merge_pairs\nk_pair_points\nk_loop_verdict\n"
    "k_frame_index\nk_frame_cams\nk_sim3_corr\nk_sim3_gather\nk_sim3_models\nk_sim3_score\nk_sim3_select\nk_sim3_flags";


// Runs `body` with the context's launch stream temporarily replaced (LAUNCH uses ctx->stream).
struct StreamSwap {
    vslam_ctx* c;
    hipStream_t saved;
    StreamSwap(vslam_ctx* ctx, hipStream_t s) : c(ctx), saved(ctx->stream) { c->stream = s; }
    ~StreamSwap() { c->stream = saved; }
};

// Raises a kernel's dynamic shared memory ceiling to the most any launch of it may ask for (kMaxDynLds, vslam_octave_launch.h).
static int raise_dyn_lds(vslam_ctx* c, const void* fn) {
    if (c->lds_raised.count(fn)) return VSLAM_OK;
    HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds));
    c->lds_raised.insert(fn);
    return VSLAM_OK;
}

static void* block_alloc(vslam_ctx* c, size_t bytes, size_t* cap) {
    int best = -1;
    for (int i = 0; i < (int)c->block_cache.size(); ++i) {
        const size_t sz = c->block_cache[i].first;
        if (sz >= bytes && sz <= 2 * bytes + (1 << 20) && (best < 0 || sz < c->block_cache[best].first)) best = i;
    }
    if (best >= 0) {
        void* p = c->block_cache[best].second;
        *cap = c->block_cache[best].first;
        c->block_cache.erase(c->block_cache.begin() + best);
        return p;
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        for (auto& b : c->block_cache) (void)hipFree(b.second);  // give the cache back and retry once
        c->block_cache.clear();
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    }
    *cap = bytes;
    return p;
}
static void block_release(vslam_ctx* c, void* p, size_t cap) {
    if (!p) return;
    if (c && c->block_cache.size() < 8 && cap <= ((size_t)1 << 30))
        c->block_cache.emplace_back(cap, p);
    else
        (void)hipFree(p);
}

int vslam::ws_reserve(vslam_ctx* c, size_t bytes) {
    if (bytes <= c->ws_cap) return VSLAM_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < vslam_ctx::kAux; ++i)
        if (c->aux[i]) HIPCHK(c, hipStreamSynchronize(c->aux[i]));
    if (c->ws) (void)hipFree(c->ws);
    c->ws = nullptr;
    c->ws_cap = 0;
    const size_t want = align_up(bytes + bytes / 8, 1 << 20);
    HIPCHK(c, hipMalloc((void**)&c->ws, want));
    c->ws_cap = want;
    return VSLAM_OK;
}

// One-time device tables (tap matrices) are allocated and copied with blocking calls: inside a stream capture that would
// invalidate the capture, so a call that still needs one says so instead (include/vslam.h: the warm-up call must run with
// the same parameters AND the same matrix-path setting as the captured one).
static bool stream_is_capturing(vslam_ctx* c) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess) (void)hipGetLastError();
    return cap != hipStreamCaptureStatusNone;
}
#define NO_TABLE_IN_CAPTURE(ctx, what)                                                                                                      \
    if (stream_is_capturing(ctx))                                                                                                           \
    return fail(ctx, VSLAM_ERR_UNSUPPORTED, std::string(what) + ": its tap tables are not on the device yet and cannot be put there during a stream capture - " \
                                                                "run one warm-up call with the same parameters and the same matrix-path setting first")

// The context's device tables (vslam_ctx::tables).  `v` of the key: the bits of sigma (Blur, Orient) or of sigma0 (the others);
// `i`: the kernel width (Blur, Orient) or the octave.
enum TableKind { kTableBlur, kTableStrip, kTableTile, kTableMx, kTableOrient };

// The device table (kind, v, i), made on first use: `fill(host)` fills a zeroed host copy of `bytes` bytes and returns a status.
// The copy is raw storage from operator new (aligned for any of the table structs, all trivially copyable aggregates of
// integers / floats); the fill functions write their struct into it member by member.
// `what` names the caller in the refusal of a call that would have to make the table inside a stream capture.
template <class T, class Fill>
static int get_table(vslam_ctx* c, TableKind kind, double v, int i, const char* what, size_t bytes, Fill fill, const T** out) {
    uint64_t vb;
    std::memcpy(&vb, &v, 8);
    const auto key = std::make_tuple((int)kind, vb, i);
    auto it = c->tables.find(key);
    if (it == c->tables.end()) {
        NO_TABLE_IN_CAPTURE(c, what);
        std::vector<char> host(bytes);
        TRY(fill(static_cast<void*>(host.data())));
        void* d = nullptr;
        HIPCHK(c, hipMalloc(&d, bytes));
        HIPCHK(c, hipMemcpy(d, host.data(), bytes, hipMemcpyHostToDevice));
        it = c->tables.emplace(key, d).first;
    }
    *out = static_cast<const T*>(it->second);
    return VSLAM_OK;
}

static inline void tap_pointers(const std::vector<uint16_t> taps[6], const uint16_t* tp[6]) {
    for (int l = 0; l < 6; ++l) tp[l] = taps[l].data();
}

// Device copy of the (zero-trimmed) quantised taps of one GaussianBlur; *n_eff = trimmed width.
static int get_taps(vslam_ctx* c, int n, double sigma, const uint16_t** out, int* n_eff) {
    std::vector<uint16_t> h;
    if (!gauss_taps_q8_trimmed(n, sigma, h)) return fail(c, VSLAM_ERR_INVALID, "invalid Gaussian kernel size");
    *n_eff = (int)h.size();
    return get_table(c, kTableBlur, sigma, n, "Gaussian blur", sizeof(uint16_t) * h.size(), [&](void* host) -> int {
        std::memcpy(host, h.data(), sizeof(uint16_t) * h.size());
        return VSLAM_OK;
    }, out);
}

static inline dim3 grid_rows(int cols, int rows, int frames = 1) { return dim3((cols + 255) / 256, rows, frames); }

// ---------------------------------------------------------------- enqueue helpers (device)

// ---- octave path selection -----------------------------------------------------------------
namespace {
enum class OctPath { Tile0, Tile1, Strip, Generic };

struct OctPlan {
    OctPath path = OctPath::Generic;
    int ks[6] = {};                 // OpenCV kernel widths (GaussianBlur's ksize)
    double sg[6] = {};
    int ke[6] = {};                 // zero-trimmed widths the fast kernels run with
    std::vector<uint16_t> taps[6];  // trimmed taps
    int nmax = 0;                   // widest of ke
    int sh = 0;                     // rows per horizontal strip workgroup (strip_plan_sh)
    int hdiff = 0;                  // octave of diff_taps.gen.h with these taps: the difference-form horizontal pass (k_gauss_h_diff)
    int ctaps = 0;                  // octave of diff_taps.gen.h with these taps: the octave kernel with its taps compiled in (PyrCfgConst)
    int mx = 0;                     // matrix-core configuration that runs these widths (mx_config_for), 0 = none; used on the opt-in path only
};
}  // namespace

static bool taps_fit_u8(const OctPlan& pl) {
    for (int l = 0; l < 6; ++l)
        for (uint16_t v : pl.taps[l])
            if (v > 255) return false;
    return true;
}

template <class CFG>
static bool matches_cfg(const int ks[6]) {
    for (int l = 0; l < 6; ++l)
        if (ks[l] != CFG::n(l)) return false;
    return true;
}

static OctPlan plan_octave(double sigma0, int o, int rows, int cols) {
    OctPlan pl;
    int& nmax = pl.nmax;
    for (int l = 0; l < 6; ++l) {
        pl.sg[l] = sigma_at(sigma0, o, l);
        pl.ks[l] = gauss_ksize_u8(pl.sg[l]);
        if (!gauss_taps_q8_trimmed(pl.ks[l], pl.sg[l], pl.taps[l])) return pl;
        pl.ke[l] = (int)pl.taps[l].size();
        nmax = std::max(nmax, pl.ke[l]);
    }
    if (!taps_fit_u8(pl)) return pl;
    if (matches_cfg<PyrCfgOct0>(pl.ke)) {
        pl.path = OctPath::Tile0;
    } else if (matches_cfg<PyrCfgOct1>(pl.ke)) {
        pl.path = OctPath::Tile1;
        pl.ctaps = hd_octave_matches<1>(pl.taps) ? 1 : 0;  // the default pyramid's octave 1
    } else if (nmax <= STRIP_MAXN) {
        pl.sh = strip_plan_sh(rows, cols, nmax);
        if (pl.sh) pl.path = OctPath::Strip;
        // the default pyramid's octaves 2-3 (and any octave with the same taps): horizontal pass in difference form
        if (pl.path == OctPath::Strip && hdiff_fits(cols) && hdiff_stage_fits(cols))
            pl.hdiff = hd_octave_matches<2>(pl.taps) ? 2 : hd_octave_matches<3>(pl.taps) ? 3 : 0;
    }
    if (pl.path != OctPath::Generic) pl.mx = mx_config_for(pl.ke);
    return pl;
}

// The plan of every octave of a call: made once by the entry point; scratch sizing, side gate and launches all read this array.
static std::vector<OctPlan> plan_octaves(double sigma0, const vslam_batch_layout& L) {
    std::vector<OctPlan> plans;
    for (int o = 0; o < L.n_octaves; ++o) plans.push_back(plan_octave(sigma0, o, L.rows[o], L.cols[o]));
    return plans;
}

// The two horizontal passes of a strip octave, launched as strip_launch() (vslam_octave_launch.h) chose.
template <int SH, int RI>
static int launch_h_strip(vslam_ctx* c, const uint16_t* h, size_t hframe, const OctIO& io, const StripLaunch& sl, const StripTaps* taps) {
    TRY(raise_dyn_lds(c, reinterpret_cast<const void*>(&k_gauss_h_strip<SH, RI>)));
    LAUNCH_ON(c, "k_gauss_h_strip", c->launch_tag, c->stream, sl.h_lds, (k_gauss_h_strip<SH, RI>), dim3(1, sl.h_grid_y, io.nf), dim3(256), h,
              hframe, io.oct, io.pframe, io.rows, io.cols, io.pitch, sl.pw, taps, io.next_base, io.nframe, io.nrows, io.ncols, io.npitch);
    return VSLAM_OK;
}

template <int O>
static int launch_h_diff(vslam_ctx* c, const uint16_t* h, size_t hframe, const OctIO& io, const StripLaunch& sl) {
    TRY(raise_dyn_lds(c, reinterpret_cast<const void*>(&k_gauss_h_diff<O>)));
    // the timing hook's "k_gauss_h_strip" is the coarse octaves' horizontal pass whichever kernel runs it (bench.py's
    // per-kernel figures, the dispatch tests); "k_gauss_h_diff" times this kernel alone
    TimedScope ts(c, "k_gauss_h_strip", c->launch_tag);
    LAUNCH_ON(c, "k_gauss_h_diff", c->launch_tag, c->stream, sl.h_lds, k_gauss_h_diff<O>, dim3(1, sl.h_grid_y, io.nf), dim3(256), h,
              hframe, io.oct, io.pframe, io.rows, io.cols, io.pitch, sl.npairs, sl.pw, io.next_base, io.nframe, io.nrows, io.ncols, io.npitch);
    return VSLAM_OK;
}

// Coarse octave: vertical strips (dot4) into the u16 scratch, then horizontal strips (dot2, or the difference form).
static int enqueue_strip_octave(vslam_ctx* c, double sigma0, int o, const OctPlan& pl, const OctIO& io, uint16_t* h) {
    const StripTaps* taps;
    TRY(get_table(c, kTableStrip, sigma0, o, "strip kernels", sizeof(StripTaps), [&](void* host) -> int {
        const uint16_t* tp[6];
        tap_pointers(pl.taps, tp);
        if (!strip_pack_taps(tp, pl.ke, *static_cast<StripTaps*>(host))) return fail(c, VSLAM_ERR_UNSUPPORTED, "strip kernels: taps out of range");
        return VSLAM_OK;
    }, &taps));
    const int rows = io.rows, cols = io.cols, nf = io.nf;
    // Diagnostics build only: VSLAM_HDIFF=0 keeps the dot2 pass where the difference form would run (A/B runs, byte-equality test)
    static const bool hdiff_off = [] {
        const char* e = VSLAM_DIAG_ENV("VSLAM_HDIFF");
        return e && e[0] == '0';
    }();
    const int hd = hdiff_off ? 0 : pl.hdiff;
    const StripLaunch sl = hd == 2   ? strip_launch(rows, cols, nf, pl.sh, true, pl.nmax, HdGeom<2>::HL, HdGeom<2>::rmax)
                           : hd == 3 ? strip_launch(rows, cols, nf, pl.sh, true, pl.nmax, HdGeom<3>::HL, HdGeom<3>::rmax)
                                     : strip_launch(rows, cols, nf, pl.sh, false, pl.nmax);
    const StripVGeom vg = strip_v_geom(rows, pl.nmax);
    const size_t P = (size_t)rows * io.pitch;
    TRY(raise_dyn_lds(c, reinterpret_cast<const void*>(&k_gauss_v_strip)));
    LAUNCH_ON(c, "k_gauss_v_strip", o, c->stream, sl.v_lds, k_gauss_v_strip, dim3((cols + STRIP_W - 1) / STRIP_W, sl.lsplit, nf), dim3(256), io.base, io.bframe,
              h, 6 * P, rows, cols, io.pitch, vg.RM, vg.rhq, taps);
    c->launch_tag = o;
    if (sl.diff) return hd == 2 ? launch_h_diff<2>(c, h, 6 * P, io, sl) : launch_h_diff<3>(c, h, 6 * P, io, sl);
    // the six instantiations strip_launch() chooses among (tests/test_octave_launch_cpu.py: no other pair ever comes back)
    switch (sl.SH * 8 + sl.RI) {
        case 16 * 8 + 4: return launch_h_strip<16, 4>(c, h, 6 * P, io, sl, taps);
        case 16 * 8 + 2: return launch_h_strip<16, 2>(c, h, 6 * P, io, sl, taps);
        case 16 * 8 + 1: return launch_h_strip<16, 1>(c, h, 6 * P, io, sl, taps);
        case 8 * 8 + 4: return launch_h_strip<8, 4>(c, h, 6 * P, io, sl, taps);
        case 4 * 8 + 4: return launch_h_strip<4, 4>(c, h, 6 * P, io, sl, taps);
        case 4 * 8 + 1: return launch_h_strip<4, 1>(c, h, 6 * P, io, sl, taps);
    }
    return fail(c, VSLAM_ERR_UNSUPPORTED, "strip kernels: no instantiation for the chosen strip shape");
}


// GaussianBlur CV_8U on nf dense images; h = u16 scratch of nf*rows*cols elements.
static int enqueue_blur(vslam_ctx* c, const uint8_t* src, size_t sstep, size_t sframe, uint8_t* dst, size_t dstep,
                        size_t dframe, uint16_t* h, int rows, int cols, int nf, int n, double sigma) {
    const uint16_t* taps;
    int rc = get_taps(c, n, sigma, &taps, &n);  // n becomes the trimmed width
    if (rc) return rc;
    const size_t P = (size_t)rows * cols;
    LAUNCH(c, "k_blur_h_generic", k_blur_h_generic, grid_rows(cols, rows, nf), dim3(256), src, sstep, sframe, h, P,
           rows, cols, taps, n);
    LAUNCH(c, "k_blur_v_generic", k_blur_v_generic, grid_rows(cols, rows, nf), dim3(256), h, P, dst, dstep, dframe,
           rows, cols, taps, n);
    return VSLAM_OK;
}

// count -> scan -> scatter over the flag entries of nf frames (kernels_compact.hip.h).
// chunk_ws: scratch of nf * chunks u32.
template <class E>
static int enqueue_compaction(vslam_ctx* c, const E& ent, size_t entries, int nf, unsigned int* chunk_ws, unsigned int cap,
                              unsigned int* counts, int append) {
    const int nchunks = (int)((entries + CMP_CHUNK - 1) / CMP_CHUNK);
    if (nchunks == 0) {
        if (!append) HIPCHK(c, hipMemsetAsync(counts, 0, sizeof(unsigned int) * (size_t)nf, c->stream));
        return VSLAM_OK;
    }
    LAUNCH(c, "k_flag_count", k_flag_count<E>, dim3(nchunks, 1, nf), dim3(256), ent, chunk_ws, nchunks);
    LAUNCH(c, "k_chunk_scan", k_chunk_scan, dim3(nf), dim3(256), chunk_ws, nchunks, counts, append);
    LAUNCH(c, "k_flag_scatter", k_flag_scatter<E>, dim3(nchunks, 1, nf), dim3(256), ent, chunk_ws, nchunks, cap);
    return VSLAM_OK;
}
static inline size_t compaction_ws_elems(size_t entries, int nf) { return (size_t)nf * ((entries + CMP_CHUNK - 1) / CMP_CHUNK) + 64; }

size_t vslam::match_list_ws_elems(size_t fwords, int n_pairs) { return compaction_ws_elems(fwords, n_pairs); }
int vslam::enqueue_match_list(vslam_ctx* c, const unsigned long long* flags, size_t fwords, const vslam_nn2* nn, unsigned int qcap, int n_pairs,
                              unsigned int* chunk_ws, vslam_match* matches, unsigned int match_cap, unsigned int* match_counts) {
    const MatchEntries ent{flags, fwords, nn, qcap, matches};
    return enqueue_compaction(c, ent, fwords, n_pairs, chunk_ws, matches ? match_cap : 0u, match_counts, 0);
}

int vslam::enqueue_inlier_list(vslam_ctx* c, const unsigned long long* flags, size_t fwords, const vslam_match* matches, const unsigned int* match_counts,
                               unsigned int match_cap, int n_pairs, unsigned int* chunk_ws, vslam_match* inliers, unsigned int inlier_cap,
                               unsigned int* inlier_counts) {
    const EpipolarEntries ent{flags, fwords, matches, match_counts, match_cap, inliers};
    return enqueue_compaction(c, ent, fwords, n_pairs, chunk_ws, inliers ? inlier_cap : 0u, inlier_counts, 0);
}

// The table of the localization's quadratic term, filled by the same device function that the
// kernels fall back to (so a lookup cannot differ from the computation).
static int ensure_loc_lut(vslam_ctx* c) {
    if (c->loc_lut) return VSLAM_OK;
    constexpr int n = LOC_LUT_N * LOC_LUT_N * LOC_LUT_N;
    float* lut = nullptr;
    HIPCHK(c, hipMalloc((void**)&lut, sizeof(float) * n));
    hipLaunchKernelGGL(k_build_localization_lut, dim3((n + 255) / 256), dim3(256), 0, c->stream, lut);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {  // never leave a table that was not built
        (void)hipFree(lut);
        return fail(c, VSLAM_ERR_HIP, std::string("k_build_localization_lut: ") + hipGetErrorString(e));
    }
    c->loc_lut = lut;
    return VSLAM_OK;
}

static void fill_geom(const vslam_ctx* c, const vslam_params& p, const vslam_batch_layout& L, ExtGeom& g) {
    std::memset(&g, 0, sizeof(g));
    g.loc_lut = c->loc_lut;
    g.n_oct = L.n_octaves;
    g.window = p.extrema_window;
    g.pad = (p.extrema_window - 1) / 2;
    g.min_contrast = p.min_contrast;
    g.localize = p.localize;
    for (int o = 0; o < L.n_octaves; ++o) {
        g.rows[o] = L.rows[o];
        g.cols[o] = L.cols[o];
        g.pitch[o] = L.pitch[o];
        g.lat_rows[o] = L.lat_rows[o];
        g.lat_cols[o] = L.lat_cols[o];
        g.wpr[o] = L.lat_words[o];
        g.oct_off[o] = L.octave_offset[o];
        g.bits_off[o] = L.bits_offset[o];
    }
}

struct DogScratch {
    uint8_t* bases = nullptr;  // nf * sum_P
    size_t bases_frame = 0;
    size_t base_off[VSLAM_MAX_OCTAVES] = {};
    uint16_t* h = nullptr;  // nf * P0 u16
    unsigned long long* lflags = nullptr;
    unsigned int* cws = nullptr;  // compaction chunk totals / offsets
    unsigned int* pbegin = nullptr;  // localize mode: per-frame list length before the current octave
    // matrix path with the lattice scan fused into the octave kernel: one byte per lattice site of the octaves that kernel covers
    uint8_t* sitemap = nullptr;
    size_t site_frame = 0, site_off[VSLAM_MAX_OCTAVES] = {};
    int site_pitch[VSLAM_MAX_OCTAVES] = {};
    // ... and the two DoG columns on either side of every seam between its 128-column strips (vslam_mx.h: MxScan::colmap)
    uint8_t* colmap = nullptr;
    size_t col_frame = 0, col_off[VSLAM_MAX_OCTAVES] = {};
};

static inline int site_pitch_of(int lat_cols) { return (lat_cols + 63) & ~63; }
static size_t col_octave_bytes(const vslam_batch_layout& L, int o) { return align_up((size_t)5 * mx_seams(L.cols[o]) * L.rows[o] * 2, 16); }

// u16 scratch elements per frame: 6 row-sum images for a strip octave, 1 for a generic octave,
// none for the LDS-tiled octaves.
static size_t dog_h_elems(const vslam_batch_layout& L, const std::vector<OctPlan>& plans) {
    size_t m = 0;
    for (int o = 0; o < L.n_octaves; ++o) {
        const size_t P = (size_t)L.rows[o] * L.pitch[o];
        if (plans[o].path == OctPath::Strip) m = std::max(m, 6 * P);
        if (plans[o].path == OctPath::Generic) m = std::max(m, P);
    }
    return m;
}

// The DoG path's scratch for nf frames: fills the geometry of `s` and asks `ws` for its buffers.
static void dog_scratch_plan(WsPlan& ws, const vslam_batch_layout& L, const std::vector<OctPlan>& plans, int nf, DogScratch& s, bool sitemap = false) {
    if (sitemap) {
        size_t off = 0;
        for (int o = 0; o < L.n_octaves; ++o) {
            s.site_off[o] = off;
            s.site_pitch[o] = site_pitch_of(L.lat_cols[o]);
            off += (size_t)L.lat_rows[o] * s.site_pitch[o];
        }
        s.site_frame = off;
        ws.add(s.sitemap, (size_t)nf * off);
        size_t coff = 0;
        for (int o = 0; o < L.n_octaves; ++o) {
            s.col_off[o] = coff;
            coff += col_octave_bytes(L, o);
        }
        s.col_frame = coff;
        ws.add(s.colmap, (size_t)nf * coff + 16);
    }
    size_t sum_p = 0;
    for (int o = 0; o < L.n_octaves; ++o) {
        s.base_off[o] = sum_p;  // octave bases keep the pitched rows of the pyramid planes
        sum_p += (size_t)L.rows[o] * L.pitch[o];
    }
    s.bases_frame = sum_p;
    ws.add(s.bases, (size_t)nf * sum_p);
    ws.add(s.h, (size_t)nf * dog_h_elems(L, plans) + 128);
    ws.add(s.lflags, (size_t)nf * L.bits_frame_words);
    ws.add(s.cws, compaction_ws_elems(L.bits_frame_words, nf));
    ws.add(s.pbegin, nf);
}


// Fused LDS-tiled octave (kernels_pyramid.hip.h); the plan has already matched CFG's widths.
template <class CFG>
static int enqueue_pyr_octave(vslam_ctx* c, double sigma0, int o, const OctPlan& pl, const OctIO& io) {
    const PyrTaps<CFG>* taps = nullptr;  // (a configuration with compiled-in taps reads no table)
    if constexpr (CFG::DO == 0)
        TRY(get_table(c, kTableTile, sigma0, o, "octave kernel", sizeof(PyrTaps<CFG>), [&](void* host) -> int {
            const uint16_t* tp[6];
            tap_pointers(pl.taps, tp);
            pyr_pack_taps<CFG>(tp, *static_cast<PyrTaps<CFG>*>(host));
            return VSLAM_OK;
        }, &taps));
    TRY(raise_dyn_lds(c, reinterpret_cast<const void*>(&k_pyr_octave<CFG>)));  // once per kernel (both tile shapes share the taps)
    const dim3 grid((io.cols + CFG::TW - 1) / CFG::TW, (io.rows + CFG::TH - 1) / CFG::TH, io.nf);
    LAUNCH_ON(c, "k_pyr_octave", o, c->stream, CFG::LDS_BYTES, k_pyr_octave<CFG>, grid, dim3(CFG::NT), io.base, io.bframe, io.oct, io.pframe, io.rows,
              io.cols, io.pitch, taps, io.next_base, io.nframe, io.nrows, io.ncols, io.npitch);
    return VSLAM_OK;
}

// The same octave through the matrix-core kernel (kernels_pyramid_mx.hip.h, vslam_mx.hip), configuration pl.mx.
static int enqueue_pyr_octave_mx(vslam_ctx* c, double sigma0, int o, const OctPlan& pl, const OctIO& io, const MxScan* scan, int up2_step = 0) {
    const void* table;
    TRY(get_table(c, kTableMx, sigma0, o, "matrix-core octave kernel", mx_taps_bytes(pl.mx), [&](void* host) -> int {
        const uint16_t* tp[6];
        tap_pointers(pl.taps, tp);
        if (!mx_pack(pl.mx, tp, host)) return fail(c, VSLAM_ERR_UNSUPPORTED, "matrix-core octave kernel: a tap exceeds 127");
        HIPCHK(c, mx_prepare(pl.mx));
        return VSLAM_OK;
    }, &table));
    hipError_t e;
    {
        TimedScope ts(c, "k_pyr_octave_mx", o);
        e = mx_launch(pl.mx, c->stream, table, io, scan, up2_step);
    }
    HIPCHK(c, e);
    return VSLAM_OK;
}

// Geometry of the dense 3x3x3 scan (kernels_extrema_dense.hip.h) for octave o of nf frames.
static DenseGeom dense_geom(const vslam_batch_layout& L, int o, int min_contrast, int nf) {
    DenseGeom g;
    g.rows = L.rows[o], g.cols = L.cols[o], g.pitch = L.pitch[o];
    g.wpr = (g.cols + 63) / 64;
    g.min_contrast = min_contrast;
    g.P = (unsigned int)((size_t)g.rows * g.pitch);
    g.dog_off = (unsigned int)(L.octave_offset[o] + (size_t)VSLAM_NUM_LEVELS * g.P);
    // a lane walks g.seg rows: long segments amortise the two halo rows, short ones give a small launch
    // enough waves to hide the loads (about 8 per SIMD)
    const long waves_per_rowseg = 4L * (((g.cols + 3) / 4 + 255) / 256) * nf;
    const long segs_wanted = std::max<long>(1, 8192 / waves_per_rowseg);
    g.seg = (int)std::min<long>(XD_SEG_MAX, std::max<long>(4, (g.rows + segs_wanted - 1) / segs_wanted));
    return g;
}

namespace {
// Where enqueue_dog writes: per-frame blocks with the given strides.
struct DogOut {
    uint8_t* pyr;
    size_t pframe;
    unsigned long long* bits = nullptr;  // candidate bits (optional)
    bool do_extrema = false;             // run the lattice scans at all
    vslam_point* points = nullptr;       // the frames' point lists and their lengths (optional, both or none)
    unsigned int* counts = nullptr;
};

// A lane of the plan as a stream.  (Lane::Main is the context's current stream: ask for it outside a StreamSwap.)
static inline hipStream_t lane_stream(const vslam_ctx* c, Lane l) { return l == Lane::Main ? c->stream : c->aux[(int)l - 1]; }

// What the plan of a chunk takes from the layout, the octave plans and the parameters; the caller adds nf, the outputs asked
// for (harris, do_extrema, lists) and the state of the call (bases_are_scratch, side, capturing, later_chunk).
static BatchPlanIn batch_plan_input(const vslam_ctx* c, const vslam_params& p, const vslam_batch_layout& L, const std::vector<OctPlan>& plans, size_t fstep) {
    BatchPlanIn in;
    in.n_octaves = L.n_octaves;
    for (int o = 0; o < L.n_octaves; ++o) {
        in.tiled[o] = plans[o].path == OctPath::Tile0 || plans[o].path == OctPath::Tile1;
        in.lattice[o] = L.lat_rows[o] > 0 && L.lat_cols[o] > 0;
        in.scan_ok[o] = mx_scan_supported(plans[o].mx);
    }
    in.up2_ok = L.n_octaves > 0 && L.rows[0] == 2 * p.rows && L.cols[0] == 2 * p.cols && fstep <= 0x7fffffff && mx_up2_supported(plans[0].mx);
    in.dog = L.n_octaves > 0;
    in.localize = p.localize, in.orient = p.orient, in.extrema_dense = p.extrema_dense, in.extrema_window = p.extrema_window;
    in.mx = c->mx;
    return in;
}

// One chunk of the DoG path, as the steps of enqueue_dog share it.  `plan` (vslam_batch_plan.h) says on which lane and when
// every piece goes; the steps decide nothing of that themselves.
struct DogChunk {
    const vslam_params& p;
    const vslam_batch_layout& L;
    const std::vector<OctPlan>& plans;  // plan_octaves() of the same (sigma0, layout), as given to dog_scratch_plan
    const uint8_t* frames;
    size_t fstep, fframe;
    int nf;
    DogScratch& s;
    DogOut out;
    BatchPlan plan;
    ExtGeom g{};
    MxScan scan[VSLAM_MAX_OCTAVES] = {};  // of the octaves whose lattice scan runs inside the octave kernel (plan.fused[o])

    // First: octave 0's bases, and what a later chunk owes the readers of the chunk before.
    int begin(vslam_ctx* c) {
        const int nf_a = plan.nf_a;
        if (p.localize) TRY(ensure_loc_lut(c));
        fill_geom(c, p, L, g);
        // (the halves of a large batch and octave 0's fused upsample: vslam_batch_plan.h)
        if (!plan.up2_fused)
            LAUNCH(c, "k_resize_linear2x_slide", k_resize_linear2x_slide, dim3(((p.cols + 3) / 4 + 255) / 256, (p.rows + 15) / 16, nf_a), dim3(256),
                   frames, fstep, fframe, s.bases + s.base_off[0], s.bases_frame, L.pitch[0], p.rows, p.cols, 16);
        if (nf_a < nf) {
            const hipStream_t up = lane_stream(c, plan.up_lane);
            if (plan.up_waits_chunk) HIPCHK(c, hipStreamWaitEvent(up, c->ev_chunk, 0));
            StreamSwap sw(c, up);
            LAUNCH(c, "k_resize_linear2x_slide", k_resize_linear2x_slide, dim3(((p.cols + 3) / 4 + 255) / 256, (p.rows + 15) / 16, nf - nf_a), dim3(256),
                   frames + (size_t)nf_a * fframe, fstep, fframe, s.bases + s.base_off[0] + (size_t)nf_a * s.bases_frame, s.bases_frame, L.pitch[0],
                   p.rows, p.cols, 16);
            HIPCHK(c, hipEventRecord(c->ev_up2, c->stream));
        }
        // a later chunk reuses the site / seam maps: its octave kernels (main stream) must not overwrite them while the previous
        // chunk's k_extrema_pack launches (side stream, low priority, possibly on a slow hardware queue) are still reading
        if (plan.wait_pack) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_pack, 0));
        // matrix path: the plain lattice scan (window 3, candidates + contrast list) runs inside the octave kernel
        // while the DoG rows are in LDS (kernels_pyramid_mx.hip.h); k_extrema_pack then replaces k_extrema_w3
        for (int o = 0; o < L.n_octaves; ++o)
            if (plan.fused[o])
                scan[o] = MxScan{s.sitemap + s.site_off[o], s.site_frame, L.lat_rows[o], L.lat_cols[o], s.site_pitch[o], p.min_contrast,
                                   s.colmap + s.col_off[o], s.col_frame, mx_seams(L.cols[o])};
        return VSLAM_OK;
    }

    // (scan_octave stands in front of octave on purpose: kernels are emitted in the order of their first use, and with the
    // octave kernels in front of k_extrema_w3 the localize modes measured 0.4 % slower - profiles/batch_plan_ab.txt)
    // Once per octave, when the plan says (after[o]): the lattice scan of octave o (initialKeypointDetection, Diff_of_Gauss.cpp:254) and the compaction
    // of its points into the frames' lists; on the list lane both wait for ev_oct[o_done], the octave whose kernels were enqueued last.
    int scan_octave(vslam_ctx* c, int o, int o_done) {
        uint8_t* const pyr = out.pyr;
        const size_t pframe = out.pframe;
        unsigned long long* const bits = out.bits;
        const bool on_side = plan.scan_lane != Lane::Main;
        const hipStream_t es = lane_stream(c, plan.scan_lane);
        if (out.do_extrema && L.lat_rows[o] > 0 && L.lat_cols[o] > 0) {
            if (on_side) HIPCHK(c, hipStreamWaitEvent(es, c->ev_oct[o_done], 0));
            if (p.extrema_dense) {
                // extension: the dense 3x3x3 test on every pixel (kernels_extrema_dense.hip.h); the layout's
                // lattice of this mode is the image itself
                const DenseGeom dg = dense_geom(L, o, p.min_contrast, nf);
                hipLaunchKernelGGL(k_extrema_dense, dim3(((dg.cols + 3) / 4 + 255) / 256, (dg.rows + dg.seg - 1) / dg.seg, nf), dim3(256), 0, es,
                                   pyr, pframe, dg, bits ? bits + L.bits_offset[o] : nullptr, s.lflags + L.bits_offset[o], L.bits_frame_words);
            } else if (plan.fused[o]) {  // the octave kernel has left the site / seam maps
                {
                    TimedScope ts(c, "k_extrema_pack", o, es);
                    HIPCHK(c, mx_launch_pack(es, scan[o], L.rows[o], L.lat_words[o], nf, bits ? bits + L.bits_offset[o] : nullptr, s.lflags + L.bits_offset[o],
                                             L.bits_frame_words, kMxStripRows));
                }
                // the lattice rows whose windows straddle a strip's first image row (3a a multiple of the strip's rows, a power of two:
                // a = 32, 64, ...) are not in the site map: the plain scan kernel runs on exactly those rows
                const int sr = kMxStripRows;
                const int n_straddle = (L.lat_rows[o] - 1) / sr;
                TimedScope ts(c, "k_extrema_w3", o, es);
                if (n_straddle > 0)
                    hipLaunchKernelGGL(k_extrema_w3<false>, dim3((L.lat_words[o] + 3) / 4, n_straddle, nf), dim3(256), 0, es, pyr, pframe, g, o, bits, s.lflags,
                                       L.bits_frame_words, sr, sr);
                // the maps' reader is on another stream than their writer: mark its end for the next chunk (plan.wait_pack)
                if (on_side) HIPCHK(c, hipEventRecord(c->ev_pack, es));
            } else if (p.extrema_window == 3) {
                const dim3 eg((L.lat_words[o] + 3) / 4, L.lat_rows[o], nf);
                if (p.localize)
                    LAUNCH_ON(c, "k_extrema_w3", o, es, 0, k_extrema_w3<true>, eg, dim3(256), pyr, pframe, g, o, bits, s.lflags, L.bits_frame_words, 0, 1);
                else
                    LAUNCH_ON(c, "k_extrema_w3", o, es, 0, k_extrema_w3<false>, eg, dim3(256), pyr, pframe, g, o, bits, s.lflags, L.bits_frame_words, 0, 1);
            } else
                hipLaunchKernelGGL(k_extrema, dim3((L.lat_cols[o] + 255) / 256, L.lat_rows[o], nf * 3), dim3(256), 0, es, pyr,
                                   pframe, g, o, bits, s.lflags, L.bits_frame_words);
            HIPCHK(c, hipGetLastError());
        }
        // compact this octave's points right away (appending to the frame's list): on the side
        // stream it overlaps the next octave's kernels instead of forming a serial tail
        if (out.do_extrema && out.points && out.counts) {
            StreamSwap sw(c, es);
            const size_t entries = (size_t)3 * L.lat_rows[o] * L.lat_words[o];
            if (p.extrema_dense) {
                DenseDogEntries ent{s.lflags + L.bits_offset[o], L.bits_frame_words, pyr, pframe, dense_geom(L, o, p.min_contrast, nf), o, out.points};
                TRY(enqueue_compaction(c, ent, entries, nf, s.cws, p.dog_cap, out.counts, o > 0 ? 1 : 0));
            } else {
                DogEntries ent{s.lflags, L.bits_frame_words, pyr, pframe, g, o, o + 1, out.points};
                TRY(enqueue_compaction(c, ent, entries, nf, s.cws, p.dog_cap, out.counts, o > 0 ? 1 : 0));
            }
        }
        return VSLAM_OK;
    }

    // Once per octave: the kernels of octave o (createPyramid, GaussPyramid.cpp:106-131) and the event that marks their end.
    int octave(vslam_ctx* c, int o) {
        const int nf_a = plan.nf_a;
        const int rows = L.rows[o], cols = L.cols[o], pitch = L.pitch[o];
        const size_t P = (size_t)rows * pitch;
        const OctPlan& pl = plans[o];
        // the fast octave kernels also emit the next octave's base (Gaussian[3] decimated 2:1)
        const bool has_next = o + 1 < L.n_octaves;
        const bool fuse_next = has_next && pl.path != OctPath::Generic;
        OctIO io{s.bases + s.base_off[o], s.bases_frame, out.pyr + L.octave_offset[o], out.pframe, rows, cols, pitch, nf,
                 fuse_next ? s.bases + s.base_off[o + 1] : nullptr, s.bases_frame, has_next ? L.rows[o + 1] : 0, has_next ? L.cols[o + 1] : 0,
                 has_next ? L.pitch[o + 1] : 0};
        const bool up2 = o == 0 && plan.up2_fused;
        if (up2) io.base = frames, io.bframe = fframe;  // the kernel reads the source frames (mx_launch: up2_step)
        const int shape = pyr_tile_wide(rows, cols) ? 1 : 0;  // the wide tile (256 x 32) or the tall one (128 x 64)
        const bool fused = plan.fused[o];
        // frames [f_lo, f_lo + n) of this octave through the LDS-tiled kernel
        auto tiled = [&](int f_lo, int n) -> int {
            const OctIO part = io.frames(f_lo, n);
            if (c->mx && pl.mx) {
                MxScan sc = scan[o];
                if (fused) sc.sitemap += (size_t)f_lo * s.site_frame, sc.colmap += (size_t)f_lo * s.col_frame;
                return enqueue_pyr_octave_mx(c, p.sigma0, o, pl, part, fused ? &sc : nullptr, up2 ? (int)fstep : 0);
            }
            if (pl.path == OctPath::Tile0)
                return shape == 1 ? enqueue_pyr_octave<PyrCfgOct0W>(c, p.sigma0, o, pl, part) : enqueue_pyr_octave<PyrCfgOct0>(c, p.sigma0, o, pl, part);
            if (pl.ctaps == 1)  // the plan's taps are the compiled-in ones
                return shape == 1 ? enqueue_pyr_octave<PyrCfgOct1WC>(c, p.sigma0, o, pl, part) : enqueue_pyr_octave<PyrCfgOct1C>(c, p.sigma0, o, pl, part);
            return shape == 1 ? enqueue_pyr_octave<PyrCfgOct1W>(c, p.sigma0, o, pl, part) : enqueue_pyr_octave<PyrCfgOct1>(c, p.sigma0, o, pl, part);
        };
        // opt-in matrix path: also the octaves the default path runs through the strip kernels (no u16 scratch round trip)
        const bool is_tiled = pl.path == OctPath::Tile0 || pl.path == OctPath::Tile1 || (c->mx && pl.mx != 0);
        if (o == 0 && nf_a < nf && !is_tiled) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_up2, 0));  // octave 0 needs every base
        if (is_tiled && o == 0 && nf_a < nf) {
            TRY(tiled(0, nf_a));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_up2, 0));
            TRY(tiled(nf_a, nf - nf_a));
        } else if (is_tiled)
            TRY(tiled(0, nf));
        else if (pl.path == OctPath::Strip)
            TRY(enqueue_strip_octave(c, p.sigma0, o, pl, io, s.h));
        else {
            for (int l = 0; l < VSLAM_NUM_LEVELS; ++l)
                TRY(enqueue_blur(c, io.base, (size_t)pitch, s.bases_frame, io.oct + (size_t)l * P, (size_t)pitch, out.pframe, s.h, rows,
                                 cols, nf, pl.ks[l], pl.sg[l]));
            LAUNCH(c, "k_dog5", k_dog5, dim3((unsigned)((P + 255) / 256), 1, nf), dim3(256), io.oct,
                   io.oct + (size_t)VSLAM_NUM_LEVELS * P, P, out.pframe);
        }
        if (has_next && !fuse_next)
            LAUNCH(c, "k_resize_nearest_half_v4", k_resize_nearest_half_v4, dim3((L.cols[o + 1] / 4 + 256) / 256, L.rows[o + 1], nf),
                   dim3(256), io.oct + (size_t)3 * P, out.pframe, pitch, s.bases + s.base_off[o + 1], s.bases_frame, L.pitch[o + 1], rows,
                   L.rows[o + 1], L.cols[o + 1]);
        if (plan.ev_oct) HIPCHK(c, hipEventRecord(c->ev_oct[o], c->stream));
        if (o == 0) TRY(sched_mark_phase(c));
        return VSLAM_OK;
    }
};

// The Harris chain of one chunk (enqueue_harris's arguments).
struct HarrisChunk {
    const uint8_t* frames;
    size_t fframe;
    int rows, cols, nf;
    float k, *resp;
    uint8_t* mask;
    float* nms2;
    unsigned long long* hflags;
    vslam_kp* kps;
    unsigned int cap, *counts, *cws;
};
}  // namespace


struct OrientPlan;
struct OrientScratch;
// One chunk of the DoG path with what the plan interleaves with it (defined with the batched path below): the Harris chain
// `hc` at the gate, and the early edge test of the orientation stage (`opl`, `os`) behind octave 0's list.
static int enqueue_dog(vslam_ctx* c, DogChunk& d, const HarrisChunk* hc = nullptr, const OrientPlan* opl = nullptr, OrientScratch* os = nullptr);

// Harris chain on nf device frames with dense rows: response (required buffer), optional mask /
// nms2 / keypoint list, all from the single-pass wave-strip kernel - its aligned form when every
// row and frame starts on a dword, the any-width form otherwise.  Strips, segments, grid and the
// flag words per frame (harris_flag_words) are vslam_harris_launch.h's.
static int enqueue_harris(vslam_ctx* c, const uint8_t* frames, size_t fframe, int rows, int cols, int nf, float k,
                          float* resp, uint8_t* mask, float* nms2, unsigned long long* hflags, vslam_kp* kps,
                          unsigned int cap, unsigned int* counts, unsigned int* chunk_ws) {
    const size_t N = (size_t)rows * cols;
    if (N >= ((size_t)1 << 31)) return fail(c, VSLAM_ERR_UNSUPPORTED, "Harris: images of 2^31 pixels or more are not supported (32-bit row offsets)");
    const HarrisLaunch g = harris_launch(rows, cols, nf, fframe);
    HarrisStripArgs a;
    a.img = frames;
    a.frame = fframe;
    a.rows = rows;
    a.cols = cols;
    a.k = k;
    a.resp = resp;
    a.mask = mask;
    a.nms2 = nms2;
    a.flags = hflags;
    a.nstrips = g.nstrips;
    a.fframe = g.flag_words;
    a.seg = g.seg;
    if (!c->dump) HIPCHK(c, hipMalloc((void**)&c->dump, 256));
    a.dump = c->dump;
    if (g.aligned)
        LAUNCH(c, "k_harris_strip", k_harris_strip<false>, dim3(g.grid_x, 1, nf), dim3(64 * HS_WAVES), a);
    else
        LAUNCH(c, "k_harris_strip", k_harris_strip<true>, dim3(g.grid_x, 1, nf), dim3(64 * HS_WAVES), a);
    if (hflags && kps && counts) {
        HarrisStripEntries ent{hflags, a.fframe, rows, cols, a.nstrips, resp, N, kps};
        TRY(enqueue_compaction(c, ent, (size_t)rows * a.nstrips, nf, chunk_ws, cap, counts, 0));
    }
    return VSLAM_OK;
}

static int h2d(vslam_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
               size_t rows) {
    // dense rows are one linear copy: hipMemcpy2D degrades to a copy per row for widths that are
    // not a multiple of 4 bytes (9 ms instead of 0.1 ms for a 1754x1240 image)
    if (dpitch == width_bytes && spitch == width_bytes)
        HIPCHK(c, hipMemcpyAsync(dst, src, width_bytes * rows, hipMemcpyHostToDevice, c->stream));
    else
        HIPCHK(c, hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, rows, hipMemcpyHostToDevice, c->stream));
    return VSLAM_OK;
}
static int d2h(vslam_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width_bytes,
               size_t rows) {
    if (dpitch == width_bytes && spitch == width_bytes)
        HIPCHK(c, hipMemcpyAsync(dst, src, width_bytes * rows, hipMemcpyDeviceToHost, c->stream));
    else
        HIPCHK(c, hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, rows, hipMemcpyDeviceToHost, c->stream));
    return VSLAM_OK;
}

// The end of the entry points that return a list: wait for the stream, then *count = what the kernels counted (it may
// exceed cap) and the first min(count, cap) records.  `bits`: candidate words to fetch in the same wait (bits_bytes = 0: none).
template <class R>
static int read_list(vslam_ctx* c, const unsigned int* d_count, const R* d_list, size_t cap, R* out, size_t* count, uint64_t* bits = nullptr,
                     const unsigned long long* d_bits = nullptr, size_t bits_bytes = 0) {
    unsigned int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, d_count, 4, hipMemcpyDeviceToHost, c->stream));
    if (bits_bytes) HIPCHK(c, hipMemcpyAsync(bits, d_bits, bits_bytes, hipMemcpyDeviceToHost, c->stream));
    TRY(vslam_ctx_sync(c));
    *count = n;
    const size_t m = std::min<size_t>(n, cap);
    if (m) HIPCHK(c, hipMemcpy(out, d_list, m * sizeof(R), hipMemcpyDeviceToHost));
    return VSLAM_OK;
}

// ---------------------------------------------------------------- what filterKeypoints and SIFT share, per image and batched

// Device copy of getGaussianKernel(n, sigma, CV_32F) for the blur of filterKeypoints and SIFT (sigma = 1.5 * sigma(o, l)), cached
// per context by (sigma, n): the per-image entry points and the batched path read the same tables.  `what`: the caller's
// prefix in error texts.
static int get_orient_taps(vslam_ctx* c, double sigma, const char* what, const float** out, int* n_out) {
    const int n = gauss_ksize_f32(sigma);
    if (n <= 0 || n > (1 << 20)) return fail(c, VSLAM_ERR_INVALID, std::string(what) + ": bad blur kernel");  // before n sizes the table
    *n_out = n;
    return get_table(c, kTableOrient, sigma, n, what, 4 * (size_t)orient_taps_pk_floats(n), [&](void* host) -> int {
        std::vector<float> k;
        if (!gauss_kernel_f32(n, sigma, k)) return fail(c, VSLAM_ERR_INVALID, std::string(what) + ": bad blur kernel");
        float* t = static_cast<float*>(host);
        std::copy(k.begin(), k.end(), t);
        // behind the taps: the zero-padded row / column forms k_orient_survivors_pk reads through scalar loads
        for (int i = 0; i < n; ++i) t[(size_t)orient_taps_row_off(n) + 3 + i] = t[(size_t)i];
        for (int i = 1; i <= n / 2; ++i) t[(size_t)orient_taps_col_off(n) + i - 1] = t[(size_t)(n / 2 + i)];
        return VSLAM_OK;
    }, out);
}

// What the per-image filterKeypoints and SIFT share: the keypoints' range checks (coordinates may leave the octave by
// `margin`; what the reference would throw on - vector::at(level), a Rect outside the padded Mat - or could not have
// produced is an error here), and for every level a keypoint uses its Gaussian plane and the cached taps of
// sigma = 1.5 * sigma(octave, level) (Diff_of_Gauss.cpp:346, :616).  Levels no keypoint uses stay null / 0.
struct KeypointLevels {
    bool used[VSLAM_NUM_LEVELS] = {};
    const uint8_t* gauss[VSLAM_NUM_LEVELS] = {};
    const float* kern[VSLAM_NUM_LEVELS] = {};
    int kn[VSLAM_NUM_LEVELS] = {};
    template <class Levels>  // OrientLevels, SiftLevels
    void fill(Levels& lv) const {
        for (int l = 0; l < VSLAM_NUM_LEVELS; ++l) lv.gauss[l] = gauss[l], lv.kern[l] = kern[l], lv.kn[l] = kn[l];
    }
};
static int keypoint_levels(vslam_ctx* c, const vslam_pyramid* py, int octave, const vslam_point* kps, size_t n, int margin, const char* what,
                           KeypointLevels& kl) {
    const int rows = py->layout.rows[octave], cols = py->layout.cols[octave], pitch = py->layout.pitch[octave];
    for (size_t i = 0; i < n; ++i) {
        const vslam_point& k = kps[i];
        if (k.level < 0 || k.level >= VSLAM_NUM_LEVELS || k.octave != octave || k.col < -margin || k.row < -margin || k.col > cols + margin ||
            k.row > rows + margin)
            return fail(c, VSLAM_ERR_RANGE, std::string(what) + ": keypoint outside the octave's data");
        kl.used[k.level] = true;
    }
    for (int l = 0; l < VSLAM_NUM_LEVELS; ++l) {
        if (!kl.used[l]) continue;
        kl.gauss[l] = py->d_block + py->layout.octave_offset[octave] + (size_t)l * rows * pitch;
        TRY(get_orient_taps(c, 1.5 * py->info.sigma[octave][l], what, &kl.kern[l], &kl.kn[l]));
    }
    return VSLAM_OK;
}

// What OrientBatchGeom and SiftBatchGeom share, from (p, L): every octave's rows / cols / pitch / oct_off and, for the levels
// initialKeypointDetection produces (1 .. 3, Diff_of_Gauss.cpp:264), the taps of sigma = 1.5 * sigma(o, l) (:346, :616).
// Every other field is zeroed.
template <class Geom>
static int fill_batch_geom(vslam_ctx* c, const vslam_params& p, const vslam_batch_layout& L, Geom& g) {
    std::memset(&g, 0, sizeof(g));
    for (int o = 0; o < L.n_octaves; ++o) {
        g.rows[o] = L.rows[o];
        g.cols[o] = L.cols[o];
        g.pitch[o] = L.pitch[o];
        g.oct_off[o] = L.octave_offset[o];
        for (int l = 1; l <= 3; ++l) TRY(get_orient_taps(c, 1.5 * sigma_at(p.sigma0, o, l), "filterKeypoints", &g.kern[o][l], &g.kn[o][l]));
    }
    return VSLAM_OK;
}


extern "C" {

// ------------------------------------------------------------------------------ lifecycle

int vslam_ctx_create(int device, void* stream, vslam_ctx** out) {
    if (!out || device < 0) return VSLAM_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device >= n) return VSLAM_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return VSLAM_ERR_HIP;
    vslam_ctx* c = new (std::nothrow) vslam_ctx();
    if (!c) return VSLAM_ERR_NOMEM;
    c->device = device;
    if (stream == VSLAM_STREAM_LEGACY) {
        c->stream = nullptr;  // the NULL stream itself: every HIP call below takes it as "stream 0"
    } else if (stream) {
        c->stream = (hipStream_t)stream;
    } else if (own_stream(c, 0, &c->stream) != VSLAM_OK) {
        delete c;
        return VSLAM_ERR_HIP;
    }
    {
        const char* e = std::getenv("VSLAM_MX");
        c->mx = e && e[0] == '1';
        const char* ff = std::getenv("VSLAM_F32_FUSED");
        c->f32_fused = ff && ff[0] == '1';
        const char* es = VSLAM_DIAG_ENV("VSLAM_ORIENT_SCALAR");
        c->orient_scalar_form = es && es[0] == '1';
        sched_init_from_env(c);
    }
    *out = c;
    return VSLAM_OK;
}

int vslam_ctx_set_matrix_path(vslam_ctx* c, int on) {
    if (!c) return VSLAM_ERR_INVALID;
    c->mx = on != 0;
    return VSLAM_OK;
}

int vslam_ctx_get_matrix_path(const vslam_ctx* c) { return c && c->mx ? 1 : 0; }

int vslam_ctx_set_f32_fused(vslam_ctx* c, int on) {
    if (!c) return VSLAM_ERR_INVALID;
    c->f32_fused = on != 0;
    return VSLAM_OK;
}

int vslam_ctx_get_f32_fused(const vslam_ctx* c) { return c && c->f32_fused ? 1 : 0; }

int vslam_ctx_destroy(vslam_ctx* c) {
    if (!c) return VSLAM_ERR_INVALID;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    sched_destroy(c);  // every stream and event the context owns
    for (auto& kv : c->tables) (void)hipFree(kv.second);
    if (c->ws) (void)hipFree(c->ws);
    for (auto& b : c->block_cache) (void)hipFree(b.second);
    if (c->loc_lut) (void)hipFree(c->loc_lut);
    if (c->dump) (void)hipFree(c->dump);
    delete c;
    return VSLAM_OK;
}

int vslam_ctx_sync(vslam_ctx* c) {
    TRY(bind_device(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

const char* vslam_last_error(const vslam_ctx* c) { return c ? c->err.c_str() : "null context"; }
const char* vslam_kernel_names(void) { return kKernelNames; }


// ------------------------------------------------------------------- host-buffer primitives

int vslam_gaussian_blur_u8(vslam_ctx* c, const uint8_t* src, int rows, int cols, size_t step, int ksize,
                           double sigma, uint8_t* dst, size_t dst_step) {
    TRY(bind_device(c));
    ARGCHK(c, src && dst && rows > 0 && cols > 0 && step >= (size_t)cols && dst_step >= (size_t)cols, "blur: bad image");
    const int n = ksize > 0 ? ksize : (sigma > 0 ? gauss_ksize_u8(sigma) : -1);
    ARGCHK(c, n > 0 && (n & 1) && n <= VSLAM_MAX_KSIZE, "blur: kernel size must be odd (or 0 with sigma > 0)");
    const size_t P = (size_t)rows * cols;
    uint8_t *d_src, *d_dst;
    uint16_t* d_h;
    WsPlan ws;
    ws.add(d_src, P), ws.add(d_dst, P), ws.add(d_h, P);
    TRY(ws.commit(c));
    TRY(h2d(c, d_src, cols, src, step, cols, rows));
    TRY(enqueue_blur(c, d_src, cols, P, d_dst, cols, P, d_h, rows, cols, 1, n, sigma));
    TRY(d2h(c, dst, dst_step, d_dst, cols, cols, rows));
    return vslam_ctx_sync(c);
}

int vslam_sobel_k1_u8_f32(vslam_ctx* c, const uint8_t* src, int rows, int cols, size_t step, int dx, int dy,
                          float* dst, size_t dst_step) {
    TRY(bind_device(c));
    ARGCHK(c, src && dst && rows > 0 && cols > 0 && step >= (size_t)cols && dst_step >= 4 * (size_t)cols, "sobel: bad image");
    ARGCHK(c, (dx == 1 && dy == 0) || (dx == 0 && dy == 1), "sobel: (dx,dy) must be (1,0) or (0,1)");
    const size_t P = (size_t)rows * cols;
    uint8_t* d_src;
    float* d_dst;
    WsPlan ws;
    ws.add(d_src, P), ws.add(d_dst, P);
    TRY(ws.commit(c));
    TRY(h2d(c, d_src, cols, src, step, cols, rows));
    LAUNCH(c, "k_sobel_k1", k_sobel_k1, grid_rows(cols, rows), dim3(256), d_src, (size_t)cols, d_dst, (size_t)cols, rows,
           cols, dx);
    TRY(d2h(c, dst, dst_step, d_dst, 4 * (size_t)cols, 4 * (size_t)cols, rows));
    return vslam_ctx_sync(c);
}

int vslam_resize_linear2x_u8(vslam_ctx* c, const uint8_t* src, int rows, int cols, size_t step, uint8_t* dst,
                             size_t dst_step) {
    TRY(bind_device(c));
    ARGCHK(c, src && dst && rows > 0 && cols > 0 && step >= (size_t)cols && dst_step >= 2 * (size_t)cols, "resize2x: bad image");
    const size_t P = (size_t)rows * cols;
    uint8_t *d_src, *d_dst;
    WsPlan ws;
    ws.add(d_src, P), ws.add(d_dst, 4 * P);
    TRY(ws.commit(c));
    TRY(h2d(c, d_src, cols, src, step, cols, rows));
    if (cols % 4 == 0)
        LAUNCH(c, "k_resize_linear2x_slide", k_resize_linear2x_slide, dim3((cols / 4 + 255) / 256, (rows + 15) / 16, 1), dim3(256),
               d_src, (size_t)cols, P, d_dst, 4 * P, 2 * cols, rows, cols, 16);
    else
        LAUNCH(c, "k_resize_linear2x", k_resize_linear2x, grid_rows(2 * cols, 2 * rows), dim3(256), d_src, (size_t)cols, P,
               d_dst, (size_t)2 * cols, 4 * P, rows, cols);
    TRY(d2h(c, dst, dst_step, d_dst, 2 * (size_t)cols, 2 * (size_t)cols, 2 * (size_t)rows));
    return vslam_ctx_sync(c);
}

int vslam_resize_nearest_half_u8(vslam_ctx* c, const uint8_t* src, int rows, int cols, size_t step, uint8_t* dst,
                                 size_t dst_step) {
    TRY(bind_device(c));
    int dr, dc;
    half_size(rows, cols, &dr, &dc);
    ARGCHK(c, src && dst && rows > 0 && cols > 0 && dr > 0 && dc > 0 && step >= (size_t)cols && dst_step >= (size_t)dc,
           "resize half: bad image");
    const size_t P = (size_t)rows * cols, Q = (size_t)dr * dc;
    uint8_t *d_src, *d_dst;
    WsPlan ws;
    ws.add(d_src, P), ws.add(d_dst, Q);
    TRY(ws.commit(c));
    TRY(h2d(c, d_src, cols, src, step, cols, rows));
    LAUNCH(c, "k_resize_nearest_half", k_resize_nearest_half, grid_rows(dc, dr), dim3(256), d_src, (size_t)cols, P, d_dst,
           (size_t)dc, Q, rows, cols, dr, dc);
    TRY(d2h(c, dst, dst_step, d_dst, dc, dc, dr));
    return vslam_ctx_sync(c);
}

int vslam_convert_scale_abs_f32(vslam_ctx* c, const float* src, int rows, int cols, size_t step, uint8_t* dst,
                                size_t dst_step) {
    TRY(bind_device(c));
    ARGCHK(c, src && dst && rows > 0 && cols > 0 && step >= 4 * (size_t)cols && dst_step >= (size_t)cols, "convertScaleAbs: bad image");
    const size_t P = (size_t)rows * cols;
    float* d_src;
    uint8_t* d_dst;
    WsPlan ws;
    ws.add(d_src, P), ws.add(d_dst, P);
    TRY(ws.commit(c));
    TRY(h2d(c, d_src, 4 * (size_t)cols, src, step, 4 * (size_t)cols, rows));
    LAUNCH(c, "k_convert_scale_abs", k_convert_scale_abs, grid_rows(cols, rows), dim3(256), d_src, (size_t)cols, d_dst,
           (size_t)cols, rows, cols);
    TRY(d2h(c, dst, dst_step, d_dst, cols, cols, rows));
    return vslam_ctx_sync(c);
}

// -------------------------------------------------------------------------------- Harris

int vslam_harris_from_grad_f32(vslam_ctx* c, const float* ix, const float* iy, int rows, int cols, size_t step,
                               float k, int window, float* resp, size_t resp_step) {
    TRY(bind_device(c));
    ARGCHK(c, ix && iy && resp && rows > 0 && cols > 0 && step >= 4 * (size_t)cols && resp_step >= 4 * (size_t)cols,
           "HarrisCorner: bad image");
    ARGCHK(c, window >= 1 && (window & 1), "HarrisCorner: window must be odd");
    const size_t P = (size_t)rows * cols, rb = 4 * (size_t)cols;
    float *d_ix, *d_iy, *d_r;
    WsPlan ws;
    ws.add(d_ix, P), ws.add(d_iy, P), ws.add(d_r, P);
    TRY(ws.commit(c));
    TRY(h2d(c, d_ix, rb, ix, step, rb, rows));
    TRY(h2d(c, d_iy, rb, iy, step, rb, rows));
    LAUNCH(c, "k_harris_from_grad", k_harris_from_grad, grid_rows(cols, rows), dim3(256), d_ix, d_iy, (size_t)cols, rows,
           cols, k, (window - 1) / 2, d_r, (size_t)cols);
    TRY(d2h(c, resp, resp_step, d_r, rb, rb, rows));
    return vslam_ctx_sync(c);
}

int vslam_harris_response_u8(vslam_ctx* c, const uint8_t* img, int rows, int cols, size_t step, float k, int window,
                             float* resp, size_t resp_step) {
    TRY(bind_device(c));
    ARGCHK(c, img && resp && rows > 0 && cols > 0 && step >= (size_t)cols && resp_step >= 4 * (size_t)cols,
           "harris_response: bad image");
    if (window != 3) return fail(c, VSLAM_ERR_UNSUPPORTED, "harris_response: fused kernel implements windowSize 3 (Harris_corners.cpp:34); use the per-stage entry points for other windows");
    const size_t P = (size_t)rows * cols;
    uint8_t* d_img;
    float* d_r;
    WsPlan ws;
    ws.add(d_img, P), ws.add(d_r, P);
    TRY(ws.commit(c));
    TRY(h2d(c, d_img, cols, img, step, cols, rows));
    TRY(enqueue_harris(c, d_img, P, rows, cols, 1, k, d_r, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
    TRY(d2h(c, resp, resp_step, d_r, 4 * (size_t)cols, 4 * (size_t)cols, rows));
    return vslam_ctx_sync(c);
}

static int nms_strict_common(vslam_ctx* c, const void* src, int elem, int rows, int cols, size_t step, int window,
                             uint8_t* mask, size_t mask_step) {
    TRY(bind_device(c));
    ARGCHK(c, src && mask && rows > 0 && cols > 0 && step >= (size_t)elem * cols && mask_step >= (size_t)cols, "NonMaximumSuppression: bad image");
    ARGCHK(c, window >= 1 && (window & 1), "NonMaximumSuppression: windowSize must be odd");
    const size_t P = (size_t)rows * cols, rb = (size_t)elem * cols;
    char* d_src;
    uint8_t* d_m;
    WsPlan ws;
    ws.add(d_src, elem * P), ws.add(d_m, P);
    TRY(ws.commit(c));
    TRY(h2d(c, d_src, rb, src, step, rb, rows));
    const int p = (window - 1) / 2;
    if (elem == 1)
        LAUNCH(c, "k_nms_strict_generic", k_nms_strict_generic<uint8_t>, grid_rows(cols, rows), dim3(256),
               (const uint8_t*)d_src, (size_t)cols, rows, cols, p, d_m, (size_t)cols);
    else
        LAUNCH(c, "k_nms_strict_generic", k_nms_strict_generic<float>, grid_rows(cols, rows), dim3(256),
               (const float*)d_src, (size_t)cols, rows, cols, p, d_m, (size_t)cols);
    TRY(d2h(c, mask, mask_step, d_m, cols, cols, rows));
    return vslam_ctx_sync(c);
}

int vslam_nms_strict_u8(vslam_ctx* c, const uint8_t* src, int rows, int cols, size_t step, int window, uint8_t* mask,
                        size_t mask_step) {
    return nms_strict_common(c, src, 1, rows, cols, step, window, mask, mask_step);
}
int vslam_nms_strict_f32(vslam_ctx* c, const float* src, int rows, int cols, size_t step, int window, uint8_t* mask,
                         size_t mask_step) {
    return nms_strict_common(c, src, 4, rows, cols, step, window, mask, mask_step);
}

int vslam_nms2_f32(vslam_ctx* c, const float* resp, int rows, int cols, size_t step, int window, float* out,
                   size_t out_step, float* true_max) {
    TRY(bind_device(c));
    ARGCHK(c, resp && out && rows > 0 && cols > 0 && step >= 4 * (size_t)cols && out_step >= 4 * (size_t)cols && window >= 1,
           "NMS2: bad arguments");
    const size_t P = (size_t)rows * cols, rb = 4 * (size_t)cols;
    float *d_r, *d_o;
    unsigned int* d_max;
    WsPlan ws;
    ws.add(d_r, P), ws.add(d_o, P), ws.add(d_max, 1);
    TRY(ws.commit(c));
    TRY(h2d(c, d_r, rb, resp, step, rb, rows));
    HIPCHK(c, hipMemsetAsync(d_max, 0, 4, c->stream));
    LAUNCH(c, "k_nms2_generic", k_nms2_generic, grid_rows(cols, rows), dim3(256), d_r, (size_t)cols, rows, cols,
           (window - 1) / 2, d_o, (size_t)cols, d_max);
    TRY(d2h(c, out, out_step, d_o, rb, rb, rows));
    unsigned int bits = 0;
    HIPCHK(c, hipMemcpyAsync(&bits, d_max, 4, hipMemcpyDeviceToHost, c->stream));
    TRY(vslam_ctx_sync(c));
    if (true_max) std::memcpy(true_max, &bits, 4);
    return VSLAM_OK;
}

int vslam_harris_keypoints_u8(vslam_ctx* c, const uint8_t* img, int rows, int cols, size_t step, float k,
                              vslam_kp* out, size_t cap, size_t* count) {
    TRY(bind_device(c));
    ARGCHK(c, img && count && rows > 0 && cols > 0 && step >= (size_t)cols && (out || cap == 0), "harris_keypoints: bad arguments");
    const size_t P = (size_t)rows * cols;
    const unsigned int dcap = (unsigned int)std::min<size_t>(cap, 0x7fffffff);
    uint8_t* d_img;
    float* d_r;
    unsigned long long* d_f;
    vslam_kp* d_k;
    unsigned int *d_n, *d_cws;
    WsPlan ws;
    ws.add(d_img, P), ws.add(d_r, P), ws.add(d_f, harris_flag_words(rows, cols)), ws.add(d_k, dcap), ws.add(d_n, 1);
    ws.add(d_cws, compaction_ws_elems(harris_flag_words(rows, cols), 1));
    TRY(ws.commit(c));
    TRY(h2d(c, d_img, cols, img, step, cols, rows));
    TRY(enqueue_harris(c, d_img, P, rows, cols, 1, k, d_r, nullptr, nullptr, d_f, d_k, dcap, d_n, d_cws));
    return read_list(c, d_n, d_k, dcap, out, count);
}

// ------------------------------------------------------------------------------ DoG pyramid

int vslam_pyramid_build_u8(vslam_ctx* c, const uint8_t* img, int rows, int cols, size_t step, int n_octaves,
                           double sigma0, vslam_pyramid** out) {
    TRY(bind_device(c));
    ARGCHK(c, img && out && rows > 0 && cols > 0 && step >= (size_t)cols && sigma0 > 0, "GaussPyramid: bad arguments");
    *out = nullptr;
    if (n_octaves <= 0) n_octaves = auto_num_octaves(rows, cols);  // GaussPyramid.hpp:18-21
    ARGCHK(c, n_octaves >= 1 && n_octaves <= VSLAM_MAX_OCTAVES, "GaussPyramid: octave count out of range");
    vslam_params p;
    vslam_params_default(&p, rows, cols);
    p.n_octaves = n_octaves;
    p.sigma0 = sigma0;
    vslam_batch_layout L;
    if (make_layout(&p, &L) != VSLAM_OK) return fail(c, VSLAM_ERR_INVALID, "GaussPyramid: image too small for the octave count");
    vslam_pyramid* py = new (std::nothrow) vslam_pyramid();
    if (!py) return fail(c, VSLAM_ERR_NOMEM, "host allocation failed");
    py->ctx = c;
    py->params = p;
    py->layout = L;
    py->info.n_octaves = n_octaves;
    py->info.n_levels = VSLAM_NUM_LEVELS;
    py->info.n_dogs = VSLAM_NUM_DOGS;
    py->info.sigma0 = sigma0;
    size_t sum_p = 0;
    for (int o = 0; o < n_octaves; ++o) {
        py->info.rows[o] = L.rows[o];
        py->info.cols[o] = L.cols[o];
        py->base_off[o] = sum_p;
        sum_p += (size_t)L.rows[o] * L.pitch[o];
        for (int l = 0; l < VSLAM_NUM_LEVELS; ++l) {
            py->info.sigma[o][l] = sigma_at(sigma0, o, l);
            py->info.ksize[o][l] = gauss_ksize_u8(py->info.sigma[o][l]);
        }
    }
    auto cleanup = [&](int rc) {
        vslam_pyramid_destroy(py);
        return rc;
    };
    py->d_block = (uint8_t*)block_alloc(c, L.pyramid_frame_bytes, &py->block_cap);
    py->d_bases = (uint8_t*)block_alloc(c, sum_p, &py->bases_cap);
    if (!py->d_block || !py->d_bases) return cleanup(fail(c, VSLAM_ERR_NOMEM, "device allocation failed (pyramid)"));
    const size_t N = (size_t)rows * cols;
    const std::vector<OctPlan> plans = plan_octaves(sigma0, L);
    uint8_t* d_img;
    DogScratch s;
    WsPlan ws;
    ws.add(d_img, N);
    dog_scratch_plan(ws, L, plans, 1, s);
    int rc = ws.commit(c);
    if (rc) return cleanup(rc);
    if ((rc = h2d(c, d_img, cols, img, step, cols, rows))) return cleanup(rc);
    // the batched path's chunk with everything on the context's stream: no side lanes, no Harris chain, no lists
    DogChunk d{p, L, plans, d_img, (size_t)cols, N, 1, s, DogOut{py->d_block, L.pyramid_frame_bytes}, batch_plan(batch_plan_input(c, p, L, plans, cols))};
    if ((rc = enqueue_dog(c, d))) return cleanup(rc);
    if (hipMemcpyAsync(py->d_bases, s.bases, sum_p, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
        return cleanup(fail(c, VSLAM_ERR_HIP, "device copy failed (bases)"));
    if ((rc = vslam_ctx_sync(c))) return cleanup(rc);
    *out = py;
    return VSLAM_OK;
}

int vslam_pyramid_destroy(vslam_pyramid* py) {
    if (!py) return VSLAM_ERR_INVALID;
    if (py->ctx) (void)hipSetDevice(py->ctx->device);
    block_release(py->ctx, py->d_block, py->block_cap);
    block_release(py->ctx, py->d_bases, py->bases_cap);
    delete py;
    return VSLAM_OK;
}

int vslam_pyramid_get_info(const vslam_pyramid* py, vslam_pyramid_info* out) {
    if (!py || !out) return VSLAM_ERR_INVALID;
    *out = py->info;
    return VSLAM_OK;
}

static int pyramid_fetch(const vslam_pyramid* py, int octave, const uint8_t* d_src, uint8_t* dst, size_t dst_step) {
    vslam_ctx* c = py->ctx;
    TRY(bind_device(c));
    const int rows = py->layout.rows[octave], cols = py->layout.cols[octave], pitch = py->layout.pitch[octave];
    ARGCHK(c, dst && dst_step >= (size_t)cols, "pyramid getter: bad destination");
    if (pitch != cols) {  // pitched plane: pack the rows on the device, then one linear copy
        const size_t P = (size_t)rows * cols;
        uint8_t* d_dense;
        WsPlan ws;
        ws.add(d_dense, P);
        TRY(ws.commit(c));
        LAUNCH(c, "k_pack_rows", k_pack_rows, grid_rows(cols, rows), dim3(256), d_src, pitch, d_dense, rows, cols);
        d_src = d_dense;
    }
    TRY(d2h(c, dst, dst_step, d_src, cols, cols, rows));
    return vslam_ctx_sync(c);
}

int vslam_pyramid_get_base(const vslam_pyramid* py, int octave, uint8_t* dst, size_t dst_step) {
    if (!py) return VSLAM_ERR_INVALID;
    if (octave < 0 || octave >= py->layout.n_octaves) return fail(py->ctx, VSLAM_ERR_RANGE, "octave out of range");
    return pyramid_fetch(py, octave, py->d_bases + py->base_off[octave], dst, dst_step);
}

int vslam_pyramid_get_gauss(const vslam_pyramid* py, int octave, int level, uint8_t* dst, size_t dst_step) {
    if (!py) return VSLAM_ERR_INVALID;
    if (octave < 0 || octave >= py->layout.n_octaves || level < 0 || level >= VSLAM_NUM_LEVELS)
        return fail(py->ctx, VSLAM_ERR_RANGE, "octave/level out of range");
    const size_t P = (size_t)py->layout.rows[octave] * py->layout.pitch[octave];
    return pyramid_fetch(py, octave, py->d_block + py->layout.octave_offset[octave] + (size_t)level * P, dst, dst_step);
}

int vslam_pyramid_get_dog(const vslam_pyramid* py, int octave, int level, uint8_t* dst, size_t dst_step) {
    if (!py) return VSLAM_ERR_INVALID;
    if (octave < 0 || octave >= py->layout.n_octaves || level < 0 || level >= VSLAM_NUM_DOGS)
        return fail(py->ctx, VSLAM_ERR_RANGE, "octave/level out of range");
    const size_t P = (size_t)py->layout.rows[octave] * py->layout.pitch[octave];
    return pyramid_fetch(py, octave,
                         py->d_block + py->layout.octave_offset[octave] + (size_t)(VSLAM_NUM_LEVELS + level) * P, dst,
                         dst_step);
}

int vslam_pyramid_get_gradients(const vslam_pyramid* py, int octave, int level, float* grad_x, float* grad_y, float* mag,
                                float* orient, size_t dst_step) {
    if (!py) return VSLAM_ERR_INVALID;
    vslam_ctx* c = py->ctx;
    TRY(bind_device(c));
    if (octave < 0 || octave >= py->layout.n_octaves || level < 0 || level >= VSLAM_NUM_LEVELS)
        return fail(c, VSLAM_ERR_RANGE, "octave/level out of range");
    const int rows = py->layout.rows[octave], cols = py->layout.cols[octave];
    ARGCHK(c, dst_step >= 4 * (size_t)cols, "pyramid gradients: bad destination step");
    float* host[4] = {grad_x, grad_y, mag, orient};
    const size_t P = (size_t)rows * cols;
    float* dev[4];
    WsPlan ws;
    for (int i = 0; i < 4; ++i) ws.add(dev[i], P);
    TRY(ws.commit(c));
    for (int i = 0; i < 4; ++i)
        if (!host[i]) dev[i] = nullptr;
    const int pitch = py->layout.pitch[octave];
    const uint8_t* g = py->d_block + py->layout.octave_offset[octave] + (size_t)level * rows * pitch;
    LAUNCH(c, "k_level_gradients", F32_KERNEL(c, k_level_gradients), grid_rows(cols, rows), dim3(256), g, pitch, rows, cols, dev[0], dev[1], dev[2], dev[3]);
    for (int i = 0; i < 4; ++i)
        if (host[i]) TRY(d2h(c, host[i], dst_step, dev[i], 4 * (size_t)cols, 4 * (size_t)cols, rows));
    return vslam_ctx_sync(c);
}

static int dog_points_host(vslam_ctx* c, const vslam_pyramid* py, int octave, int window, int min_contrast, int localize,
                           uint64_t* bits, vslam_point* out, size_t cap, size_t* count) {
    TRY(bind_device(c));
    ARGCHK(c, py && py->ctx == c && count && (out || cap == 0), "initialKeypointDetection: bad arguments");
    if (octave < 0 || octave >= py->layout.n_octaves) return fail(c, VSLAM_ERR_RANGE, "octave out of range");
    ARGCHK(c, window >= 3 && (window & 1), "initialKeypointDetection: windowSize must be odd and >= 3");
    vslam_params p = py->params;
    p.extrema_window = window;
    p.min_contrast = min_contrast;
    p.localize = localize;
    p.dog_cap = (uint32_t)std::min<size_t>(cap, 0x7fffffff);
    vslam_batch_layout L;
    if (make_layout(&p, &L) != VSLAM_OK) return fail(c, VSLAM_ERR_INVALID, "bad extrema parameters");
    ExtGeom g;
    if (p.localize) TRY(ensure_loc_lut(c));
    fill_geom(c, p, L, g);
    const size_t words = L.bits_frame_words;
    unsigned long long *d_bits, *d_lf;
    vslam_point* d_pts;
    unsigned int *d_n, *d_cws;
    WsPlan ws;
    ws.add(d_bits, words), ws.add(d_lf, words), ws.add(d_pts, p.dog_cap), ws.add(d_n, 1), ws.add(d_cws, compaction_ws_elems(words, 1));
    TRY(ws.commit(c));
    HIPCHK(c, hipMemsetAsync(d_n, 0, 4, c->stream));
    const size_t ow = (size_t)3 * L.lat_rows[octave] * L.lat_words[octave];
    if (ow) {
        if (window == 3) {
            const dim3 eg((L.lat_words[octave] + 3) / 4, L.lat_rows[octave], 1);
            if (localize)
                LAUNCH(c, "k_extrema_w3", k_extrema_w3<true>, eg, dim3(256), py->d_block, L.pyramid_frame_bytes, g, octave, d_bits, d_lf, words, 0, 1);
            else
                LAUNCH(c, "k_extrema_w3", k_extrema_w3<false>, eg, dim3(256), py->d_block, L.pyramid_frame_bytes, g, octave, d_bits, d_lf, words, 0, 1);
        } else {
            LAUNCH(c, "k_extrema", k_extrema, dim3((L.lat_cols[octave] + 255) / 256, L.lat_rows[octave], 3), dim3(256),
                   py->d_block, L.pyramid_frame_bytes, g, octave, d_bits, d_lf, words);
        }
        DogEntries ent{d_lf, words, py->d_block, L.pyramid_frame_bytes, g, octave, octave + 1, d_pts};
        TRY(enqueue_compaction(c, ent, ow, 1, d_cws, p.dog_cap, d_n, 0));
    }
    return read_list(c, d_n, d_pts, p.dog_cap, out, count, bits, d_bits + L.bits_offset[octave], bits ? ow * 8 : 0);
}

int vslam_dog_extrema(vslam_ctx* c, const vslam_pyramid* py, int octave, int window, int min_contrast, uint64_t* bits,
                      vslam_point* out, size_t cap, size_t* count) {
    return dog_points_host(c, py, octave, window, min_contrast, 0, bits, out, cap, count);
}

int vslam_dog_extrema_dense(vslam_ctx* c, const vslam_pyramid* py, int octave, int min_contrast, uint64_t* bits,
                            vslam_point* out, size_t cap, size_t* count) {
    TRY(bind_device(c));
    ARGCHK(c, py && py->ctx == c && count && (out || cap == 0), "dense extrema: bad arguments");
    if (octave < 0 || octave >= py->layout.n_octaves) return fail(c, VSLAM_ERR_RANGE, "octave out of range");
    ARGCHK(c, min_contrast >= 0 && min_contrast <= 65535, "dense extrema: min_contrast out of range");
    const vslam_batch_layout& L = py->layout;
    DenseGeom g = dense_geom(L, octave, min_contrast, 1);
    const size_t words = (size_t)3 * g.rows * g.wpr;
    const unsigned int ocap = (unsigned int)std::min<size_t>(cap, 0x7fffffff);
    unsigned long long *d_bits, *d_lf;
    vslam_point* d_pts;
    unsigned int *d_n, *d_cws;
    WsPlan ws;
    ws.add(d_bits, words), ws.add(d_lf, words), ws.add(d_pts, ocap), ws.add(d_n, 1), ws.add(d_cws, compaction_ws_elems(words, 1));
    TRY(ws.commit(c));
    HIPCHK(c, hipMemsetAsync(d_n, 0, 4, c->stream));
    LAUNCH(c, "k_extrema_dense", k_extrema_dense, dim3(((g.cols + 3) / 4 + 255) / 256, (g.rows + g.seg - 1) / g.seg, 1), dim3(256),
           py->d_block, L.pyramid_frame_bytes, g, bits ? d_bits : nullptr, d_lf, words);
    DenseDogEntries ent{d_lf, words, py->d_block, L.pyramid_frame_bytes, g, octave, d_pts};
    TRY(enqueue_compaction(c, ent, words, 1, d_cws, ocap, d_n, 0));
    return read_list(c, d_n, d_pts, ocap, out, count, bits, d_bits, bits ? words * 8 : 0);
}

int vslam_dog_keypoints(vslam_ctx* c, const vslam_pyramid* py, int octave, int window, vslam_point* out, size_t cap,
                        size_t* count) {
    return dog_points_host(c, py, octave, window, 0, 1, nullptr, out, cap, count);
}

int vslam_localize_points(vslam_ctx* c, const int* diffs, size_t n, int* keep, int* value) {
    TRY(bind_device(c));
    ARGCHK(c, (diffs && keep && value) || n == 0, "FeaturePointLocalization: bad arguments");
    ARGCHK(c, n <= 0x7fffffff, "FeaturePointLocalization: too many points");
    if (n == 0) return VSLAM_OK;
    int4* d_in;
    int2* d_out;
    WsPlan ws;
    ws.add(d_in, n), ws.add(d_out, n);
    TRY(ws.commit(c));
    HIPCHK(c, hipMemcpyAsync(d_in, diffs, 16 * n, hipMemcpyHostToDevice, c->stream));
    TRY(ensure_loc_lut(c));  // same path as the fused kernels: table for small differences, closed form otherwise
    LAUNCH(c, "k_localize_points", k_localize_points, dim3((unsigned)((n + 255) / 256)), dim3(256), d_in, (int)n, d_out, c->loc_lut);
    std::vector<int2> h(n);
    HIPCHK(c, hipMemcpyAsync(h.data(), d_out, 8 * n, hipMemcpyDeviceToHost, c->stream));
    TRY(vslam_ctx_sync(c));
    for (size_t i = 0; i < n; ++i) keep[i] = h[i].x, value[i] = h[i].y;
    return VSLAM_OK;
}

int vslam_filter_keypoints(vslam_ctx* c, const vslam_pyramid* py, int octave, const vslam_point* kps, size_t n,
                           vslam_point* out, size_t cap, size_t* count) {
    TRY(bind_device(c));
    ARGCHK(c, py && py->ctx == c && count && (kps || n == 0) && (out || cap == 0), "filterKeypoints: bad arguments");
    if (octave < 0 || octave >= py->layout.n_octaves) return fail(c, VSLAM_ERR_RANGE, "octave out of range");
    ARGCHK(c, n <= 0x7fffffff, "filterKeypoints: too many keypoints");
    *count = 0;
    if (n == 0) return VSLAM_OK;
    const int rows = py->layout.rows[octave], cols = py->layout.cols[octave], pitch = py->layout.pitch[octave];
    const size_t P = (size_t)rows * cols;  // dense f32 scratch images
    KeypointLevels kl;
    TRY(keypoint_levels(c, py, octave, kps, n, 0, "filterKeypoints", kl));
    int max_r = 0;
    for (int l = 0; l < VSLAM_NUM_LEVELS; ++l) max_r = std::max(max_r, kl.kn[l] / 2);
    const size_t lds = orient_lds_bytes(max_r);
    if (lds > 150 * 1024) return fail(c, VSLAM_ERR_UNSUPPORTED, "filterKeypoints: blur kernel too wide for the LDS strip");
    const unsigned int ocap = (unsigned int)std::min<size_t>(cap, 0x7fffffff);
    vslam_point *d_kps, *d_out;
    unsigned long long* d_masks;
    unsigned int *d_n, *d_cws;
    float *d_mag[VSLAM_NUM_LEVELS], *d_ori[VSLAM_NUM_LEVELS];
    WsPlan ws;
    ws.add(d_kps, n), ws.add(d_masks, n), ws.add(d_out, ocap), ws.add(d_n, 1), ws.add(d_cws, compaction_ws_elems(n, 1));
    for (int l = 0; l < VSLAM_NUM_LEVELS; ++l)
        if (kl.used[l]) ws.add(d_mag[l], P), ws.add(d_ori[l], P);
    TRY(ws.commit(c));
    OrientLevels lv{};
    kl.fill(lv);
    HIPCHK(c, hipMemcpyAsync(d_kps, kps, sizeof(vslam_point) * n, hipMemcpyHostToDevice, c->stream));
    for (int l = 0; l < VSLAM_NUM_LEVELS; ++l) {
        if (!kl.used[l]) continue;
        // processGradients for the level (GaussPyramid.cpp:65-104): magnitude and orientation only
        // (the orientation image is only BINNED here: no bin depends on the arctangent's variant, kernels_aux.hip.h)
        LAUNCH(c, "k_level_gradients", k_level_gradients<false>, grid_rows(cols, rows), dim3(256), kl.gauss[l], pitch, rows, cols, (float*)nullptr,
               (float*)nullptr, d_mag[l], d_ori[l]);
        lv.mag[l] = d_mag[l];
        lv.orient[l] = d_ori[l];
    }
    const auto k_orient = F32_KERNEL(c, k_orient_keypoints);
    TRY(raise_dyn_lds(c, reinterpret_cast<const void*>(k_orient)));
    LAUNCH_ON(c, "k_orient_keypoints", -1, c->stream, lds, k_orient, dim3((unsigned)n), dim3(256), d_kps, (int)n, lv, pitch, rows, cols, d_masks);
    OrientEntries ent{d_masks, d_kps, n, d_out};
    TRY(enqueue_compaction(c, ent, n, 1, d_cws, ocap, d_n, 0));
    return read_list(c, d_n, d_out, ocap, out, count);
}

int vslam_sift_descriptors(vslam_ctx* c, const vslam_pyramid* py, int octave, const vslam_point* kps, size_t n, float* desc,
                           uint8_t* defined) {
    TRY(bind_device(c));
    ARGCHK(c, py && py->ctx == c && (kps || n == 0) && (desc || n == 0), "SIFT: bad arguments");
    if (octave < 0 || octave >= py->layout.n_octaves) return fail(c, VSLAM_ERR_RANGE, "octave out of range");
    ARGCHK(c, n <= 0x7fffffff / 128, "SIFT: too many keypoints");
    if (n == 0) return VSLAM_OK;
    const int rows = py->layout.rows[octave], cols = py->layout.cols[octave], pitch = py->layout.pitch[octave];
    KeypointLevels kl;
    TRY(keypoint_levels(c, py, octave, kps, n, SIFT_PAD, "SIFT", kl));
    std::vector<float2> cs(n);
    for (size_t i = 0; i < n; ++i) vslam_cos_sin_deg((float)kps[i].value, &cs[i].x, &cs[i].y);  // keypoint.value holds the angle in degrees (:594)
    vslam_point* d_kps;
    float2* d_cs;
    float* d_desc;
    uint8_t* d_def;
    WsPlan ws;
    ws.add(d_kps, n), ws.add(d_cs, n), ws.add(d_desc, 128 * n), ws.add(d_def, n);
    TRY(ws.commit(c));
    HIPCHK(c, hipMemcpyAsync(d_kps, kps, sizeof(vslam_point) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_cs, cs.data(), sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    SiftLevels lv{};
    kl.fill(lv);
    LAUNCH(c, "k_sift_descriptors", F32_KERNEL(c, k_sift_descriptors), dim3((unsigned)n), dim3(256), d_kps, d_cs, (int)n, lv, pitch, rows, cols, d_desc, d_def);
    std::vector<uint8_t> h_def(n);
    HIPCHK(c, hipMemcpyAsync(desc, d_desc, sizeof(float) * 128 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_def.data(), d_def, n, hipMemcpyDeviceToHost, c->stream));
    TRY(vslam_ctx_sync(c));
    size_t undefined = 0;
    for (size_t i = 0; i < n; ++i) undefined += h_def[i] == 0;
    if (defined) std::memcpy(defined, h_def.data(), n);
    if (undefined && !defined)
        return fail(c, VSLAM_ERR_RANGE, "SIFT: " + std::to_string(undefined) + " keypoint window(s) leave the padded level (undefined in the reference)");
    return VSLAM_OK;
}

static int gradient_windows(vslam_ctx* c, const float* gx_windows, const float* gy_windows, int window_elems, size_t n, float* sums,
                            float* response, const char* what) {
    TRY(bind_device(c));
    ARGCHK(c, window_elems >= 0 && ((gx_windows && gy_windows) || window_elems == 0 || n == 0) && (sums || response || n == 0), what);
    ARGCHK(c, n <= 0x7fffffff / 3, what);
    if (n == 0) return VSLAM_OK;
    const size_t we = (size_t)window_elems * n;
    float *d_gx, *d_gy, *d_s, *d_r;
    WsPlan ws;
    ws.add(d_gx, we + 1), ws.add(d_gy, we + 1), ws.add(d_s, 3 * n), ws.add(d_r, n);
    TRY(ws.commit(c));
    if (we) {
        HIPCHK(c, hipMemcpyAsync(d_gx, gx_windows, 4 * we, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_gy, gy_windows, 4 * we, hipMemcpyHostToDevice, c->stream));
    }
    LAUNCH(c, "k_edge_response_windows", k_edge_response_windows, dim3((unsigned)((n + 255) / 256)), dim3(256), d_gx, d_gy, window_elems, (int)n,
           sums ? d_s : (float*)nullptr, response ? d_r : (float*)nullptr);
    if (sums) HIPCHK(c, hipMemcpyAsync(sums, d_s, 12 * n, hipMemcpyDeviceToHost, c->stream));
    if (response) HIPCHK(c, hipMemcpyAsync(response, d_r, 4 * n, hipMemcpyDeviceToHost, c->stream));
    return vslam_ctx_sync(c);
}

int vslam_edge_response_windows(vslam_ctx* c, const float* gx_windows, const float* gy_windows, int window_elems, size_t n,
                                float* response) {
    return gradient_windows(c, gx_windows, gy_windows, window_elems, n, nullptr, response, "computeEdgeResponse: bad arguments");
}

int vslam_structure_matrix_windows(vslam_ctx* c, const float* gx_windows, const float* gy_windows, int window_elems, size_t n,
                                   float* sums) {
    return gradient_windows(c, gx_windows, gy_windows, window_elems, n, sums, nullptr, "StructureMatrix: bad arguments");
}

// ------------------------------------------------------------- device-resident batched path

struct OrientScratch {
    unsigned long long* flags = nullptr;  // [nf][fwords] edge-test ballots
    unsigned int* surv = nullptr;         // [nf][scap] surviving record indices
    unsigned int* scounts = nullptr;      // [nf]
    unsigned long long* masks = nullptr;  // [nf][scap] histogram-peak masks
    unsigned int* cws = nullptr;          // compaction scratch
    unsigned int* obegin = nullptr;       // [nf] list length after octave 0 (the early edge-test launch covers [0, obegin))
    unsigned int* ranges = nullptr;       // [nf][OR_RANGE_STRIDE] first survivor of each octave, of each (octave, level) (k_survivor_ranges)
    size_t fwords = 0;
};
static void orient_scratch_plan(WsPlan& ws, const vslam_params& p, int nf, OrientScratch& s) {
    s.fwords = ((size_t)p.dog_cap + 63) / 64;
    const size_t scap = p.oriented_cap;
    ws.add(s.flags, (size_t)nf * s.fwords);
    ws.add(s.surv, (size_t)nf * scap);
    ws.add(s.scounts, nf);
    ws.add(s.obegin, nf);
    ws.add(s.ranges, (size_t)nf * OR_RANGE_STRIDE);
    ws.add(s.masks, (size_t)nf * scap);
    ws.add(s.cws, compaction_ws_elems(std::max(s.fwords, scap), nf));
}

// Geometry / blur taps of the batched filterKeypoints and the LDS budget of each octave's launch.
struct OrientPlan {
    OrientBatchGeom g;
    int need[VSLAM_MAX_OCTAVES] = {};  // LDS floats of octave o's launch of k_orient_survivors
    int smax[VSLAM_MAX_OCTAVES] = {};  // largest span (16 + 2 R) of the octave's levels: <= OR_PK_MAX_SPAN -> k_orient_survivors_pk
};
static int make_orient_plan(vslam_ctx* c, const vslam_params& p, const vslam_batch_layout& L, OrientPlan& pl) {
    OrientBatchGeom& g = pl.g;
    TRY(fill_batch_geom(c, p, L, g));
    g.n_oct = L.n_octaves;
    constexpr int kBigLds = 36 * 1024;  // floats: 144 KB
    for (int o = 0; o < L.n_octaves; ++o) {
        int worst = 0, strip = 0;
        for (int l = 1; l <= 3; ++l) {
            const int span = OR_WIN + 2 * (g.kn[o][l] / 2);
            // maps + taps + strip + region + the u8 patch of interior survivors (k_orient_survivors)
            worst = std::max(worst, 3 * span + span * OR_WIN + span * span + (span + 2) * ((span + 8) >> 2));
            strip = std::max(strip, span * (OR_WIN + 3));
            pl.smax[o] = std::max(pl.smax[o], span);
        }
        // regions that exceed even the big budget are read tap by tap; the strip, the maps and the taps still need room
        pl.need[o] = worst <= kBigLds ? worst : std::max(strip, std::min(worst, kBigLds));
    }
    return VSLAM_OK;
}

// The edge test (Diff_of_Gauss.cpp:331-335) for the records octave 0 has appended.  Called on the stream
// the list is written on, right behind that octave's compaction (`counts` is then the list length after
// octave 0); the kernel itself goes to `other` (the Harris chain's stream, idle by then) so that it runs
// beside the next octaves' scans instead of between them - when the plan forks it (BatchPlan::early_edge_forked).
static int enqueue_edge_flags_early(vslam_ctx* c, const vslam_params& p, const OrientPlan& pl, int nf, const uint8_t* pyr, size_t pframe,
                                    const vslam_point* points, const unsigned int* counts, const OrientScratch& s, bool fork) {
    const hipStream_t other = lane_stream(c, Lane::Harris);
    HIPCHK(c, hipMemcpyAsync(s.obegin, counts, sizeof(unsigned int) * (size_t)nf, hipMemcpyDeviceToDevice, c->stream));
    if (fork) {
        HIPCHK(c, hipEventRecord(c->ev_list0, c->stream));
        HIPCHK(c, hipStreamWaitEvent(other, c->ev_list0, 0));
    }
    {
        StreamSwap sw(c, fork ? other : c->stream);
        LAUNCH(c, "k_edge_flags", k_edge_flags, dim3((unsigned)((s.fwords * 64 + 255) / 256), nf), dim3(256), points, (const unsigned int*)nullptr,
               (const unsigned int*)s.obegin, p.dog_cap, pyr, pframe, pl.g, s.flags, s.fwords);
        if (fork) HIPCHK(c, hipEventRecord(c->ev_edge, c->stream));
    }
    return VSLAM_OK;
}

// filterKeypoints for the keypoint lists of nf frames (kernels_orient_batch.hip.h), on the
// context's current stream; the lists must be complete on that stream.  `plan`: whether the early edge test has run for
// this chunk and on which lane, and whether the per-octave launches spread over the idle side lanes.
static int enqueue_orient_batch(vslam_ctx* c, const vslam_params& p, const vslam_batch_layout& L, const OrientPlan& pl, int nf, const uint8_t* pyr,
                                size_t pframe, const vslam_point* points, const unsigned int* counts, const OrientScratch& s,
                                vslam_point* oriented, unsigned int* oriented_counts, const BatchPlan& plan) {
    const OrientBatchGeom& g = pl.g;
    const size_t scap = p.oriented_cap;
    const size_t fw = s.fwords;
    if (plan.early_edge_forked) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_edge, 0));  // the two launches share a flag word
    LAUNCH(c, "k_edge_flags", k_edge_flags, dim3((unsigned)((fw * 64 + 255) / 256), nf), dim3(256), points,
           (const unsigned int*)(plan.early_edge ? s.obegin : nullptr), counts, p.dog_cap, pyr, pframe, g, s.flags, fw);
    SurvivorEntries se{s.flags, fw, s.surv};
    TRY(enqueue_compaction(c, se, fw, nf, s.cws, (unsigned int)scap, s.scounts, 0));
    LAUNCH(c, "k_survivor_ranges", k_survivor_ranges, dim3(nf), dim3(128), points, p.dog_cap, s.surv, s.scounts, (unsigned int)scap, L.n_octaves, s.ranges);
    const auto k_surv = F32_KERNEL(c, k_orient_survivors);
    TRY(raise_dyn_lds(c, reinterpret_cast<const void*>(k_surv)));
    const int gwg = (int)std::min<long>(1024, std::max<long>(16, 8192 / nf));
    // The launches below are independent (each takes its own survivors, each writes its own mask words) and every one ends
    // on a tail of half-empty CUs: with two idle side streams at hand (the Harris chain's and the upsample's: both are
    // done long before the list is) they go out round-robin over three streams and share the chip.
    const bool spread = plan.spread;
    const hipStream_t side_a = lane_stream(c, Lane::Harris), side_b = lane_stream(c, Lane::Up);
    hipStream_t lanes[3] = {c->stream, spread ? side_a : c->stream, spread ? side_b : c->stream};
    if (spread) {
        HIPCHK(c, hipEventRecord(c->ev_or_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(side_a, c->ev_or_fork, 0));
        HIPCHK(c, hipStreamWaitEvent(side_b, c->ev_or_fork, 0));
    }
    int next = 0;
    {
        TimedScope ts(c, "k_orient_survivors");  // with the launches spread, this brackets the main stream's share only
        for (int o = 0; o < L.n_octaves; ++o) {  // one launch per octave: its own survivors, its own LDS footprint
            if (pl.smax[o] <= OR_PK_MAX_SPAN && !c->orient_scalar_form) {  // the fine octaves: packed-f32 form, two waves per survivor, one launch per level
                // 8 gwg workgroups per frame (256 at 256 frames): ~20 survivors each on a dense frame.  With 2 gwg (80 each) the
                // launch ended on a long tail of half-empty CUs: 9.0 ms of these launches per 256-frame step against 8.4
                constexpr int pk_mult = 8;
                for (int l = 1; l <= 3; ++l) {
                    auto kfn = k_orient_survivors_pk<0, false>;
                    if (c->f32_fused) {  // (vslam_ctx_set_f32_fused: the multiply-adds of the blur as v_pk_fma_f32; the generic tap count serves every level)
                        kfn = k_orient_survivors_pk<0, true>;
                    } else {
                        switch (g.kn[o][l]) {  // the default pyramid's octave 0 (sigma0 = 1.6) with its tap counts compiled in: 6.85 -> 6.5 ms per step
                            case 25: kfn = k_orient_survivors_pk<25, false>; break;
                            case 31: kfn = k_orient_survivors_pk<31, false>; break;
                            case 39: kfn = k_orient_survivors_pk<39, false>; break;
                            default: break;
                        }
                    }
                    hipLaunchKernelGGL(kfn, dim3(pk_mult * gwg, nf), dim3(128), (size_t)orient_pk_lds_floats(OR_WIN + 2 * (g.kn[o][l] / 2)) * 4,
                                       lanes[next++ % 3], points, p.dog_cap, s.surv, s.ranges, (unsigned int)scap, pyr, pframe, g, o, l, s.masks);
                }
                continue;
            }
            hipLaunchKernelGGL(k_surv, dim3(gwg, nf), dim3(256), (size_t)pl.need[o] * 4, lanes[next++ % 3], points, p.dog_cap, s.surv, s.ranges,
                               (unsigned int)scap, pyr, pframe, g, pl.need[o], o, s.masks);
        }
    }
    HIPCHK(c, hipGetLastError());
    if (spread) {
        HIPCHK(c, hipEventRecord(c->ev_or_join[0], side_a));
        HIPCHK(c, hipEventRecord(c->ev_or_join[1], side_b));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_or_join[0], 0));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_or_join[1], 0));
    }
    OrientBatchEntries oe{s.masks, s.surv, s.scounts, (unsigned int)scap, points, p.dog_cap, oriented};
    TRY(enqueue_compaction(c, oe, scap, nf, s.cws, (unsigned int)scap, oriented_counts, 0));
    return VSLAM_OK;
}

// SIFT() for the oriented lists of nf frames (kernels_sift.hip.h), on the context's current stream,
// behind the kernels that produced the lists.
static int enqueue_sift_batch(vslam_ctx* c, const vslam_params& p, const vslam_batch_layout& L, int nf, const uint8_t* pyr, size_t pframe,
                              const vslam_point* oriented, const unsigned int* ocounts, float* desc, uint8_t* defined) {
    SiftBatchGeom g;
    TRY(fill_batch_geom(c, p, L, g));  // same taps as the orientation blur
    for (int b = 0; b < 36; ++b) vslam_cos_sin_deg((float)(10 * b), &g.cs36[b].x, &g.cs36[b].y);  // host libm, like the reference
    // 8 x 32 workgroups per frame at 256 frames (~120 points each on a dense frame): with 32 the launch ended on a tail of
    // half-empty CUs (11.3 ms per 256-frame step against 10.1)
    const int gwg = 8 * (int)std::min<long>(1024, std::max<long>(16, 8192 / nf));
    LAUNCH(c, "k_sift_descriptors", F32_KERNEL(c, k_sift_descriptors_batch), dim3(gwg, nf), dim3(256), oriented, ocounts, p.oriented_cap, pyr, pframe, g, desc, defined);
    return VSLAM_OK;
}

static int enqueue_harris_on(vslam_ctx* c, hipStream_t st, const HarrisChunk& h) {
    StreamSwap sw(c, st);
    return enqueue_harris(c, h.frames, h.fframe, h.rows, h.cols, h.nf, h.k, h.resp, h.mask, h.nms2, h.hflags, h.kps, h.cap, h.counts, h.cws);
}

// createPyramid (GaussPyramid.cpp:106-131) + initialKeypointDetection (Diff_of_Gauss.cpp:254) for the frames of one chunk,
// with the chunk's other work enqueued where d.plan puts it: the one loop of the batched path and of vslam_pyramid_build_u8.
static int enqueue_dog(vslam_ctx* c, DogChunk& d, const HarrisChunk* hc, const OrientPlan* opl, OrientScratch* os) {
    // (why the gate octave and which work is held back behind it: vslam_batch_plan.h)
    const BatchPlan& pl = d.plan;
    const int n_oct = d.L.n_octaves;
    TRY(d.begin(c));
    struct TagReset {
        vslam_ctx* c;
        ~TagReset() { c->launch_tag = -1; }
    } tag_reset{c};
    for (int o = 0, oo = 0; o < n_oct; ++o) {
        c->launch_tag = o;  // the timing hook's "name@o" (TimedScope) for every launch enqueued at this octave
        TRY(d.octave(c, o));
        if (hc && o == pl.harris_after) {
            HIPCHK(c, hipStreamWaitEvent(lane_stream(c, pl.harris_lane), c->ev_oct[o], 0));
            TRY(enqueue_harris_on(c, lane_stream(c, pl.harris_lane), *hc));
        }
        for (; oo < n_oct && pl.after[oo] == o; ++oo) {  // the scans due now, the held-back ones in order
            TRY(d.scan_octave(c, oo, o));
            if (oo == 0 && pl.early_edge) {  // on the stream the list is written on, behind octave 0's records
                StreamSwap sw(c, lane_stream(c, pl.scan_lane));
                TRY(enqueue_edge_flags_early(c, d.p, *opl, d.nf, d.out.pyr, d.out.pframe, d.out.points, d.out.counts, *os, pl.early_edge_forked));
            }
        }
    }
    if (pl.ev_chunk) HIPCHK(c, hipEventRecord(c->ev_chunk, c->stream));
    return VSLAM_OK;
}

// The outputs of the chunk of a batch call that starts at frame f0: every buffer the caller gave, f0 frames further on
// (and that much shorter: a pointer still travels with the size of what lies behind it).
static vslam_batch_out chunk_out(const vslam_batch_out& out, const vslam_params& p, const vslam_batch_layout& L, int f0) {
    const size_t N = (size_t)p.rows * p.cols;
    vslam_batch_out co = out;
    auto advance = [f0](auto*& ptr, size_t& bytes, size_t per_frame) {
        if (!ptr) return;
        ptr += (size_t)f0 * per_frame;
        bytes -= (size_t)f0 * per_frame * sizeof(*ptr);
    };
#define VSLAM_ADVANCE(field, per_frame) advance(co.field, co.field##_bytes, per_frame)
    VSLAM_ADVANCE(response, N), VSLAM_ADVANCE(nms_mask, N), VSLAM_ADVANCE(nms2, N);
    VSLAM_ADVANCE(harris_kps, p.harris_cap), VSLAM_ADVANCE(harris_counts, 1);
    VSLAM_ADVANCE(pyramid, L.pyramid_frame_bytes), VSLAM_ADVANCE(extrema_bits, L.bits_frame_words);
    VSLAM_ADVANCE(dog_points, p.dog_cap), VSLAM_ADVANCE(dog_counts, 1);
    VSLAM_ADVANCE(oriented_points, p.oriented_cap), VSLAM_ADVANCE(oriented_counts, 1), VSLAM_ADVANCE(oriented_survivors, 1);
    VSLAM_ADVANCE(descriptors, (size_t)p.oriented_cap * 128), VSLAM_ADVANCE(descriptor_defined, p.oriented_cap);
#undef VSLAM_ADVANCE
    return co;
}

int vslam_detect_batch_dev(vslam_ctx* c, const vslam_params* pp, const uint8_t* d_frames, size_t frame_stride,
                           int n_frames, const vslam_batch_out* out) {
    TRY(bind_device(c));
    ARGCHK(c, pp && d_frames && out && n_frames > 0, "detect_batch: bad arguments");
    const vslam_params p = *pp;
    ARGCHK(c, p.rows > 0 && p.cols > 0 && frame_stride >= (size_t)p.rows * p.cols, "detect_batch: bad frame geometry");
    vslam_batch_layout L;
    if (make_layout(&p, &L) != VSLAM_OK) return fail(c, VSLAM_ERR_INVALID, "detect_batch: bad parameters");
    const bool dog = p.n_octaves > 0;
    const bool want_kps = out->harris_kps && out->harris_counts;
    const bool harris = p.do_harris && (out->response || out->nms_mask || out->nms2 || want_kps);
    ARGCHK(c, !dog || out->pyramid, "detect_batch: the DoG path needs out->pyramid");
    {   // every buffer against the size the caller states for it: nothing is launched on an undersized buffer
        ARGCHK(c, out->struct_size == sizeof(vslam_batch_out),
               "detect_batch: out->struct_size is not sizeof(vslam_batch_out) (set it and every x_bytes; vslam_batch_out_required gives the numbers)");
        vslam_batch_out need{};
        if (vslam_batch_out_required(&p, n_frames, &need) != VSLAM_OK) return fail(c, VSLAM_ERR_INVALID, "detect_batch: bad parameters");
#define VSLAM_SIZECHK(field)                                                                                               \
    if (out->field && out->field##_bytes < need.field##_bytes)                                                             \
        return fail(c, VSLAM_ERR_INVALID, std::string("detect_batch: out->" #field " holds ") + std::to_string(out->field##_bytes) + \
                                              " bytes, " + std::to_string(n_frames) + " frames need " + std::to_string(need.field##_bytes))
        VSLAM_SIZECHK(response);
        VSLAM_SIZECHK(nms_mask);
        VSLAM_SIZECHK(nms2);
        VSLAM_SIZECHK(harris_kps);
        VSLAM_SIZECHK(harris_counts);
        VSLAM_SIZECHK(pyramid);
        VSLAM_SIZECHK(extrema_bits);
        VSLAM_SIZECHK(dog_points);
        VSLAM_SIZECHK(dog_counts);
        VSLAM_SIZECHK(oriented_points);
        VSLAM_SIZECHK(oriented_counts);
        VSLAM_SIZECHK(oriented_survivors);
        VSLAM_SIZECHK(descriptors);
        VSLAM_SIZECHK(descriptor_defined);
#undef VSLAM_SIZECHK
    }
    const bool orient = dog && p.orient;
    ARGCHK(c, !orient || (p.localize && out->dog_points && out->dog_counts && out->oriented_points && out->oriented_counts &&
                          p.oriented_cap > 0 && p.dog_cap > 0 && p.extrema_window == 3),
           "detect_batch: orient needs localize = 1, windowSize 3, the DoG point list and the oriented outputs");
    ARGCHK(c, !out->descriptors || orient, "detect_batch: descriptors need orient = 1");
    ARGCHK(c, !out->descriptor_defined || out->descriptors, "detect_batch: descriptor_defined without descriptors");
    const size_t N = (size_t)p.rows * p.cols;
    // Whole-batch launches: every kernel sees all frames (grid.z = frames), so even the coarse
    // octaves fill the chip.  Scratch: octave bases (+ u16 row sums of the non-tiled octaves).
    const int chunk = std::min(n_frames, 256);
    const std::vector<OctPlan> plans = plan_octaves(p.sigma0, L);
    // the plan of a chunk (vslam_batch_plan.h): what does not change over the call here, the rest per chunk below
    BatchPlanIn pin = batch_plan_input(c, p, L, plans, p.cols);
    pin.nf = chunk;
    pin.harris = harris;
    pin.lists = out->dog_points && out->dog_counts;
    pin.do_extrema = out->extrema_bits || pin.lists;
    pin.bases_are_scratch = true;
    DogScratch s;
    OrientScratch os;
    float* resp_ws = nullptr;
    unsigned long long* hflags = nullptr;
    unsigned int* hcws = nullptr;
    WsPlan ws;
    if (dog) dog_scratch_plan(ws, L, plans, chunk, s, batch_plan(pin).sitemap);
    if (orient) orient_scratch_plan(ws, p, chunk, os);
    if (harris) {
        if (!out->response) ws.add(resp_ws, (size_t)chunk * N);
        ws.add(hflags, (size_t)chunk * harris_flag_words(p.rows, p.cols));
        ws.add(hcws, compaction_ws_elems(harris_flag_words(p.rows, p.cols), chunk));
    }
    c->phase_marked = false;
    TRY(ws.commit(c));
    OrientPlan opl;
    if (orient) TRY(make_orient_plan(c, p, L, opl));
    // Fork: the Harris chain and the extrema/compaction chain run on the context's auxiliary streams beside the octave
    // kernels.  Measured on MI355X: +2.8 % (11.2k vs 10.9k frames/s) -- small, because every kernel of the batch is
    // VALU-issue-bound rather than HBM-bound; per-kernel durations grow accordingly when kernels share the chip.
    // (the capture rule - no fork from one side stream to another while a capture is on - is batch_plan()'s)
    pin.capturing = stream_is_capturing(c);
    // the shape of this call (the stream tuner and the join watchdog compare calls of one shape only)
    const unsigned long long call_key = ((unsigned long long)(unsigned)n_frames << 40) ^ ((unsigned long long)(unsigned)p.rows << 20) ^ (unsigned)p.cols ^
                                        ((unsigned long long)(p.localize + 2 * p.orient + 4 * p.extrema_dense + 8 * (out->descriptors != nullptr)) << 60) ^
                                        ((unsigned long long)(unsigned)p.n_octaves << 56) ^ ((unsigned long long)(c->mx ? 1 : 0) << 39);
    BatchFork fork{c};  // (an early return below drains the side streams)
    TRY(fork.begin(call_key, dog && harris && n_frames >= 32, (size_t)n_frames * N >= ((size_t)16 << 20), pin.capturing));
    pin.side = fork.side;
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int nf = std::min(chunk, n_frames - f0);
        const uint8_t* fr = d_frames + (size_t)f0 * frame_stride;
        const vslam_batch_out co = chunk_out(*out, p, L, f0);
        pin.nf = nf;
        pin.later_chunk = f0 > 0;
        const BatchPlan plan = batch_plan(pin);
        // The Harris chain: without the DoG path or the side streams it is simply enqueued here.  With
        // them it goes to its own stream - at once for small batches, behind the last LDS-tiled octave
        // kernel for large ones (vslam_batch_plan.h explains the gate; enqueue_dog enqueues it there).
        const HarrisChunk hc{fr, frame_stride, p.rows, p.cols, nf, p.harris_k, co.response ? co.response : resp_ws, co.nms_mask, co.nms2,
                             want_kps ? hflags : nullptr, want_kps ? co.harris_kps : nullptr, p.harris_cap, want_kps ? co.harris_counts : nullptr, hcws};
        if (harris && plan.harris_after < 0) TRY(enqueue_harris_on(c, lane_stream(c, plan.harris_lane), hc));
        if (dog) {
            const size_t pframe = L.pyramid_frame_bytes;
            DogChunk d{p, L, plans, fr, (size_t)p.cols, frame_stride, nf, s,
                       DogOut{co.pyramid, pframe, (unsigned long long*)co.extrema_bits, pin.do_extrema, co.dog_points, co.dog_counts}, plan};
            TRY(enqueue_dog(c, d, harris ? &hc : nullptr, orient ? &opl : nullptr, &os));
            if (orient) {  // filterKeypoints behind the list, on the stream that produced it
                StreamSwap sw(c, lane_stream(c, plan.scan_lane));
                TRY(enqueue_orient_batch(c, p, L, opl, nf, co.pyramid, pframe, co.dog_points, co.dog_counts, os, co.oriented_points, co.oriented_counts, plan));
                if (co.oriented_survivors)
                    HIPCHK(c, hipMemcpyAsync(co.oriented_survivors, os.scounts, sizeof(unsigned int) * (size_t)nf, hipMemcpyDeviceToDevice, c->stream));
                if (co.descriptors)
                    TRY(enqueue_sift_batch(c, p, L, nf, co.pyramid, pframe, co.oriented_points, co.oriented_counts, co.descriptors, co.descriptor_defined));
            }
        }
    }
    return fork.end();
}


int vslam_ctx_follow(vslam_ctx* c, const vslam_ctx* leader) {
    TRY(bind_device(c));
    ARGCHK(c, leader && leader != c && leader->device == c->device, "ctx_follow: the leader must be another context on the same device");
    if (leader->ev_phase) HIPCHK(c, hipStreamWaitEvent(c->stream, leader->ev_phase, 0));  // no batch call yet: nothing to wait for
    return VSLAM_OK;
}

int vslam_detect_batch_host(vslam_ctx* c, const vslam_params* pp, const uint8_t* frames, size_t frame_stride, int n_frames,
                            const vslam_host_lists* out) {
    TRY(bind_device(c));
    ARGCHK(c, pp && frames && out && n_frames > 0 && n_frames <= 65535, "detect_batch_host: bad arguments");
    ARGCHK(c, out->struct_size == sizeof(vslam_host_lists), "detect_batch_host: out->struct_size is not sizeof(vslam_host_lists)");
    vslam_params p = *pp;
    ARGCHK(c, p.rows > 0 && p.cols > 0 && frame_stride >= (size_t)p.rows * p.cols, "detect_batch_host: bad frame geometry");
    ARGCHK(c, !p.orient && !p.extrema_dense, "detect_batch_host: the Harris and DoG lists only (orient / extrema_dense: vslam_detect_batch_dev)");
    const bool want_h = out->harris || out->harris_offsets || out->harris_counts, want_d = out->dog || out->dog_offsets || out->dog_counts;
    ARGCHK(c, !want_h || (out->harris_offsets && out->harris_counts && (out->harris || out->harris_bytes == 0)), "detect_batch_host: incomplete Harris list");
    ARGCHK(c, !want_d || (out->dog_offsets && out->dog_counts && (out->dog || out->dog_bytes == 0)), "detect_batch_host: incomplete DoG list");
    ARGCHK(c, want_h || want_d, "detect_batch_host: no list requested");
    p.do_harris = want_h ? 1 : 0;
    if (!want_d) p.n_octaves = 0;
    ARGCHK(c, !want_d || p.n_octaves > 0, "detect_batch_host: the DoG list needs n_octaves > 0");
    vslam_batch_out need{};
    if (vslam_batch_out_required(&p, n_frames, &need) != VSLAM_OK) return fail(c, VSLAM_ERR_INVALID, "detect_batch_host: bad parameters");
    const size_t n = (size_t)n_frames, N = (size_t)p.rows * p.cols;
    // one device block for everything this call needs (recycled through the context's block cache when small)
    const size_t hpk = want_h ? out->harris_bytes / sizeof(vslam_kp) * sizeof(vslam_kp) : 0, dpk = want_d ? out->dog_bytes / sizeof(vslam_point) * sizeof(vslam_point) : 0;
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += align_up(bytes ? bytes : 1, 256);
        return o;
    };
    const size_t o_frames = carve(n * N), o_pyr = carve(want_d ? need.pyramid_bytes : 0), o_hk = carve(want_h ? need.harris_kps_bytes : 0),
                 o_hc = carve(n * 4), o_dp = carve(want_d ? need.dog_points_bytes : 0), o_dc = carve(n * 4), o_hp = carve(hpk), o_dpk = carve(dpk),
                 o_off = carve(2 * (n + 1) * 8);
    size_t cap = 0;
    char* blk = (char*)block_alloc(c, off, &cap);
    if (!blk) return fail(c, VSLAM_ERR_NOMEM, "detect_batch_host: device allocation failed");
    struct Release {
        vslam_ctx* c;
        void* p;
        size_t cap;
        ~Release() {
            (void)hipStreamSynchronize(c->stream);
            block_release(c, p, cap);
        }
    } rel{c, blk, cap};
    uint8_t* d_frames = (uint8_t*)(blk + o_frames);
    HIPCHK(c, hipMemsetAsync(blk + o_hc, 0, n * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(blk + o_dc, 0, n * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(blk + o_off, 0, 2 * (n + 1) * 8, c->stream));
    TRY(h2d(c, d_frames, N, frames, frame_stride, N, n));
    vslam_batch_out bo{};
    bo.struct_size = sizeof(bo);
    if (want_h) {
        bo.harris_kps = (vslam_kp*)(blk + o_hk), bo.harris_kps_bytes = need.harris_kps_bytes;
        bo.harris_counts = (uint32_t*)(blk + o_hc), bo.harris_counts_bytes = need.harris_counts_bytes;
    }
    if (want_d) {
        bo.pyramid = (uint8_t*)(blk + o_pyr), bo.pyramid_bytes = need.pyramid_bytes;
        bo.dog_points = (vslam_point*)(blk + o_dp), bo.dog_points_bytes = need.dog_points_bytes;
        bo.dog_counts = (uint32_t*)(blk + o_dc), bo.dog_counts_bytes = need.dog_counts_bytes;
    }
    TRY(vslam_detect_batch_dev(c, &p, d_frames, N, n_frames, &bo));
    uint64_t* d_off = (uint64_t*)(blk + o_off);
    if (want_h) TRY(vslam_pack_lists_dev(c, bo.harris_kps, sizeof(vslam_kp), p.harris_cap, bo.harris_counts, n_frames, blk + o_hp, hpk, d_off));
    if (want_d) TRY(vslam_pack_lists_dev(c, bo.dog_points, sizeof(vslam_point), p.dog_cap, bo.dog_counts, n_frames, blk + o_dpk, dpk, d_off + (n + 1)));
    if (want_h) {
        HIPCHK(c, hipMemcpyAsync(out->harris_offsets, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out->harris_counts, bo.harris_counts, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_d) {
        HIPCHK(c, hipMemcpyAsync(out->dog_offsets, d_off + (n + 1), (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out->dog_counts, bo.dog_counts, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the offsets say how many records exist
    if (want_h) {
        const size_t bytes = std::min<size_t>(out->harris_offsets[n] * sizeof(vslam_kp), hpk);
        if (bytes) HIPCHK(c, hipMemcpyAsync(out->harris, blk + o_hp, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_d) {
        const size_t bytes = std::min<size_t>(out->dog_offsets[n] * sizeof(vslam_point), dpk);
        if (bytes) HIPCHK(c, hipMemcpyAsync(out->dog, blk + o_dpk, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

int vslam_pack_lists_dev(vslam_ctx* c, const void* lists, size_t record_bytes, uint32_t cap, const uint32_t* counts, int n_frames,
                         void* packed, size_t packed_bytes, uint64_t* offsets) {
    TRY(bind_device(c));
    ARGCHK(c, lists && counts && offsets && n_frames > 0 && n_frames <= 65535 && cap > 0 && (packed || packed_bytes == 0),
           "pack_lists: bad arguments (1 .. 65535 frames per call)");
    ARGCHK(c, record_bytes >= 4 && record_bytes % 4 == 0 && record_bytes <= 4096, "pack_lists: record_bytes must be a multiple of 4");
    const unsigned int rec_dw = (unsigned int)(record_bytes / 4);
    LAUNCH(c, "k_pack_offsets", k_pack_offsets, dim3(1), dim3(256), counts, cap, n_frames, (unsigned long long*)offsets);
    const unsigned long long frame_dw = (unsigned long long)cap * rec_dw;
    const unsigned int gx = (unsigned int)std::min<unsigned long long>((frame_dw + 2047) / 2048, 96);
    if (packed_bytes >= 4)
        LAUNCH(c, "k_pack_copy", k_pack_copy, dim3(gx, 1, n_frames), dim3(256), (const unsigned int*)lists, rec_dw, cap, counts,
               (const unsigned long long*)offsets, (unsigned int*)packed, (unsigned long long)(packed_bytes / 4));
    return VSLAM_OK;
}

int vslam_pack_points16_dev(vslam_ctx* c, const vslam_point* lists, uint32_t cap, const uint32_t* counts, int n_frames, vslam_point16* packed,
                            size_t packed_bytes, uint64_t* offsets) {
    TRY(bind_device(c));
    ARGCHK(c, lists && counts && offsets && n_frames > 0 && n_frames <= 65535 && cap > 0 && (packed || packed_bytes == 0),
           "pack_points16: bad arguments (1 .. 65535 frames per call)");
    ARGCHK(c, (reinterpret_cast<uintptr_t>(lists) & 7) == 0 && (reinterpret_cast<uintptr_t>(packed) & 15) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7) == 0,
           "pack_points16: lists must be 8-byte aligned, packed 16-byte aligned (the records move as 8- and 16-byte words)");
    static_assert(sizeof(vslam_point) == 24 && sizeof(vslam_point16) == 16, "record layouts");
    LAUNCH(c, "k_pack_offsets", k_pack_offsets, dim3(1), dim3(256), counts, cap, n_frames, (unsigned long long*)offsets);
    const unsigned int gx = (unsigned int)std::min<unsigned long long>(((unsigned long long)cap + 1023) / 1024, 96);
    if (packed_bytes >= sizeof(vslam_point16))
        LAUNCH(c, "k_pack_copy", k_pack_points16, dim3(gx, 1, n_frames), dim3(256), reinterpret_cast<const int2*>(lists), cap, counts,
               (const unsigned long long*)offsets, reinterpret_cast<uint4*>(packed), (unsigned long long)(packed_bytes / sizeof(vslam_point16)));
    return VSLAM_OK;
}

int vslam_count_totals_dev(vslam_ctx* c, const uint32_t* harris_counts, const uint32_t* dog_counts, int n_frames, uint64_t* totals) {
    TRY(bind_device(c));
    ARGCHK(c, totals && n_frames > 0 && (harris_counts || dog_counts), "count_totals: bad arguments");
    LAUNCH(c, "k_count_totals", k_count_totals, dim3(1), dim3(256), harris_counts, dog_counts, n_frames, (unsigned long long*)totals);
    return VSLAM_OK;
}

}  // extern "C"
