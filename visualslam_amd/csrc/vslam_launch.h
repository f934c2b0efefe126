// What the HIP translation units of the C ABI (every vslam_*.hip but the matrix-core octave kernels' vslam_mx.hip and
// vslam_mx0.hip) share to enqueue kernels: the launch macros the timing hook sees, the helpers one unit compiles for the
// others, the context's bump workspace with its per-call plan, and the plumbing of the host-memory entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vslam_ctx.h"
#include "vslam_place_plan.h"

// Launch on `stream` with `lds` bytes of dynamic LDS, bracketed for the timing hook as "name@tag".
#define LAUNCH_ON(ctx, name, tag, stream, lds, kern, grid, block, ...)        \
    do {                                                                      \
        {                                                                     \
            TimedScope ts_(ctx, name, tag, stream);                           \
            hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);  \
        }                                                                     \
        HIPCHK(ctx, hipGetLastError());                                       \
    } while (0)
// ... on the context stream, no dynamic LDS, tagged with the octave being enqueued.
#define LAUNCH(ctx, name, kern, grid, block, ...) LAUNCH_ON(ctx, name, (ctx)->launch_tag, (ctx)->stream, 0, kern, grid, block, __VA_ARGS__)
// The instantiation of a `template <bool FMA>` kernel (mad_f32, kernels_aux.hip.h) that the context's f32_fused setting asks for.
#define F32_KERNEL(ctx, kern) ((ctx)->f32_fused ? kern<true> : kern<false>)


static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

namespace vslam {
// Grows the context's workspace to `bytes` (vslam_hip.hip): waits for the context's streams first, never inside a launch sequence.
int ws_reserve(vslam_ctx* c, size_t bytes);
// The match list of vslam_match_dev: count -> scan -> scatter (kernels_compact.hip.h, MatchEntries) over the accepted-query
// flag words of n_pairs pairs, fwords words each.  The compaction kernels are compiled in vslam_hip.hip, with the other lists'.
// chunk_ws: scratch of match_list_ws_elems(fwords, n_pairs) u32; matches may be null (totals only).
size_t match_list_ws_elems(size_t fwords, int n_pairs);
int enqueue_match_list(vslam_ctx* c, const unsigned long long* flags, size_t fwords, const vslam_nn2* nn, unsigned int qcap, int n_pairs,
                       unsigned int* chunk_ws, vslam_match* matches, unsigned int match_cap, unsigned int* match_counts);
// n(row) of every row in use of n_pairs descriptor sets (k_desc_norms, compiled in vslam_match.hip; vslam_match_guided_dev forms
// d2 from the same norms): norms [n_pairs][S.cap].
int enqueue_desc_norms(vslam_ctx* c, const vslam_desc_sets& S, int n_pairs, float* norms);
// The merge of the guided searches' partial results with the guided acceptance (k_match_guided_merge, compiled in
// vslam_match_guided.hip; vslam_match_guided_hf_dev merges its own search's parts the same way): part [n_pairs][nsplit][Q.cap]
// -> nn [n_pairs][Q.cap] and the accepted-query ballot words flags [n_pairs][fwords].
struct MatchPart;
int enqueue_guided_merge(vslam_ctx* c, const vslam_desc_sets& Q, int n_pairs, const MatchPart* part, unsigned int nsplit, float ratio2,
                         float max_desc_dist2, vslam_nn2* nn, unsigned long long* flags, unsigned int fwords);
// The inlier list of vslam_epipolar_dev, the same way (EpipolarEntries): the winner's ballot words over the match records of
// n_pairs pairs -> the inlier records in list order.  chunk_ws as above; inliers may be null (totals only).
int enqueue_inlier_list(vslam_ctx* c, const unsigned long long* flags, size_t fwords, const vslam_match* matches, const unsigned int* match_counts,
                        unsigned int match_cap, int n_pairs, unsigned int* chunk_ws, vslam_match* inliers, unsigned int inlier_cap,
                        unsigned int* inlier_counts);
// The {x, y, x', y'} scratch of the two-view entry points (k_epi_coords, compiled in vslam_epipolar.hip; vslam_pose_dev reads
// the same records): one EpiXY per match record below each pair's count, xy [n_pairs][match_cap].
struct EpiXY;
int enqueue_epi_coords(vslam_ctx* c, const vslam_match* matches, const unsigned int* match_counts, unsigned int match_cap,
                       const vslam_point* query_points, unsigned int query_cap, const vslam_point* train_points, unsigned int train_cap,
                       int n_pairs, EpiXY* xy);
// The inlier ballot words of every pair under models[j].F (k_epi_flags, compiled in vslam_epipolar.hip; vslam_refit_dev asks
// for them under its output models): flags [n_pairs][fwords], the words that hold a record below the count.
int enqueue_epi_flags(vslam_ctx* c, const EpiXY* xy, const unsigned int* match_counts, unsigned int match_cap, const vslam_epipolar* models,
                      double max_dist2, int n_pairs, unsigned long long* flags);
// The inlier ballot words of every pair under (models[j].H, models[j].G) (k_hom_flags, compiled in vslam_homography.hip;
// vslam_hrefit_dev asks for them under its output models): flags [n_pairs][fwords], the words that hold a record below the count.
int enqueue_hom_flags(vslam_ctx* c, const EpiXY* xy, const unsigned int* match_counts, unsigned int match_cap, const vslam_homography* models,
                      double max_dist2, int n_pairs, unsigned long long* flags);
// The degeneracy verdict and the gate (k_hom_verdict, compiled in vslam_homography.hip; vslam_hrefit_dev runs it again over
// its output models): models[j].n_epipolar and .degenerate from models[j].n_inliers and epi[j]; gated may be null or epi itself.
int enqueue_hom_verdict(vslam_ctx* c, const vslam_epipolar* epi, int n_pairs, unsigned int num, unsigned int den, unsigned int min_inliers,
                        vslam_homography* models, vslam_epipolar* gated);
// The structure side of the multi-view stages (vslam_chain_dev, vslam_resect_dev, vslam_tracks_dev, vslam_bundle_dev): what
// vslam_pose_dev read and wrote for n_pairs consecutive pairs, and the capacity of the frames' point lists.
struct StructLists {
    const vslam_pose* poses;
    const vslam_match* matches;
    const unsigned int* match_counts;
    unsigned int match_cap;
    const uint64_t* front_bits;
    unsigned int point_cap;
    int n_pairs;
};
// The link table of the trajectory's step 1 (k_chain_link, compiled in vslam_chain.hip; vslam_resect_dev, vslam_tracks_dev and
// vslam_bundle_dev link by the same rule): prev [n_pairs - 1][point_cap] is preset to 0xffffffff and row j - 1 gets, per train
// index, the lowest live record of pair j - 1.  n_pairs >= 2.
int enqueue_chain_link(vslam_ctx* c, const StructLists& L, unsigned int* prev);
// The continuation table of the tracks section's step 2 (k_trk_next, compiled in vslam_tracks.hip; vslam_bundle_dev walks the
// same paths): next [n_pairs - 1][match_cap] is preset to 0xffffffff and row j - 1 gets, per record of pair j - 1, the lowest
// candidate of pair j.  prev: the link table above.  n_pairs >= 2.
int enqueue_trk_next(vslam_ctx* c, const StructLists& L, const vslam_chain* chain, const unsigned int* prev, unsigned int* next);
// The word search of vslam_words_dev (k_desc_norms, k_words_nn, k_words_merge; compiled in vslam_words.hip; every round of
// vslam_vocab_kmeans_dev assigns with it): the word, its d2 and the histogram of n_sets >= 1 sets against the vocabulary V, a
// one-set vslam_desc_sets of pl.m's train capacity whose count the caller has put on the device.  The scratch is the caller's, of
// words_plan's sizes: qnorm pl.m.q_elems, vnorm pl.vnorm_elems, part pl.m.part_elems records of 8 bytes.  row_norms: qnorm is
// computed here (the rows of a caller that asks again have not changed).  words, dist2 and hist may each be null; hist is zeroed.
struct WordsScratch {
    float *qnorm, *vnorm;
    unsigned long long* part;
};
int enqueue_words(vslam_ctx* c, const vslam_desc_sets& sets, int n_sets, const vslam_desc_sets& V, const WordsPlan& pl, const WordsScratch& ws,
                  bool row_norms, int* words, float* dist2, unsigned int* hist);
}  // namespace vslam

// The workspace buffers of one call.  add() states a buffer once - where its pointer goes, its type, its element count -
// and commit() reserves the sum and sets every pointer: the size reserved cannot differ from the size handed out.
// Buffers lie in the order of the add() calls, each on a 256-byte boundary.  No heap: the per-image entry points are
// bound by launch latency, so a request list costs them nothing but a few stores.
// (anonymous namespace, here and below: the member functions of these host-only types stay out of the library's dynamic symbols)
namespace {
class WsPlan {
    struct Slot {
        void* where;                   // the caller's T*
        void (*set)(void*, char*);     // stores a T* there
        size_t off;
    };
    static constexpr int kMaxSlots = 32;  // the most any entry point asks for is 17 (vslam_filter_keypoints)
    Slot slots[kMaxSlots];
    int n = 0;
    size_t total = 0;

  public:
    WsPlan() = default;
    WsPlan(const WsPlan&) = delete;  // (the slots point at the caller's variables)
    WsPlan& operator=(const WsPlan&) = delete;
    template <typename T>
    void add(T*& p, size_t count) {
        if (n < kMaxSlots) slots[n] = Slot{&p, [](void* w, char* q) { *static_cast<T**>(w) = reinterpret_cast<T*>(q); }, total};
        ++n;
        total += align_up(count * sizeof(T), 256);
    }
    // The pointers given to add() must still be where they were: structs that hold them are not moved or copied in between.
    int commit(vslam_ctx* c) {
        if (n > kMaxSlots) return fail(c, VSLAM_ERR_NOMEM, "workspace plan: more buffers than WsPlan::kMaxSlots");
        TRY(vslam::ws_reserve(c, total));
        for (int i = 0; i < n; ++i) slots[i].set(slots[i].where, c->ws + slots[i].off);
        return VSLAM_OK;
    }
};

// The list outputs that the `out` of the four stages over match records has (vslam_epipolar_dev, vslam_refit_dev,
// vslam_homography_dev, vslam_hrefit_dev): inlier_bits, and inlier_counts with inliers.  add() asks for the scratch they need
// - the ballot words when the caller gives no inlier_bits, the compaction's chunk counts -, flags() is where the stage's flags
// kernel writes, list() the compaction.  Not moved between add() and commit(): the plan points at its members.
template <typename Out>
struct ListOut {
    const Out* out;
    unsigned int fwords;  // the plan's: ballot words per pair, and flag_words of them in all
    size_t flag_words;
    int n_pairs;
    unsigned long long* flags_ws = nullptr;
    unsigned int* chunk_ws = nullptr;

    bool wanted() const { return out->inlier_bits || out->inlier_counts; }
    void add(WsPlan& ws) {
        if (wanted() && !out->inlier_bits) ws.add(flags_ws, flag_words);
        if (out->inlier_counts) ws.add(chunk_ws, vslam::match_list_ws_elems(fwords, n_pairs));
    }
    unsigned long long* flags() const { return out->inlier_bits ? reinterpret_cast<unsigned long long*>(out->inlier_bits) : flags_ws; }
    int list(vslam_ctx* c, const vslam_match* matches, const unsigned int* match_counts, unsigned int match_cap) const {
        if (!out->inlier_counts) return VSLAM_OK;
        return vslam::enqueue_inlier_list(c, flags(), fwords, matches, match_counts, match_cap, n_pairs, chunk_ws, out->inliers, out->inlier_cap,
                                          out->inlier_counts);
    }
};
}  // namespace

// What the entry points that work from host memory through per-call device buffers share - DevBufs: every *_host entry point;
// HostPair: the single-pair ones (vslam_epipolar_host, vslam_refit_host, vslam_homography_host, vslam_hrefit_host, vslam_pose_host); HostSets: the
// matchers' (vslam_match_host and its guided and mutual forms); HostMirror: the batched ones (vslam_chain_host, vslam_resect_host,
// vslam_resect_refine_host, vslam_tracks_host, vslam_bundle_host) -, and the answer of a device entry point whose caller has no
// HIP device.
namespace {
// No context can exist without a HIP device, so a caller that has none still gets the ABI's answer for that: checked
// after the arguments, before the context is touched.
inline int usable_ctx(vslam_ctx* c) {
    if (c) return bind_device(c);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return VSLAM_ERR_HIP;
    return VSLAM_ERR_INVALID;
}

// Device buffers of one host-memory call: freed when the call returns.
struct DevBufs {
    std::vector<void*> all;
    ~DevBufs() {
        for (void* p : all) (void)hipFree(p);
    }
    template <typename T>
    int get(vslam_ctx* c, T*& p, size_t count) {
        void* q = nullptr;
        HIPCHK(c, hipMalloc(&q, (count ? count : 1) * sizeof(T)));
        all.push_back(q);
        p = static_cast<T*>(q);
        return VSLAM_OK;
    }
    template <typename T>
    int put(vslam_ctx* c, T*& p, const T* host, size_t count) {
        TRY(get(c, p, count));
        if (count) HIPCHK(c, hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
        return VSLAM_OK;
    }
};

// One host pair of the two-view entry points (vslam_epipolar_host, vslam_refit_host, vslam_homography_host, vslam_hrefit_host,
// vslam_pose_host): the checks they share, in the ABI's order, the device copies of the three lists and of the count, and -
// for the four that have them - the list outputs: lists() fills them into the device entry point's `out`, download() brings
// them back.
struct HostPair {
    const vslam_match* matches;
    const vslam_point *query_points, *train_points;
    size_t n_matches, n_query, n_train;
    vslam_match* d_matches = nullptr;
    vslam_point *d_q = nullptr, *d_t = nullptr;
    uint32_t *d_cnt = nullptr, h_cnt = 0, mcap = 0, qcap = 0, tcap = 0;  // a capacity of at least 1 on every side
    size_t fwords = 0, used_words = 0;                                    // ballot words of the capacity, and those that hold a record
    uint64_t* h_bits = nullptr;                                           // the caller's list outputs, as lists() was given them
    vslam_match* h_inliers = nullptr;
    size_t h_cap = 0, *h_total = nullptr;

    // `more`: a further record count of the stage's; `own`: what a check of the stage's own, due before the last one here, found
    int check(vslam_ctx* c, const char* stage, size_t more = 0, const char* own = nullptr) const {
        ARGCHK(c, (matches || n_matches == 0) && (query_points || n_query == 0) && (train_points || n_train == 0), std::string(stage) + ": null input");
        ARGCHK(c, n_matches < (1u << 31) && n_query < (1u << 31) && n_train < (1u << 31) && more < (1u << 31), std::string(stage) + ": too many records");
        ARGCHK(c, !own, std::string(stage) + ": " + own);
        ARGCHK(c, n_matches == 0 || (n_query > 0 && n_train > 0), std::string(stage) + ": matches without points");
        return VSLAM_OK;
    }
    int upload(vslam_ctx* c, DevBufs& dev) {  // (records without points were refused by check())
        h_cnt = (uint32_t)n_matches;
        TRY(dev.put(c, d_matches, matches, n_matches));
        TRY(dev.put(c, d_q, query_points, n_query));
        TRY(dev.put(c, d_t, train_points, n_train));
        TRY(dev.put(c, d_cnt, &h_cnt, 1));
        mcap = std::max<uint32_t>(h_cnt, 1), qcap = std::max<uint32_t>((uint32_t)n_query, 1), tcap = std::max<uint32_t>((uint32_t)n_train, 1);
        fwords = ((size_t)mcap + 63) / 64, used_words = (n_matches + 63) / 64;
        return VSLAM_OK;
    }
    // After upload(): inlier_bits, inlier_counts, inliers and inlier_cap of `out` (vslam_epipolar_out, vslam_refit_out,
    // vslam_homography_out, vslam_hrefit_out) for the host outputs the caller gave.
    template <typename Out>
    int lists(vslam_ctx* c, DevBufs& dev, Out& out, uint64_t* inlier_bits, vslam_match* inliers, size_t inlier_cap, size_t* n_inliers) {
        h_bits = inlier_bits, h_inliers = inliers, h_cap = inlier_cap, h_total = n_inliers;
        if (inlier_bits) {
            TRY(dev.get(c, out.inlier_bits, fwords));
            out.inlier_bits_bytes = fwords * sizeof(uint64_t);
        }
        if (n_inliers) {
            TRY(dev.get(c, out.inlier_counts, 1));
            out.inlier_counts_bytes = sizeof(uint32_t);
            if (inliers) {
                TRY(dev.get(c, out.inliers, inlier_cap));
                out.inliers_bytes = inlier_cap * sizeof(vslam_match);
                out.inlier_cap = (uint32_t)inlier_cap;
            }
        }
        return VSLAM_OK;
    }
    // After the device entry point and the copies of the entry point's own outputs: the words that hold a record, the total,
    // the wait for the stream, and the list clamped to the caller's capacity.
    template <typename Out>
    int download(vslam_ctx* c, const Out& out) const {
        uint32_t total = 0;
        if (h_bits && used_words) HIPCHK(c, hipMemcpyAsync(h_bits, out.inlier_bits, used_words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (h_total) HIPCHK(c, hipMemcpyAsync(&total, out.inlier_counts, sizeof(total), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h_total) {
            *h_total = total;
            const size_t k = std::min<size_t>(total, h_cap);
            if (h_inliers && k) HIPCHK(c, hipMemcpy(h_inliers, out.inliers, k * sizeof(vslam_match), hipMemcpyDeviceToHost));
        }
        return VSLAM_OK;
    }
};

// The two host descriptor sets and the host outputs of the single-pair matcher entry points (vslam_match_host,
// vslam_match_guided_host, vslam_match_guided_hf_host, vslam_match_mutual_host): the device copies as a vslam_desc_sets pair with
// a capacity of at least 1, the nn / match_counts / matches buffers of the device entry point's `out`, and their way back.
struct HostSets {
    const float* desc[2];  // query, train
    const uint8_t* defined[2];
    const vslam_point* points[2];
    size_t n[2];
    vslam_nn2* nn;
    vslam_match* matches;
    size_t match_cap, *n_matches;
    vslam_desc_sets Q{}, T{};
    uint32_t h_cnt[2] = {0, 0};

    // with_points: the points go up too (with no rows: one unread record, so that the set has its points)
    int upload(vslam_ctx* c, DevBufs& dev, bool with_points) {
        vslam_desc_sets* sets[2] = {&Q, &T};
        for (int i = 0; i < 2; ++i) {
            h_cnt[i] = (uint32_t)n[i];
            float* d = nullptr;
            uint8_t* f = nullptr;
            vslam_point* q = nullptr;
            TRY(dev.put(c, d, desc[i], n[i] * 128));
            if (defined[i]) TRY(dev.put(c, f, defined[i], n[i]));
            if (with_points) TRY(dev.put(c, q, points[i], n[i]));
            *sets[i] = vslam_desc_sets{d, f, q, nullptr, std::max<uint32_t>(h_cnt[i], 1)};
        }
        uint32_t* d_cnt = nullptr;
        TRY(dev.put(c, d_cnt, h_cnt, 2));
        Q.counts = d_cnt, T.counts = d_cnt + 1;
        return VSLAM_OK;
    }
    template <typename Out>  // vslam_match_out, vslam_match_mutual_out
    int outputs(vslam_ctx* c, DevBufs& dev, Out& out) const {
        out.struct_size = sizeof(out);
        if (nn) {
            TRY(dev.get(c, out.nn, n[0]));
            out.nn_bytes = std::max<size_t>(n[0], 1) * sizeof(vslam_nn2);
        }
        if (n_matches) {
            TRY(dev.get(c, out.match_counts, 1));
            out.match_counts_bytes = sizeof(uint32_t);
            if (matches) {
                TRY(dev.get(c, out.matches, match_cap));
                out.matches_bytes = match_cap * sizeof(vslam_match);
                out.match_cap = (uint32_t)match_cap;
            }
        }
        return VSLAM_OK;
    }
    // After the device entry point: nn, then `also` (a whole output of the entry point's own), the total, and the clamped list.
    template <typename Out>
    int download(vslam_ctx* c, const Out& out, void* also = nullptr, const void* d_also = nullptr, size_t also_bytes = 0) const {
        uint32_t total = 0;
        if (nn && n[0]) HIPCHK(c, hipMemcpyAsync(nn, out.nn, n[0] * sizeof(vslam_nn2), hipMemcpyDeviceToHost, c->stream));
        if (also && also_bytes) HIPCHK(c, hipMemcpyAsync(also, d_also, also_bytes, hipMemcpyDeviceToHost, c->stream));
        if (n_matches) HIPCHK(c, hipMemcpyAsync(&total, out.match_counts, sizeof(total), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (n_matches) {
            *n_matches = total;
            const size_t m = std::min<size_t>(total, match_cap);
            if (matches && m) HIPCHK(c, hipMemcpy(matches, out.matches, m * sizeof(vslam_match), hipMemcpyDeviceToHost));
        }
        return VSLAM_OK;
    }
};

// The device mirror of one batched host-memory call: each input and each output is stated once - the host array, its element
// count, where its device pointer goes -, and finish() brings the outputs back whole.  The first failure is kept and what is
// stated after it is skipped: the entry point asks status() once, before the device entry point.  (The single-pair entry
// points copy back parts of their lists: HostPair::download.)
class HostMirror {
    struct Back {
        void* host;
        const void* dev;
        size_t bytes;
    };
    static constexpr int kMaxOut = 8;  // the most any entry point has is 5 (vslam_resect_host)
    vslam_ctx* c;
    DevBufs bufs;
    Back back[kMaxOut];
    int n = 0, rc = VSLAM_OK;

  public:
    explicit HostMirror(vslam_ctx* ctx) : c(ctx) {}
    // An input goes up; an optional one that is not there stays null.
    template <typename T>
    T* in(const T* host, size_t count) {
        T* d = nullptr;
        if (host && !rc) rc = bufs.put(c, d, host, count);
        return d;
    }
    // An output the caller gave (the others are skipped): d gets `count` elements on the device and bytes their size.  keep: the
    // caller's bytes go up first, so that the rows the call leaves untouched come back as they were; otherwise the call writes
    // every element.  A d that is set already is the buffer (in place over an input).
    template <typename T>
    void out(T*& d, size_t& bytes, T* host, size_t count, bool keep) {
        if (!host || rc) return;
        if (n == kMaxOut) rc = fail(c, VSLAM_ERR_NOMEM, "host mirror: more outputs than HostMirror::kMaxOut");
        else if (!d) rc = keep ? bufs.put(c, d, static_cast<const T*>(host), count) : bufs.get(c, d, count);
        if (rc) return;
        bytes = count * sizeof(T);
        back[n++] = Back{host, d, bytes};
    }
    int status() const { return rc; }
    // After the device entry point: the outputs come back in the order they were stated, and the call waits for them.
    int finish() {
        for (int i = 0; i < n; ++i) HIPCHK(c, hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return VSLAM_OK;
    }
};
}  // namespace
