// Vocabulary training (include/vslam.h, "vocabulary training"): what one round of Lloyd's algorithm runs after the word search
// (kernels_words.hip.h, as vslam_words_dev enqueues it) has written this round's words and the histogram of words per set.
//   k_kmeans_init       : once per call: the clamped counts of the sets (the call's own copy) and the call's state
//   k_kmeans_count      : the rows in use whose word differs from the last round's: one integer atomic add per wave
//   k_kmeans_columns    : hist[.][k] -> its exclusive scan over the sets, in place (one thread per word), and N_k
//   k_kmeans_scan       : one workgroup: the exclusive scans of N_k and of the blocks ceil(N_k / 256) over the words, the round's
//                         report, and the verdict: a converged call sets state->done and zeroes the call's copy of the counts
//   k_kmeans_members    : one workgroup per set walks its rows in chunks of 256, ascending; a row's slot is the start of its word +
//                         the set's offset in it + the row's rank among the chunk's rows of that word (from the chunk's words in
//                         LDS); the set's offset row is the cursor, advanced by this workgroup alone: no atomics
//   k_kmeans_block_sums : one wave per block of <= 256 members: lane l owns dimensions 2l and 2l + 1 (a 64-bit load per row,
//                         512 bytes across the wave), eight rows in flight ahead of the two f64 additions per row they feed
//   k_kmeans_update     : one workgroup per word, one thread per dimension: folds the word's block sums in ascending order,
//                         divides, rounds, writes the word and its size
// Every kernel after the verdict reads state->done and returns at once; the word search of the later rounds returns at once
// because every count it reads is 0.  Integers decide where a row goes; the f64 additions happen in the order of the header
// alone: member order inside a block (one lane, one accumulator per dimension), block order inside a word.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "vslam_kmeans_plan.h"

namespace vslam {

struct KmState {
    unsigned int done;     // the call has converged
    unsigned int changed;  // k_kmeans_count's sum of this round, taken and zeroed by k_kmeans_scan
    unsigned int pad[2];
};

// grid = ceil(n_sets / 256)
__global__ __launch_bounds__(256) void k_kmeans_init(const unsigned int* __restrict__ counts, unsigned int cap, unsigned int n_sets,
                                                     unsigned int K, unsigned int* __restrict__ kcounts, unsigned int* __restrict__ vcount,
                                                     KmState* __restrict__ state) {
    const unsigned int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_sets) kcounts[f] = min(counts[f], cap);
    if (f == 0) {
        *state = KmState{0u, 0u, {0u, 0u}};
        *vcount = K;
    }
}

// grid = (ceil(cap / 256), n_sets).  first: round 1, where every row in use counts.
__global__ __launch_bounds__(256) void k_kmeans_count(const unsigned int* __restrict__ kcounts, unsigned int cap, const int* __restrict__ cur,
                                                      const int* __restrict__ prev, int first, KmState* state) {
    if (state->done) return;
    const unsigned int f = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    bool c = false;
    if (q < kcounts[f]) c = first || cur[(size_t)f * cap + q] != prev[(size_t)f * cap + q];
    const unsigned int n = (unsigned int)__popcll(__ballot(c));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&state->changed, n);
}

// grid = ceil(K / 256).  hist [n_sets][K] -> offs (the same buffer): offs[f][k] = sum of hist[g][k] over g < f; N[k] = the column's sum.
__global__ __launch_bounds__(256) void k_kmeans_columns(unsigned int* hist, unsigned int n_sets, unsigned int K, unsigned int* __restrict__ N,
                                                        const KmState* state) {
    if (state->done) return;
    const unsigned int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    unsigned int run = 0;
    for (unsigned int f = 0; f < n_sets; ++f) {
        const unsigned int h = hist[(size_t)f * K + k];
        hist[(size_t)f * K + k] = run;
        run += h;
    }
    N[k] = run;
}

// grid = 1.  wstart, bstart [K + 1]; report may be null; round: t - 1.
__global__ __launch_bounds__(256) void k_kmeans_scan(const unsigned int* __restrict__ N, const uint8_t* __restrict__ vocab_defined, unsigned int K,
                                                     unsigned int n_sets, unsigned int round, unsigned int* __restrict__ wstart,
                                                     unsigned int* __restrict__ bstart, unsigned int* __restrict__ kcounts,
                                                     unsigned int* __restrict__ vcount, vslam_kmeans_round* __restrict__ report, KmState* state) {
    __shared__ unsigned int s_rows[256], s_blocks[256], s_empty[256];
    __shared__ unsigned int s_conv;
    const unsigned int t = threadIdx.x;
    const bool done = state->done != 0;
    __syncthreads();  // every thread has read the verdict of the rounds before
    if (done) return;
    const unsigned int per = (K + 255) / 256, k0 = min(t * per, K), k1 = min(k0 + per, K);
    unsigned int rows = 0, blocks = 0, empty = 0;
    for (unsigned int k = k0; k < k1; ++k) {
        const unsigned int n = N[k];
        rows += n;
        blocks += (n + KM_BLOCK - 1) / KM_BLOCK;
        empty += (n == 0 && (!vocab_defined || vocab_defined[k])) ? 1u : 0u;
    }
    s_rows[t] = rows, s_blocks[t] = blocks, s_empty[t] = empty;
    __syncthreads();
    if (t == 0) {
        unsigned int r = 0, b = 0, e = 0;
        for (int i = 0; i < 256; ++i) {
            const unsigned int ri = s_rows[i], bi = s_blocks[i];
            s_rows[i] = r, s_blocks[i] = b;
            r += ri, b += bi, e += s_empty[i];
        }
        wstart[K] = r, bstart[K] = b;
        const unsigned int changed = state->changed;
        state->changed = 0;
        const bool conv = round > 0 && changed == 0;
        if (report) report[round] = vslam_kmeans_round{r, changed, e, 1u};
        if (conv) state->done = 1;
        s_conv = conv ? 1u : 0u;
    }
    __syncthreads();
    rows = s_rows[t], blocks = s_blocks[t];
    for (unsigned int k = k0; k < k1; ++k) {
        const unsigned int n = N[k];
        wstart[k] = rows, bstart[k] = blocks;
        rows += n;
        blocks += (n + KM_BLOCK - 1) / KM_BLOCK;
    }
    if (s_conv) {  // the word search of the later rounds finds no row and no word
        for (unsigned int f = t; f < n_sets; f += 256) kcounts[f] = 0;
        if (t == 0) *vcount = 0;
    }
}

// grid = n_sets, KM_CHUNK lanes.  offs [n_sets][K]: k_kmeans_columns' offsets, this workgroup's row of it is its cursor.
// members [rows in use with a word]: the row ids f * cap + q in member order.
__global__ __launch_bounds__(256) void k_kmeans_members(const int* __restrict__ cur, const unsigned int* __restrict__ kcounts, unsigned int cap,
                                                        unsigned int K, unsigned int* offs, const unsigned int* __restrict__ wstart,
                                                        unsigned int* __restrict__ members, const KmState* state) {
    __shared__ int s_w[KM_CHUNK];
    if (state->done) return;
    const unsigned int f = blockIdx.x, t = threadIdx.x, n = kcounts[f];
    unsigned int* cursor = offs + (size_t)f * K;
    for (unsigned int base = 0; base < n; base += KM_CHUNK) {
        const unsigned int q = base + t;
        const int w = q < n ? cur[(size_t)f * cap + q] : -1;
        s_w[t] = w;
        __syncthreads();
        unsigned int before = 0, at = 0;
        bool last = true;
        if (w >= 0) {
            for (unsigned int j = 0; j < KM_CHUNK; ++j) {
                const bool same = s_w[j] == w;
                before += (same && j < t) ? 1u : 0u;
                last = last && !(same && j > t);
            }
            at = cursor[w] + before;
            members[wstart[w] + at] = f * cap + q;
        }
        __syncthreads();  // every cursor of this chunk has been read, and s_w too
        if (w >= 0 && last) cursor[w] = at + 1;
        __syncthreads();  // ... and written, before the next chunk reads it
    }
}

// grid = ceil(max_blocks / KM_WAVES), 64 * KM_WAVES lanes: wave g of the grid owns block g of the list of all blocks of all words
// (bstart [K + 1]: the first block of each word).  bsum [max_blocks][128] f64.
__global__ __launch_bounds__(64 * KM_WAVES) void k_kmeans_block_sums(const float* __restrict__ desc, const unsigned int* __restrict__ members,
                                                                     const unsigned int* __restrict__ wstart, const unsigned int* __restrict__ bstart,
                                                                     unsigned int K, double* __restrict__ bsum, const KmState* state) {
    if (state->done) return;
    const unsigned int lane = threadIdx.x & 63;
    const unsigned int g = __builtin_amdgcn_readfirstlane(blockIdx.x * KM_WAVES + (threadIdx.x >> 6));
    if (g >= bstart[K]) return;
    unsigned int lo = 0, hi = K;  // the word k with bstart[k] <= g < bstart[k + 1]
    while (hi - lo > 1) {
        const unsigned int mid = (lo + hi) >> 1;
        if (bstart[mid] <= g) lo = mid;
        else hi = mid;
    }
    const unsigned int b = g - bstart[lo], first = wstart[lo] + b * KM_BLOCK, n = min(KM_BLOCK, wstart[lo + 1] - first);
    unsigned int ids[KM_BLOCK / 64];
#pragma unroll
    for (unsigned int j = 0; j < KM_BLOCK / 64; ++j) ids[j] = 64 * j + lane < n ? members[first + 64 * j + lane] : 0u;
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (unsigned int j = 0; j < KM_BLOCK / 64; ++j) {
        if (64 * j >= n) break;
        const unsigned int cj = min(64u, n - 64 * j);
        auto row = [&](unsigned int i) {  // this lane's two entries of member 64 j + i
            const unsigned int id = (unsigned int)__builtin_amdgcn_readlane((int)ids[j], (int)i);
            return reinterpret_cast<const float2*>(desc + (size_t)id * 128)[lane];
        };
        unsigned int i = 0;
        for (; i + 8 <= cj; i += 8) {  // eight loads, then the sixteen additions they feed, in member order
            float2 r[8];
#pragma unroll
            for (unsigned int u = 0; u < 8; ++u) r[u] = row(i + u);
#pragma unroll
            for (unsigned int u = 0; u < 8; ++u) {
                a0 = a0 + (double)r[u].x;
                a1 = a1 + (double)r[u].y;
            }
        }
        for (; i < cj; ++i) {  // the last block of a word: up to seven rows more
            const float2 r = row(i);
            a0 = a0 + (double)r.x;
            a1 = a1 + (double)r.y;
        }
    }
    reinterpret_cast<double2*>(bsum + (size_t)g * 128)[lane] = make_double2(a0, a1);
}

// grid = K, 128 lanes.  vocab: V_(t-1) in, V_t out (a word without members is not written).  sizes may be null.
__global__ __launch_bounds__(128) void k_kmeans_update(float* __restrict__ vocab, const unsigned int* __restrict__ wstart,
                                                       const unsigned int* __restrict__ bstart, const double* __restrict__ bsum,
                                                       unsigned int* __restrict__ sizes, const KmState* state) {
    if (state->done) return;
    const unsigned int k = blockIdx.x, d = threadIdx.x;
    const unsigned int n = wstart[k + 1] - wstart[k];
    if (sizes && d == 0) sizes[k] = n;
    if (n == 0) return;
    const unsigned int b0 = bstart[k], b1 = bstart[k + 1];
    double sum = bsum[(size_t)b0 * 128 + d];
    for (unsigned int b = b0 + 1; b < b1; ++b) sum = sum + bsum[(size_t)b * 128 + d];
    vocab[(size_t)k * 128 + d] = (float)(sum / (double)n);
}

}  // namespace vslam
