// filterKeypoints (Diff_of_Gauss.cpp:301-372): edge rejection by
// computeEdgeResponse (:79-109), then the 36-bin orientation histogram (:112-133) of the
// keypoint's 16x16 window, magnitudes weighted by GaussianBlur(sigma = 1.5 * sigma(o, l)).
//
// The reference blurs a 16x16 ROI of the 8-padded magnitude image once per keypoint; the ROI is
// not isolated, so the filter reads the parent around the window and reflect-101 applies at the
// PARENT's edges.  One workgroup per keypoint does exactly that: the row pass over the
// (16 + 2R) x 16 strip the column pass needs goes to LDS, the symmetric column pass, the
// histogram and the peak test follow in the workgroup.  Every f32 operation is rounded where
// OpenCV's scalar filters round (row: s = k0*S0; s += ki*Si left to right; column: s = kc*S0;
// s += k(c+i)*(S(+i) + S(-i)); histogram: row-major += per bin), so the result is the oracle's
// bit for bit.  Peaks leave as a 36-bit mask per keypoint; kernels_compact.hip.h turns the masks
// into the ordered SLAM::point list.
//
// The steps the three orientation kernels share - this one, k_orient_survivors (kernels_orient_batch.hip.h) and
// k_orient_survivors_pk (kernels_orient_pk.hip.h) - are stated here once: the edge test, the gradient of a staged u8 patch,
// magnitude_at, the symmetric column pass, the bin masks of a wave and the histogram / peak mask of a window.  The bin of an
// angle, the magnitude of a gradient and the address of a level's plane, which SIFT needs too, stand in kernels_aux.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_aux.hip.h"

namespace vslam {

constexpr int OR_WIN = 16;   // windowSize, Diff_of_Gauss.cpp:304
constexpr int OR_PAD = 8;    // padding = windowSize / 2, :305
constexpr int OR_BINS = 36;  // :352

struct OrientLevels {  // per Gaussian level of the octave (null / 0 when no keypoint uses it)
    const uint8_t* gauss[VSLAM_NUM_LEVELS];
    const float* mag[VSLAM_NUM_LEVELS];
    const float* orient[VSLAM_NUM_LEVELS];
    const float* kern[VSLAM_NUM_LEVELS];
    int kn[VSLAM_NUM_LEVELS];
};

// computeEdgeResponse on the Sobel (ksize 1, reflect-101) gradients of an 8-bit Gaussian level,
// formed on the fly (they are integers, exact in f32).  Window [y-p, y+p) x [x-p, x+p) of the
// unpadded image at the keypoint's padded coordinates; out-of-image reads (only possible for
// windowSize > 3, where the reference itself reads out of bounds) are clamped like the oracle.
__device__ __forceinline__ float edge_response_u8(const uint8_t* __restrict__ G, int gpitch, int rows, int cols, int y, int x, int pad) {
    float Ix2 = 0.f, Iy2 = 0.f, IxIy = 0.f;
    for (int u = y - pad; u < y + pad; ++u) {
        const int r = clampi(u, 0, rows - 1);
        for (int v = x - pad; v < x + pad; ++v) {
            const int c = clampi(v, 0, cols - 1);
            float gx, gy;
            gradient_at(G, gpitch, rows, cols, r, c, gx, gy);
            Ix2 += gx * gx;
            Iy2 += gy * gy;
            IxIy += gx * gy;
        }
    }
    const float det = (float)((double)Ix2 * (double)Iy2 - (double)IxIy * (double)IxIy);  // cv::determinant, :105
    const float tr = (float)(0.0 + (double)Ix2 + (double)Iy2);                            // cv::trace, :106
    return (tr * tr) / det;                                                               // :107
}

// filterKeypoints' edge rejection (:331-335): the keypoint stays iff its response is below ((r + 1)^2) / r, r = 10
__device__ __forceinline__ bool passes_edge_test(const uint8_t* __restrict__ G, int gpitch, int rows, int cols, int y, int x, int pad) {
    const float r = 10.0f, threshold = ((r + 1.0f) * (r + 1.0f)) / r;  // :331-332
    return edge_response_u8(G, gpitch, rows, cols, y, x, pad) < threshold;  // :335
}

// Sobel (ksize 1) gradient of an interior pixel from a staged u8 patch: c0 = the pixel's byte, pb = bytes per patch row
__device__ __forceinline__ void patch_gradient(const uint8_t* c0, int pb, float& gx, float& gy) {
    gx = (float)((int)c0[1] - (int)c0[-1]), gy = (float)((int)c0[pb] - (int)c0[-pb]);
}

// cv::magnitude of the level's Sobel gradients at one pixel (processGradients, GaussPyramid.cpp:65-104)
__device__ __forceinline__ float magnitude_at(const uint8_t* __restrict__ G, int gpitch, int rows, int cols, int r, int c) {
    float x, y;
    gradient_at(G, gpitch, rows, cols, r, c, x, y);
    return gradient_magnitude(x, y);
}

// Symmetric column pass of window pixel (i, j) over the row-filtered strip rb[16 + 2R][16], taps kl[2R + 1]:
// s = k[R] * S(0); s += k[R + t] * (S(+t) + S(-t))
template <bool FMA>
__device__ __forceinline__ float column_pass_sym(const float* kl, const float* rb, int R, int i, int j) {
    float s0 = kl[R] * rb[(i + R) * OR_WIN + j];
#pragma unroll 4
    for (int t = 1; t <= R; ++t) s0 = mad_f32<FMA>(kl[R + t], rb[(i + R + t) * OR_WIN + j] + rb[(i + R - t) * OR_WIN + j], s0);
    return s0;
}

// Lane B of the wave gets the 64-bit mask of the lanes whose bin is B (bins 0..63) from the six ballots of the bin
// index's bit planes: mask = AND_k (plane_k XOR (bit k of B ? 0 : ~0)).  12 + 22 instructions for the wave.
// nsel[k] = the lane's own (bit k of lane ? 0 : ~0), formed once per kernel (bin_plane_selectors).
__device__ __forceinline__ void bin_plane_selectors(int lane, unsigned int (&nsel)[6]) {
#pragma unroll
    for (int b = 0; b < 6; ++b) nsel[b] = ((lane >> b) & 1) ? 0u : ~0u;
}
__device__ __forceinline__ void bin_masks_from_planes(int mybin, const unsigned int (&nsel)[6], unsigned int& lo, unsigned int& hi) {
    lo = hi = ~0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned long long plane = __ballot((mybin >> k) & 1);
        lo &= (unsigned int)plane ^ nsel[k];
        hi &= (unsigned int)(plane >> 32) ^ nsel[k];
    }
}

// A 256-thread workgroup's bin masks, binmask[bin][wave]: every wave ballots its 64 pixels (thread = window pixel, bin_of = its
// histogram bin) and the bin's lane stores the wave's mask
__device__ __forceinline__ void store_bin_masks(unsigned long long (*binmask)[4], int bin_of, const unsigned int (&nsel)[6]) {
    unsigned int mlo, mhi;
    bin_masks_from_planes(bin_of, nsel, mlo, mhi);
    if ((threadIdx.x & 63) < OR_BINS) binmask[threadIdx.x & 63][threadIdx.x >> 6] = ((unsigned long long)mhi << 32) | mlo;
}

// Histogram and peaks of one window (:112-133, :352-366), by ONE wave, lane = bin: a bin's magnitudes are added in pixel order
// (binmask[4 bin + w] = the pixels 64 w .. 64 w + 63 that fall into the bin; ascending bit = ascending pixel index), the 36 sums
// sit in lanes 0..35, so the maximum and the peak test need no pass through LDS.  Returns the 36-bit mask of the peaks.
__device__ __forceinline__ unsigned long long peak_mask(const unsigned long long* binmask, const float* mw, int lane) {
    float h = 0.0f;
    if (lane < OR_BINS) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned long long m = binmask[lane * 4 + w];
            while (m) {
                h += mw[64 * w + __builtin_ctzll(m)];
                m &= m - 1;
            }
        }
    }
    float mx = lane < OR_BINS ? h : 0.0f;  // sums of non-negative weights: 0 is neutral, and bin 0 is among them
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float peakThreshold = mx * 0.8f;                 // :358
    const bool peak = lane < OR_BINS && h > peakThreshold;  // :362
    return __ballot(peak);
}

// grid = (keypoints), 256 threads, dynamic LDS = orient_lds_bytes(max R).  FMA: the filter's multiply-adds fused (mad_f32).
template <bool FMA>
__global__ __launch_bounds__(256) void k_orient_keypoints(const vslam_point* __restrict__ kps, int n, OrientLevels lv, int gpitch, int rows, int cols,
                                                           unsigned long long* __restrict__ masks) {
    extern __shared__ __attribute__((aligned(16))) float orient_smem[];
    __shared__ float mw[OR_WIN * OR_WIN];
    __shared__ unsigned long long binmask[OR_BINS][4];  // per bin, per wave: the wave's pixels that fall into it
    __shared__ int keep_s;
    const int q = blockIdx.x;
    const vslam_point kp = kps[q];
    const int x = kp.col, y = kp.row, level = kp.level;
    if (threadIdx.x == 0) keep_s = passes_edge_test(lv.gauss[level], gpitch, rows, cols, y, x, kp.padding);
    __syncthreads();
    if (!keep_s) {
        if (threadIdx.x == 0) masks[q] = 0ull;
        return;
    }
    const int kn = lv.kn[level], R = kn >> 1;
    const float* __restrict__ k = lv.kern[level];
    const float* __restrict__ M = lv.mag[level];
    const int prows = rows + 2 * OR_PAD, pcols = cols + 2 * OR_PAD;
    const int span = OR_WIN + 2 * R;
    float* rb = orient_smem;                                  // [span][16] row-filtered strip
    int* cx = reinterpret_cast<int*>(orient_smem + span * OR_WIN);  // [span] source column of padded column x - R + i
    float* kl = orient_smem + span * OR_WIN + span;                 // [span >= kn] the taps: from LDS, not from memory, inside the filter loops
    for (int i = threadIdx.x; i < span; i += 256) {
        cx[i] = clampi(reflect101(x + i - R, pcols) - OR_PAD, 0, cols - 1);
        if (i < kn) kl[i] = k[i];
    }
    __syncthreads();
    for (int it = threadIdx.x; it < span * OR_WIN; it += 256) {
        const int rr = it >> 4, c = it & 15;
        const int sy = clampi(reflect101(y + rr - R, prows) - OR_PAD, 0, rows - 1);  // padOctave = replicate
        const float* __restrict__ S = M + (size_t)sy * cols;
        float s0 = kl[0] * S[cx[c]];
#pragma unroll 4
        for (int i = 1; i < kn; ++i) s0 = mad_f32<FMA>(kl[i], S[cx[c + i]], s0);
        rb[it] = s0;
    }
    __syncthreads();
    unsigned int nsel[6];
    bin_plane_selectors(threadIdx.x & 63, nsel);
    {
        const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
        mw[threadIdx.x] = column_pass_sym<FMA>(kl, rb, R, i, j);
        const float o = lv.orient[level][(size_t)clampi(y + i - OR_PAD, 0, rows - 1) * cols + clampi(x + j - OR_PAD, 0, cols - 1)];
        store_bin_masks(binmask, hist_bin<OR_BINS>(o), nsel);  // fastAtan2 on integer gradients stays below 359.8
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const unsigned long long m = peak_mask(&binmask[0][0], mw, threadIdx.x);
        if (threadIdx.x == 0) masks[q] = m;
    }
}

static inline size_t orient_lds_bytes(int R) { return (size_t)(OR_WIN + 2 * R) * OR_WIN * 4 + (size_t)(OR_WIN + 2 * R) * 8; }  // strip + column map + taps

// StructureMatrix (Harris_corners.cpp:10-29) / computeEdgeResponse (Diff_of_Gauss.cpp:79-109) on
// caller-gathered windows (the per-point C++ entry points): gxw / gyw hold n windows of `elems`
// gradient values in the reference's loop order.  sums (may be null): n x (Ix2, IxIy, Iy2), the
// entries of M; response (may be null): tr^2 / det.
__global__ __launch_bounds__(256) void k_edge_response_windows(const float* __restrict__ gxw, const float* __restrict__ gyw, int elems,
                                                                int n, float* __restrict__ sums, float* __restrict__ response) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float Ix2 = 0.f, Iy2 = 0.f, IxIy = 0.f;
    for (int e = 0; e < elems; ++e) {
        const float gx = gxw[(size_t)i * elems + e], gy = gyw[(size_t)i * elems + e];
        Ix2 += gx * gx;
        Iy2 += gy * gy;
        IxIy += gx * gy;
    }
    if (sums) sums[3 * (size_t)i] = Ix2, sums[3 * (size_t)i + 1] = IxIy, sums[3 * (size_t)i + 2] = Iy2;
    if (response) {
        const float det = (float)((double)Ix2 * (double)Iy2 - (double)IxIy * (double)IxIy);
        const float tr = (float)(0.0 + (double)Ix2 + (double)Iy2);
        response[i] = (tr * tr) / det;
    }
}

}  // namespace vslam
