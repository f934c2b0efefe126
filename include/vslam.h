/*
 * vslam.h -- C ABI of the MI355X-native keypoint-detection front end.
 *
 * The reference (JacobYoung115/VisualSLAM, KeyPointDetection/) has no FFI layer: its hot
 * path is plain C++ functions over cv::Mat.  This header is the
 * drop-in boundary a maintainer binds instead: every entry point names the reference
 * function / OpenCV call site it replaces (paths relative to KeyPointDetection/).
 * The C++ mirror of the reference signatures (HarrisCorner, NMS2, GaussPyramid,
 * initialKeypointDetection ...) sits on top of this ABI in visualslam_amd/cxx/.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, int status return (0 = VSLAM_OK, negative =
 *     error); no exceptions cross the ABI; vslam_last_error(ctx) gives the message.
 *   - Images are row-major, `step` = bytes between rows (cv::Mat::step).
 *   - "host" entry points take host pointers, copy in/out and are synchronous.
 *     "_dev" entry points take DEVICE pointers, are asynchronous on the context's HIP
 *     stream and never synchronise: they are the path bench.py measures.
 *   - One context per GPU/stream.  A context is not thread-safe; distinct contexts are
 *     independent.  All kernels are hand-written HIP for gfx950; there is no CPU
 *     fallback: without a GPU every compute entry point fails with VSLAM_ERR_HIP.
 *   - Semantics ("intended" vs "literal" for the reference's defects) follow SURVEY.md
 *     Appendix B and are restated per function below.
 */
#ifndef VSLAM_H
#define VSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_VERSION 200 /* 0.2.0: vslam_batch_out carries buffer sizes (round 3) */

enum {
    VSLAM_OK = 0,
    VSLAM_ERR_INVALID = -1,     /* bad argument (null pointer, non-positive size, even window ...) */
    VSLAM_ERR_HIP = -2,         /* a HIP runtime call or kernel launch failed (incl. no GPU) */
    VSLAM_ERR_NOMEM = -3,       /* device or host allocation failed */
    VSLAM_ERR_UNSUPPORTED = -4, /* parameter combination not implemented */
    VSLAM_ERR_RANGE = -5        /* octave / level index out of range */
};

#define VSLAM_MAX_OCTAVES 16
#define VSLAM_NUM_LEVELS 6 /* scaleSamples_ + 3, include/src/GaussPyramid/GaussPyramid.hpp:65-66 */
#define VSLAM_NUM_DOGS 5   /* include/src/GaussPyramid/GaussPyramid.cpp:193 */

typedef struct vslam_ctx vslam_ctx;
typedef struct vslam_pyramid vslam_pyramid;

/* Binary-compatible with SLAM::point (Diff_of_Gauss.cpp:27-35): six ints, 24 bytes.
 * row/col are in 1-padded coordinates exactly as the reference produces them (:289). */
typedef struct {
    int32_t row, col, value, padding, octave, level;
} vslam_point;

/* Harris keypoint: NMS2 survivor whose 8-bit view exceeds 253 (Harris_corners.cpp:139,181). */
typedef struct {
    int32_t row, col;
    float response;
} vslam_kp;

/* ---------------------------------------------------------------- lifecycle */

int vslam_version(void);
const char* vslam_status_string(int status);

/* device: HIP device ordinal.
 * stream: the hipStream_t every call of this context is enqueued on:
 *   - a stream handle of the caller: work is ordered with whatever else the caller enqueues there;
 *   - VSLAM_STREAM_LEGACY: the device's legacy NULL stream (the library then launches on stream 0).
 *     A caller whose own work runs on the NULL stream (handle 0, e.g. torch's default stream) must
 *     pass THIS, not NULL;
 *   - NULL: the context creates and owns a non-blocking stream.  It is NOT ordered against the NULL
 *     stream or any other stream: device buffers handed to vslam_detect_batch_dev must be complete
 *     before the call, and its results are complete only after vslam_ctx_sync.
 * The batched path forks internal side streams from this stream and joins them back before it
 * returns, so ordering on this stream covers all of its work. */
#define VSLAM_STREAM_LEGACY ((void*)1)
int vslam_ctx_create(int device, void* stream, vslam_ctx** out);
int vslam_ctx_destroy(vslam_ctx* ctx);
int vslam_ctx_sync(vslam_ctx* ctx);
/* The batched path runs its Harris chain and its scans / lists on two side streams.  When those YIELD to the octave kernels
 * (lowest stream priority, vslam_ctx_set_side_stream_priority below) HIP's choice of hardware queue decides how they fare:
 * on an unlucky queue they crawl (up to -20 %).  A host that wants the library to look for a better
 * pair of yielding streams opts in with vslam_ctx_tune_side_streams(ctx, 1) BEFORE the context's first batch call
 * (VSLAM_ERR_UNSUPPORTED afterwards; off by default; VSLAM_STREAM_TUNER=1 does the same for contexts created afterwards).
 * Opting in also selects yielding side streams (as set_side_stream_priority(ctx, 1) would), unless a level has been pinned:
 * at any other level there is nothing to compare, the tuner ends at its first call (state 2, pair 0) and the join watchdog
 * below runs as usual.  The context then times its 2nd to 5th full-size batch call of one shape on three candidate pairs of
 * side streams and adopts the fastest at the first later call that finds those calls finished (an event query: no call
 * ever waits on the host, and nothing is timed while the context's stream is being captured; results never depend on the
 * pair); the join watchdog starts once the comparison has ended.
 * vslam_ctx_side_stream_report: the index of the pair in use (0 = the first created) and the state of the comparison
 * (0 off or not started, 1 measuring, 2 decided).  Diagnostic only. */
int vslam_ctx_tune_side_streams(vslam_ctx* ctx, int on);
/* Priority of the batched path's two side streams (Harris chain; scans and lists).  Default (low = 0): the context stream's
 * own priority - within 3.5 % of the best schedule for every hardware-queue layout measured.  low = 1:
 * the device's LOWEST priority, so that the side work yields to the octave kernels - 2-3 % faster when every stream has a
 * hardware queue to itself, up to 18 % slower when one does not: for a host that controls GPU_MAX_HW_QUEUES and its own
 * stream count (vslam::BatchDetector::Options::yielding_side_streams; Stream's host-fed mode).  Before the context's first
 * batch call only (VSLAM_ERR_UNSUPPORTED afterwards); VSLAM_SIDE_PRIORITY=low|main sets the default of new contexts.
 * Results never depend on it. */
int vslam_ctx_set_side_stream_priority(vslam_ctx* ctx, int low);
/* Always on (VSLAM_JOIN_WATCH=0 disables; idle while a comparison of the tuner above runs and during stream captures):
 * the first full-size batch calls of a context measure how long the context's stream waits at the end of the call for the
 * side streams (three events on the stream, read by a later call once complete - no host wait).  Three calls whose median
 * wait exceeds the level's limit (3 % of the call with yielding side streams = level 0, 10 % at the default level 1) start a
 * trial of the next level - 1: side streams at the context stream's priority, 2: side work on the context's stream itself -
 * which is kept only if its fastest call is 1 % faster than the previous level's; then the watch ends (done).  Results
 * never depend on the level.  last_lag_fraction: the most recent measurement (-1: none yet).
 * CAPTURE NOTE: the watch (like the tuner) calls hipEventQuery / hipEventElapsedTime and records timing events on the
 * context's stream.  It checks the capture status of THAT stream only: a process that captures in GLOBAL mode on another
 * stream (torch.cuda.graph's default) while this context makes un-captured batch calls should switch the watch off for the
 * context - vslam_ctx_set_join_watch(ctx, 0), or VSLAM_JOIN_WATCH=0 for every context - or pin a level. */
int vslam_ctx_join_watch_report(const vslam_ctx* ctx, int* level, int* done, float* last_lag_fraction);
/* on = 0: this context takes no more measurements and stays at its current level; on = 1 (the default) resumes. */
int vslam_ctx_set_join_watch(vslam_ctx* ctx, int on);
/* Pins the side-stream level of a context and ends its watch: 0 yielding side streams, 1 side streams at the context
 * stream's priority, 2 no side streams (every kernel of a batch call on the context's stream, in order).  Before the
 * context's first batch call only (VSLAM_ERR_UNSUPPORTED afterwards).  Results never depend on the level. */
int vslam_ctx_pin_side_streams(vslam_ctx* ctx, int level);
int vslam_ctx_side_stream_report(const vslam_ctx* ctx, int* pair, int* state);
/* Two batches in flight: a second context (own stream, own output buffers) whose batch starts when `leader`'s most
 * recent vslam_detect_batch_dev call is past its octave-0 kernels - the long, issue-bound part - instead of beside
 * them.  The coarse octaves, scans and list kernels that follow are short and leave issue slots idle; the follower's
 * octave 0 can fill them (+3..5 % frames/s measured for two contexts taking alternate batches, each following the
 * other, when their streams get hardware queues of their own; see DESIGN section 5.4 for when they do not).
 * Enqueues one event wait on ctx's stream; a no-op if the leader has not run a batch yet.
 * visualslam_amd/cxx/batch_detector.hpp (Options::pipelines) uses it. */
int vslam_ctx_follow(vslam_ctx* ctx, const vslam_ctx* leader);
/* OPT-IN, off by default (environment: VSLAM_MX=1 switches it on for every context created afterwards): the
 * Gaussian levels of the LDS-tiled octaves (GaussVector + Diff_of_Gauss, GaussPyramid.cpp:166-200) as banded
 * matrix products on the matrix cores (v_mfma_i32_32x32x32_i8) instead of packed dot instructions.  Results are
 * bit-identical (exact integer arithmetic either way); BASELINE.json's north star rules MFMA out for this path, so
 * the default, and everything bench.py reports as `value` / `roofline`, stays on the dot kernels. */
int vslam_ctx_set_matrix_path(vslam_ctx* ctx, int on);
int vslam_ctx_get_matrix_path(const vslam_ctx* ctx);
/* Which OpenCV the f32 stages reproduce bit for bit.  The reference's f32 arithmetic runs inside OpenCV: cv::phase
 * (GaussPyramid.cpp:96) and GaussianBlur on CV_32F windows (Diff_of_Gauss.cpp:348, :616-618).  OpenCV dispatches both at run
 * time: its SSE2 baseline rounds every product and sum, its AVX2 + FMA3 code fuses the multiply-adds of fastAtan32f's
 * polynomial and of the separable filter's row / column passes.  on = 0 (default): the baseline; on = 1 (environment:
 * VSLAM_F32_FUSED=1 for contexts created afterwards): the fused form - in vslam_pyramid_get_gradients' orientation image,
 * vslam_filter_keypoints, vslam_sift_descriptors and the batched orient / descriptor stages.  The CPU oracle carries the same
 * switch (vo_set_fma_variant) and the parity tests hold bit for bit under either; which one a given OpenCV build computes is
 * what tools/pin_with_opencv.sh reports.  Between the two (profiles/r06_fma_risk.json, and on the GPU at scale
 * tests/test_gpu_f32_variant.py): orientation values differ by at most one unit in the last place, no histogram bin and no
 * oriented point changes, descriptor entries differ by at most 5e-7.  The integer rows (Harris, pyramid, DoG, extrema,
 * localization) do not depend on it. */
int vslam_ctx_set_f32_fused(vslam_ctx* ctx, int on);
int vslam_ctx_get_f32_fused(const vslam_ctx* ctx);
const char* vslam_last_error(const vslam_ctx* ctx);

/* ------------------------------------------ host-side parameter helpers (no GPU) */

/* Kernel width cv::GaussianBlur derives for CV_8U when ksize = Size(0,0):
 * cvRound(sigma*6+1)|1  (call site GaussPyramid.cpp:177). */
int vslam_gauss_ksize_u8(double sigma);
/* The 8.8 fixed-point taps cv::GaussianBlur uses on CV_8U (sum == 256); taps[n]. */
int vslam_gauss_taps_q8(int n, double sigma, uint16_t* taps);
/* GaussPyramid::calculateSigma(octave, level), GaussPyramid.cpp:160-162. */
double vslam_sigma_at(double sigma0, int octave, int level);
/* GaussPyramid::calculateNumOctaves, GaussPyramid.cpp:150-152. */
int vslam_auto_num_octaves(int rows, int cols);
/* Size cv::resize(..., 0.5, 0.5, INTER_NEAREST) produces (GaussPyramid.cpp:126). */
void vslam_half_size(int rows, int cols, int* out_rows, int* out_cols);
/* Lattice of initialKeypointDetection (Diff_of_Gauss.cpp:267-268): sites
 * i = pad, pad+window, ... < rows (likewise cols). */
void vslam_extrema_lattice(int rows, int cols, int window, int* lat_rows, int* lat_cols);

/* ------------------------------------------------- host-buffer primitives (GPU) */

/* cv::GaussianBlur(src, dst, Size(ksize,ksize) or Size(0,0), sigma, 0, BORDER_DEFAULT)
 * on CV_8U: Harris_corners.cpp:158, GaussPyramid.cpp:177. */
int vslam_gaussian_blur_u8(vslam_ctx* ctx, const uint8_t* src, int rows, int cols, size_t step, int ksize,
                           double sigma, uint8_t* dst, size_t dst_step);
/* cv::Sobel(src, dst, CV_32F, dx, dy, ksize=1, 1, 0, BORDER_DEFAULT):
 * Harris_corners.cpp:163-164, GaussPyramid.cpp:87,90.  (dx,dy) = (1,0) or (0,1). */
int vslam_sobel_k1_u8_f32(vslam_ctx* ctx, const uint8_t* src, int rows, int cols, size_t step, int dx, int dy,
                          float* dst, size_t dst_step);
/* cv::resize(src, dst, Size(), 2, 2, INTER_LINEAR), GaussPyramid.cpp:110. */
int vslam_resize_linear2x_u8(vslam_ctx* ctx, const uint8_t* src, int rows, int cols, size_t step, uint8_t* dst,
                             size_t dst_step);
/* cv::resize(src, dst, Size(), 0.5, 0.5, INTER_NEAREST), GaussPyramid.cpp:126. */
int vslam_resize_nearest_half_u8(vslam_ctx* ctx, const uint8_t* src, int rows, int cols, size_t step,
                                 uint8_t* dst, size_t dst_step);
/* cv::convertScaleAbs(src f32, dst u8), Harris_corners.cpp:176,181, as the reference's x86-64 OpenCV
 * build evaluates it: round_half_even(|x|) saturated to 255 for |x| < 2^31; NaN and |x| >= 2^31 give 0
 * (cvRound = cvtss2si / cvtps2dq returns INT_MIN there and saturate_cast<uchar> maps it to 0). */
int vslam_convert_scale_abs_f32(vslam_ctx* ctx, const float* src, int rows, int cols, size_t step, uint8_t* dst,
                                size_t dst_step);

/* --------------------------------------------------------------- Harris (host) */

/* Mat HarrisCorner(Mat& Ix, Mat& Iy), Harris_corners.cpp:31-68 (with StructureMatrix
 * :10-29): arbitrary f32 gradients, literal f32 accumulation order, double determinant.
 * Intended rows x cols output (Appendix B-1).  Reference literals: k=0.04f, window=3. */
int vslam_harris_from_grad_f32(vslam_ctx* ctx, const float* ix, const float* iy, int rows, int cols,
                               size_t step, float k, int window, float* resp, size_t resp_step);
/* Front end of Harris main(): GaussianBlur 3x3 -> Sobel x,y -> HarrisCorner
 * (Harris_corners.cpp:158-172) as ONE fused kernel over the 8-bit frame. window must be 3. */
int vslam_harris_response_u8(vslam_ctx* ctx, const uint8_t* img, int rows, int cols, size_t step, float k,
                             int window, float* resp, size_t resp_step);
/* Mat NonMaximumSuppression(Mat& response, int windowSize), Harris_corners.cpp:70-81:
 * mask(255/0) = response > max(neighbours, centre excluded).  windowSize odd. */
int vslam_nms_strict_u8(vslam_ctx* ctx, const uint8_t* src, int rows, int cols, size_t step, int window,
                        uint8_t* mask, size_t mask_step);
int vslam_nms_strict_f32(vslam_ctx* ctx, const float* src, int rows, int cols, size_t step, int window,
                         uint8_t* mask, size_t mask_step);
/* Mat NMS2(Mat& response, int windowSize), Harris_corners.cpp:83-129: half-open window
 * (literal, Appendix B-4), f32 map out (intended, B-3).  true_max (may be NULL) receives
 * the value the reference prints at :127. */
int vslam_nms2_f32(vslam_ctx* ctx, const float* resp, int rows, int cols, size_t step, int window, float* out,
                   size_t out_step, float* true_max);
/* Whole Harris executable minus display: response -> NMS2(5) -> 8-bit view > 253
 * (Harris_corners.cpp:158-182).  Row-major keypoint list; *count = total found (may
 * exceed cap; only cap entries are written). */
int vslam_harris_keypoints_u8(vslam_ctx* ctx, const uint8_t* img, int rows, int cols, size_t step, float k,
                              vslam_kp* out, size_t cap, size_t* count);

/* ------------------------------------------------------------ DoG pyramid (host) */

typedef struct {
    int n_octaves;
    int n_levels; /* 6 */
    int n_dogs;   /* 5 */
    double sigma0;
    int rows[VSLAM_MAX_OCTAVES], cols[VSLAM_MAX_OCTAVES];
    double sigma[VSLAM_MAX_OCTAVES][VSLAM_NUM_LEVELS];
    int ksize[VSLAM_MAX_OCTAVES][VSLAM_NUM_LEVELS];
} vslam_pyramid_info;

/* GaussPyramid(Mat& img, int numOctaves, double sigma) -> createPyramid
 * (GaussPyramid.hpp:17, GaussPyramid.cpp:106-131): 2x bilinear base, per octave 6
 * Gaussians (each blurred from the octave base, :166-185) and 5 saturating DoGs
 * (:191-200), next base = Gaussian[3] decimated (:123-126).  The images stay in HBM;
 * the getters copy one image to the host.  n_octaves <= 0 selects the automatic count
 * of the second constructor (GaussPyramid.hpp:18-21). */
int vslam_pyramid_build_u8(vslam_ctx* ctx, const uint8_t* img, int rows, int cols, size_t step, int n_octaves,
                           double sigma0, vslam_pyramid** out);
int vslam_pyramid_destroy(vslam_pyramid* pyr);
int vslam_pyramid_get_info(const vslam_pyramid* pyr, vslam_pyramid_info* out);
/* octaveImage / octaveBlur / octaveDiff (GaussPyramid.hpp:29,31,32). */
int vslam_pyramid_get_base(const vslam_pyramid* pyr, int octave, uint8_t* dst, size_t dst_step);
int vslam_pyramid_get_gauss(const vslam_pyramid* pyr, int octave, int level, uint8_t* dst, size_t dst_step);
int vslam_pyramid_get_dog(const vslam_pyramid* pyr, int octave, int level, uint8_t* dst, size_t dst_step);

/* GaussPyramid::processGradients for one Gaussian level (GaussPyramid.cpp:65-104; getters
 * octaveGradX / octaveGradY / octaveGradMag / octaveGradOrient, GaussPyramid.hpp:33-36):
 * Sobel x, Sobel y (ksize 1), cv::magnitude, cv::phase in degrees (OpenCV's fastAtan2
 * polynomial, ~0.01 deg from atan2).  Computed on demand from the HBM-resident Gaussian
 * (the reference materialises all 96 bytes per pyramid pixel in its constructor).  Any of the
 * four CV_32F destinations may be NULL; dst_step in bytes. */
int vslam_pyramid_get_gradients(const vslam_pyramid* pyr, int octave, int level, float* grad_x, float* grad_y,
                                float* mag, float* orient, size_t dst_step);

/* void initialKeypointDetection(vector<SLAM::point>&, GaussPyramid&, int octave, int
 * windowSize), Diff_of_Gauss.cpp:254-297, up to the FeaturePointLocalization call.
 * Literal stride-`window` lattice and half-open window (Appendix B-7), padded
 * coordinates (B-8).
 *   bits (may be NULL): candidate bitmask, 3 levels x lat_rows x words_per_row uint64
 *     words, words_per_row = (lat_cols+63)/64, bit (lj & 63) of word
 *     [((level-1)*lat_rows + li)*words_per_row + lj/64].
 *   out/cap/count: candidates with value >= min_contrast in the reference's loop order
 *     (level, i, j); *count = total (may exceed cap). */
int vslam_dog_extrema(vslam_ctx* ctx, const vslam_pyramid* pyr, int octave, int window, int min_contrast,
                      uint64_t* bits, vslam_point* out, size_t cap, size_t* count);

/* EXTENSION, not a reference function (note under the table): the dense
 * 3x3x3 scale-space test the north star's wording names.  The rule of Diff_of_Gauss.cpp:282-287
 * (candidate iff the value equals the minimum or the maximum of its window, ties included) and the
 * replicate border of padOctave (:260), applied to EVERY pixel of DoG levels 1..3 with the full
 * 3x3x3 neighbourhood (the reference tests a half-open 2x2x3 window on a stride-3 lattice:
 * vslam_dog_extrema above is that, and is what parity is judged on).
 *   bits (may be NULL): 3 levels x rows x words_per_row uint64 words, words_per_row = (cols+63)/64,
 *     bit (x & 63) of word [((level-1)*rows + y)*words_per_row + x/64].
 *   out/cap/count: candidates with value >= min_contrast in (level, y, x) order as
 *     SLAM::point(y+1, x+1, value, 1, octave, level) - padded coordinates like :289;
 *     *count = total (may exceed cap). */
int vslam_dog_extrema_dense(vslam_ctx* ctx, const vslam_pyramid* pyr, int octave, int min_contrast, uint64_t* bits,
                            vslam_point* out, size_t cap, size_t* count);

/* The same function through its call to FeaturePointLocalization (Diff_of_Gauss.cpp:290,
 * :223-251): exactly the points the reference appends to `keypoints`, in its order, with the
 * value rewritten at :246.  The contrast test is evaluated for EVERY candidate with the
 * reference's own arithmetic (A*A^T is singular; cv::invert's closed form decides, see
 * kernels_localize.hip.h) - no min_contrast shortcut. */
int vslam_dog_keypoints(vslam_ctx* ctx, const vslam_pyramid* pyr, int octave, int window, vslam_point* out,
                        size_t cap, size_t* count);
/* bool FeaturePointLocalization(vector<Mat>& dogs_padded, vector<SLAM::point>&, int level,
 * SLAM::point&), Diff_of_Gauss.cpp:223-251, for n independent candidates.  diffs = n x
 * (d_x, d_y, d_scale, value) as read at :226-228 and from point.value; keep[i] = the function's
 * return value, value[i] = point.value afterwards (unchanged when not kept). */
int vslam_localize_points(vslam_ctx* ctx, const int* diffs, size_t n, int* keep, int* value);

/* void filterKeypoints(GaussPyramid&, int octave, vector<SLAM::point>& keypoints,
 * vector<SLAM::point>& reducedKeypoints), Diff_of_Gauss.cpp:301-372, with computeEdgeResponse
 * (:79-109) and orientationHistogram (:112-133): edge rejection tr^2/det < 12.1 on the level's
 * Sobel gradients, then the 36-bin histogram of the 16x16 window of the 8-padded magnitude /
 * orientation images, magnitudes weighted by GaussianBlur(sigma = 1.5 * sigma(octave, level))
 * evaluated as the reference does on a non-isolated ROI (parent pixels, reflect-101 at the
 * parent's edge).  kps: the octave's keypoints (vslam_dog_keypoints output: 1-padded
 * coordinates, level 1..3).  out: one SLAM::point{row, col, angle = bin*10, 0, octave, level}
 * per histogram bin above 0.8 * max, in keypoint order then ascending bin.  *count = total
 * (may exceed cap).  A keypoint the reference would throw on (level outside 0..5, window
 * outside the padded image, other octave) gives VSLAM_ERR_RANGE. */
int vslam_filter_keypoints(vslam_ctx* ctx, const vslam_pyramid* pyr, int octave, const vslam_point* kps, size_t n,
                           vslam_point* out, size_t cap, size_t* count);
/* float computeEdgeResponse(const SLAM::point&, const Mat& grad_x, const Mat& grad_y),
 * Diff_of_Gauss.cpp:79-109, for n points whose gradient windows the caller has gathered in the
 * reference's loop order (:93-94): gx_windows / gy_windows = n x window_elems f32. */
int vslam_edge_response_windows(vslam_ctx* ctx, const float* gx_windows, const float* gy_windows, int window_elems,
                                size_t n, float* response);

/* void StructureMatrix(Mat& M, Mat& Ix, Mat& Iy, int padding, int i, int j), Harris_corners.cpp:10-29,
 * for n pixels whose (2*padding+1)^2 gradient windows the caller has gathered in the
 * reference's loop order (:16-17): sums = n x (Ix2, IxIy, Iy2) = M(0,0), M(0,1) = M(1,0), M(1,1). */
int vslam_structure_matrix_windows(vslam_ctx* ctx, const float* gx_windows, const float* gy_windows, int window_elems,
                                   size_t n, float* sums);

/* ------------------------------------------- SIFT descriptor stage (host buffers) */

/* const Point2f Rotation::cos_sin_of_angle(float theta, bool degrees = true), rotation.cpp:9-17, with
 * convertToRadians (:5-7): theta * (CV_PI / 180.0f) in double, narrowed to float, cos / sin of it
 * (host libm, like the reference).  Pure host computation. */
void vslam_cos_sin_deg(float theta_deg, float* cos_out, float* sin_out);
/* std::vector<Point2i> Rotation::getRotatedWindowPoints(Mat& I, const Point2i& center, int windowSize,
 * float theta, bool degrees = true), rotation.cpp:112-130 (with rotate_pt_CW :19-27): the
 * (windowSize+1)^2 points of the square around `center` rotated clockwise, rows outer;
 * xy[2q] = x, xy[2q+1] = y.  The Mat argument of the reference is unused.  Pure host computation. */
int vslam_rotated_window_points(int cx, int cy, int window, float theta_deg, int32_t* xy);
/* void SIFT(vector<SLAM::point>& reducedKeypoints, vector<vector<float>>& featureDescriptors_vec,
 * GaussPyramid&, int octave), Diff_of_Gauss.cpp:561-693, with rotateImageSection (:528-559): one
 * 128-float descriptor per oriented keypoint of the octave (vslam_filter_keypoints output: value =
 * angle in degrees), desc = n x 128.  Literal reference behaviour, including the stride-16 walk of
 * the 17 x 17 point list (:545) and Mat::at<>(point.x, point.y) with x as the ROW (:549-554) on the
 * 20-padded level images.  Mat::at checks nothing, so a sample is linear element
 * x * (cols + 40) + y of the padded Mat; a keypoint whose 256 samples all lie inside that buffer is
 * DEFINED (always the case for square and portrait octaves away from the last rows), otherwise the
 * reference reads foreign memory: defined[k] = 0 and a zero descriptor.  defined may be NULL, in
 * which case any undefined keypoint makes the call return VSLAM_ERR_RANGE (after filling desc).
 * A flat window gives the reference's all-NaN descriptor (0 / 0 at :661).
 * Histogram bins: the reference indexes histo.at((int)(orientation * 8/360.f)) (:126), which throws for
 * an orientation of exactly 360.0; the kernels clamp the bin to 0..7 instead.  The gradients here come
 * from integer Sobel differences, for which cv::phase never returns 360.0, so the two agree on every
 * input this entry point can be given; the clamp only keeps an impossible value from indexing outside LDS. */
int vslam_sift_descriptors(vslam_ctx* ctx, const vslam_pyramid* pyr, int octave, const vslam_point* oriented, size_t n,
                           float* desc, uint8_t* defined);
/* featureDescriptors.dat, Diff_of_Gauss.cpp:837-863: int32 {n, 128, 24} (24 = sizeof(std::vector<float>)
 * on LP64, what `sizeof(featureDescriptors_vec.front())` writes) followed by n x 128 float32,
 * native byte order.  Pure host computation. */
int vslam_descriptor_file_write(const char* path, const float* desc, size_t n);

/* ------------------------------------------- device-resident batched detection */

typedef struct {
    int rows, cols;      /* frame size */
    int n_octaves;       /* DoG octaves (reference literal 4, Diff_of_Gauss.cpp:742); 0 = no DoG */
    double sigma0;       /* 1.6, Diff_of_Gauss.cpp:743 */
    float harris_k;      /* 0.04f, Harris_corners.cpp:36 */
    int do_harris;       /* run the Harris path */
    int extrema_window;  /* 3, Diff_of_Gauss.cpp:772 */
    int min_contrast;    /* list threshold on the 8-bit DoG value; 8 */
    int localize;        /* 1: dog_points = FeaturePointLocalization survivors (vslam_dog_keypoints),
                          * min_contrast unused; 0 (default): candidates with value >= min_contrast */
    int orient;          /* 1: also run filterKeypoints (Diff_of_Gauss.cpp:301-372) on every frame's
                          * keypoint list -> oriented_points / oriented_counts; needs localize = 1 */
    uint32_t harris_cap; /* per-frame capacity of the Harris keypoint list */
    uint32_t dog_cap;    /* per-frame capacity of the DoG point list */
    uint32_t oriented_cap; /* per-frame capacity of the oriented keypoint list (and of the
                            * edge-test survivors it is made from) */
    int extrema_dense;   /* EXTENSION (0 = the reference's lattice test, the default and the parity path): 1 runs the
                          * dense 3x3x3 scale-space test of vslam_dog_extrema_dense on every pixel of DoG levels 1..3
                          * of every frame instead.  extrema_bits then holds, per octave, 3 levels x rows x
                          * ceil(cols/64) words (layout.lat_rows / lat_cols / lat_words report rows / cols / words per
                          * row) and dog_points the candidates with value >= min_contrast in (octave, level, y, x)
                          * order.  Needs extrema_window = 3, localize = 0, orient = 0. */
} vslam_params;

/* Byte layout of the per-frame output blocks, so that a caller can allocate them. */
typedef struct {
    int n_octaves;
    int rows[VSLAM_MAX_OCTAVES], cols[VSLAM_MAX_OCTAVES];
    int lat_rows[VSLAM_MAX_OCTAVES], lat_cols[VSLAM_MAX_OCTAVES], lat_words[VSLAM_MAX_OCTAVES];
    /* pyramid block of one frame: for octave o, Gaussian l at octave_offset[o] + l*P_o and
     * DoG l at octave_offset[o] + (6+l)*P_o, P_o = rows[o]*pitch[o]; row r of a plane starts at
     * r*pitch[o].  pitch[o] = cols[o] rounded up to a multiple of 16 (so it equals cols[o] for the
     * usual frame sizes); the padding bytes are unspecified. */
    int pitch[VSLAM_MAX_OCTAVES];
    size_t octave_offset[VSLAM_MAX_OCTAVES];
    size_t pyramid_frame_bytes;
    /* candidate bitmask block of one frame: octave o starts at word bits_offset[o] */
    size_t bits_offset[VSLAM_MAX_OCTAVES];
    size_t bits_frame_words;
    /* algorithmic HBM bytes per frame: input + response + mask +
     * Gaussian and DoG stacks */
    size_t algorithmic_bytes_harris, algorithmic_bytes_dog;
} vslam_batch_layout;

/* Device pointers; any may be NULL to skip that output (it is then neither computed for its own sake
 * nor written).  Every pointer travels with the size of the buffer behind it: `x_bytes` is the number of
 * bytes the caller allocated at `x`.  vslam_detect_batch_dev checks each non-NULL buffer against what
 * n_frames frames need (vslam_batch_out_required fills in exactly those numbers) and returns
 * VSLAM_ERR_INVALID - before anything is launched - if one is too small or struct_size is not
 * sizeof(vslam_batch_out); a kernel never writes past a size stated here. */
typedef struct {
    size_t struct_size;      /* = sizeof(vslam_batch_out) */
    float* response;         /* [n][rows][cols]  HarrisCorner output */
    size_t response_bytes;
    uint8_t* nms_mask;       /* [n][rows][cols]  NonMaximumSuppression(8-bit view, 3) */
    size_t nms_mask_bytes;
    float* nms2;             /* [n][rows][cols]  NMS2(response, 5) map (optional) */
    size_t nms2_bytes;
    vslam_kp* harris_kps;    /* [n][harris_cap] */
    size_t harris_kps_bytes;
    uint32_t* harris_counts; /* [n] totals (may exceed cap) */
    size_t harris_counts_bytes;
    uint8_t* pyramid;        /* [n][pyramid_frame_bytes], 16-byte aligned, planes pitched (layout.pitch) */
    size_t pyramid_bytes;
    uint64_t* extrema_bits;  /* [n][bits_frame_words] */
    size_t extrema_bits_bytes;
    vslam_point* dog_points; /* [n][dog_cap], order (octave, level, i, j) */
    size_t dog_points_bytes;
    uint32_t* dog_counts;    /* [n] totals (may exceed cap) */
    size_t dog_counts_bytes;
    vslam_point* oriented_points; /* [n][oriented_cap] filterKeypoints output: {row, col, angle, 0, octave, level},
                                   * order (octave, keypoint, histogram bin); params.orient = 1 */
    size_t oriented_points_bytes;
    uint32_t* oriented_counts;    /* [n] oriented points of the EVALUATED survivors (may exceed cap): the true total
                                   * iff oriented_survivors[f] <= oriented_cap */
    size_t oriented_counts_bytes;
    uint32_t* oriented_survivors; /* [n] optional: keypoints of the frame that pass the edge test (Diff_of_Gauss.cpp:336).
                                   * Only the first oriented_cap of them (list order) get their histogram evaluated, so
                                   * oriented_survivors[f] > oriented_cap flags a truncated frame */
    size_t oriented_survivors_bytes;
    float* descriptors;           /* [n][oriented_cap][128] optional: SIFT() descriptors (Diff_of_Gauss.cpp:561-693) of the
                                   * oriented points, same order; needs the oriented outputs.  Row q of frame f is
                                   * valid for q < min(oriented_counts[f], oriented_cap) */
    size_t descriptors_bytes;
    uint8_t* descriptor_defined;  /* [n][oriented_cap] optional, with descriptors: 0 where the rotated window leaves the
                                   * padded level (zero descriptor, see vslam_sift_descriptors) */
    size_t descriptor_defined_bytes;
} vslam_batch_out;

/* Defaults of the reference's literals; the three list capacities scale with the frame area
 * (harris_cap = dog_cap = rows*cols/8, oriented_cap = rows*cols/32, each rounded up to a multiple
 * of 4096 and not below 65536 / 65536 / 16384: 262144 / 262144 / 65536 at 1920x1080, 1040384 / 1040384 /
 * 262144 at 3840x2160). */
void vslam_params_default(vslam_params* p, int rows, int cols);
/* Pure host computation (no GPU needed). */
int vslam_batch_layout_query(const vslam_params* p, vslam_batch_layout* out);
/* Bytes each output buffer needs for n_frames frames under *p: sets struct_size and every x_bytes field
 * of *sizes (also for outputs the parameters do not produce - a buffer is only needed where its pointer
 * will be non-NULL); the pointers are left as they are.  Pure host computation. */
int vslam_batch_out_required(const vslam_params* p, int n_frames, vslam_batch_out* sizes);
/* Harris + DoG over n frames already resident in HBM (frame f at d_frames +
 * f*frame_stride, dense rows).  Asynchronous on the context stream.  This is the fused
 * path of BASELINE config 4: every frame is read from HBM once per path and every
 * output written once; frames are independent, so a multi-GPU job shards frames across
 * ranks with no data-path collective.
 * Stream capture: a call may be recorded into a hipGraph (hipStreamBeginCapture on the context's stream ... EndCapture)
 * once ONE call with the same parameters, the same batch size AND the same matrix-path setting
 * (vslam_ctx_set_matrix_path) has run outside a capture - the workspace, the blur taps (each path has its own tables) and
 * the side streams are created by the first call, and a capture can allocate nothing: a captured call that finds a table
 * missing returns VSLAM_ERR_UNSUPPORTED and launches nothing more.  The side-stream forks all start from
 * and join back to the capturing stream; the stream tuner does not time captured calls
 * (tests/test_gpu_batch.py::test_batch_call_captured_into_a_graph). */
int vslam_detect_batch_dev(vslam_ctx* ctx, const vslam_params* p, const uint8_t* d_frames, size_t frame_stride,
                           int n_frames, const vslam_batch_out* out);

/* The same detection for callers with HOST memory and no device code of their own (plain C, ctypes + numpy, ...):
 * n_frames dense frames in host memory in, the two keypoint lists out, packed frame after frame; synchronous.
 * Harris list (when p->do_harris) and DoG list (when p->n_octaves > 0; p->localize chooses candidates with value >=
 * min_contrast or FeaturePointLocalization's survivors, as in vslam_detect_batch_dev).  For each list: `x` receives
 * the records of all frames back to back (x_bytes = capacity of the caller's buffer; records beyond it are not
 * written), x_offsets[f] (n_frames + 1 entries) the record index where frame f starts, x_counts[f] the frame's true
 * total (may exceed the per-frame capacity p->harris_cap / p->dog_cap, only that many are listed).  A list whose
 * three pointers are all NULL is skipped.  The images (response, pyramid ...) stay on the device and are dropped:
 * use the per-image entry points or vslam_detect_batch_dev for them.  This is a convenience path - it allocates its
 * device buffers per call and copies over PCIe synchronously; the throughput path is vslam_detect_batch_dev
 * (visualslam_amd/cxx/batch_detector.hpp pipelines it from host memory). */
typedef struct {
    size_t struct_size; /* = sizeof(vslam_host_lists) */
    vslam_kp* harris;
    size_t harris_bytes;
    uint64_t* harris_offsets;
    uint32_t* harris_counts;
    vslam_point* dog;
    size_t dog_bytes;
    uint64_t* dog_offsets;
    uint32_t* dog_counts;
} vslam_host_lists;
int vslam_detect_batch_host(vslam_ctx* ctx, const vslam_params* p, const uint8_t* frames, size_t frame_stride, int n_frames,
                            const vslam_host_lists* out);

/* Packs the first min(counts[f], cap) records of every frame's list ([n_frames][cap] records of
 * record_bytes each: harris_kps, dog_points or oriented_points of vslam_detect_batch_dev) back to back
 * into `packed`, frame after frame, and writes offsets[f] = sum over g < f of min(counts[g], cap) for
 * f = 0..n_frames (offsets[n_frames] = total records): a host-fed caller then downloads
 * offsets[n_frames] * record_bytes bytes instead of n_frames * cap records of mostly padding.  All
 * pointers are DEVICE pointers; asynchronous on the context stream, behind the call that wrote the lists.
 * Records that do not fit packed_bytes are not written (offsets still give their positions, so
 * offsets[n_frames] * record_bytes > packed_bytes tells the caller).  record_bytes: a multiple of 4. */
int vslam_pack_lists_dev(vslam_ctx* ctx, const void* lists, size_t record_bytes, uint32_t cap, const uint32_t* counts,
                         int n_frames, void* packed, size_t packed_bytes, uint64_t* offsets);

/* The same for SLAM::point lists (dog_points, oriented_points) with every record squeezed from 24 to 16 bytes on the way:
 * a host-fed caller downloads a third fewer bytes (the lists are what saturates PCIe on the batched path).  Lossless for
 * what the detector writes: `padding` is 0 or 1, `octave` < VSLAM_MAX_OCTAVES, `level` < 6 - the three small fields share
 * one word, tag = level | octave << 8 | padding << 16.  vslam_points16_expand (host, pure arithmetic) is the inverse:
 * expand(pack(list)) is byte-identical to the list (tests/test_gpu_batch.py::test_pack_points16).  packed_bytes counts
 * bytes of `packed`; records that do not fit are not written, offsets are as for vslam_pack_lists_dev.  `lists` 8-byte,
 * `packed` 16-byte aligned (VSLAM_ERR_INVALID otherwise: the records move as 8- and 16-byte words). */
typedef struct {
    int32_t row, col, value;
    uint32_t tag; /* level | octave << 8 | padding << 16 */
} vslam_point16;
int vslam_pack_points16_dev(vslam_ctx* ctx, const vslam_point* lists, uint32_t cap, const uint32_t* counts, int n_frames,
                            vslam_point16* packed, size_t packed_bytes, uint64_t* offsets);
/* Host: out[i] = the SLAM::point of in[i], i < n (no GPU involved). */
void vslam_points16_expand(const vslam_point16* in, size_t n, vslam_point* out);

/* The sending side of the one collective of the multi-GPU path: totals[0] = sum of
 * harris_counts[0..n_frames), totals[1] = the same for dog_counts (either list may be NULL -> 0), as two
 * uint64 in DEVICE memory, asynchronous on the context stream - so that the rank's {harris, dog} pair
 * can go into ncclAllGather on the same stream without a host round trip. */
int vslam_count_totals_dev(vslam_ctx* ctx, const uint32_t* harris_counts, const uint32_t* dog_counts, int n_frames,
                           uint64_t* totals);

/* ---------------------------------------------------------------- descriptor matching
 * The step the reference stops short of (Diff_of_Gauss.cpp:687: "final step is graphing and comparing two images with each
 * other"; its README's step 2, "Feature description / Image Matching"): for every query descriptor the nearest and the
 * second-nearest train descriptor by squared Euclidean distance, and Lowe's ratio test on the two.  The search is exact,
 * and its arithmetic is fixed here so that a CPU can restate it bit for bit (tests/matchref.py):
 *   s(a, b)  = acc = +0.0f; acc = fmaf(a[k], b[k], acc) for k = 0 .. 127 ascending  (what v_mfma_f32_32x32x2_f32 computes)
 *   n(a)     = s(a, a)
 *   d2(a, b) = (n(a) + n(b)) - 2 s(a, b) in f32: the sum rounded, the doubling exact, the difference rounded.
 * d2 is a pure function of the two rows and is stored as computed, WITHOUT a clamp: d2(a, a) is exactly 0, but for two
 * nearly identical rows it can be slightly NEGATIVE.  Rows may hold any f32 value - subnormals, infinities, NaN, either zero:
 * the chains are IEEE (no flush to zero), and a distance of +inf or NaN never wins (a query row with no other distance gets
 * {-1, +inf, +inf}).  -inf CAN occur - nearly identical rows whose norms are each about 2^127: n(a) + n(b) still rounds to a finite
 * value, 2 s to +inf - and it wins and is accepted like any smaller value.
 * Selection for one query row over the train rows j = 0 .. nt-1 ascending: best = second = +inf, index = -1; if d2 < best
 * then second = best, best = d2, index = j; otherwise if d2 < second then second = d2.  Ties keep the lowest index, a NaN
 * distance never wins, and two equal minima give second_dist2 == dist2.  Skipped: a train row whose `defined` byte is 0,
 * and with same_octave a train row whose points[j].octave differs from the query's.  A query row whose `defined` byte is 0
 * gets {-1, +inf, +inf}.  A query is ACCEPTED iff index >= 0 and (second == +inf or best < ratio2 * second), the product
 * rounded once to f32.  Results depend neither on vslam_ctx_set_f32_fused nor on vslam_ctx_set_matrix_path. */
typedef struct {
    int32_t index; /* train row, -1: none */
    float dist2, second_dist2;
} vslam_nn2;
typedef struct {
    int32_t query, train;
    float dist2;
} vslam_match;
/* n sets of descriptor rows, DEVICE pointers, set j at j * cap rows: exactly the descriptors / descriptor_defined /
 * oriented_points / oriented_counts buffers of vslam_detect_batch_dev with cap = oriented_cap. */
typedef struct {
    const float* desc;         /* [n][cap][128], 16-byte aligned */
    const uint8_t* defined;    /* [n][cap], NULL = all defined */
    const vslam_point* points; /* [n][cap], required with same_octave, else may be NULL */
    const uint32_t* counts;    /* [n] on the device; rows in use = min(counts[j], cap) */
    uint32_t cap;
} vslam_desc_sets;
/* Like vslam_batch_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;     /* = sizeof(vslam_match_out) */
    vslam_nn2* nn;          /* [n_pairs][query.cap] optional; rows past a set's count are left untouched */
    size_t nn_bytes;
    vslam_match* matches;   /* [n_pairs][match_cap] optional, needs match_counts: the accepted queries, ascending query order */
    size_t matches_bytes;
    uint32_t* match_counts; /* [n_pairs] totals (may exceed match_cap) */
    size_t match_counts_bytes;
    uint32_t match_cap;
} vslam_match_out;
/* Pair j matches set j of `query` against set j of `train`, j < n_pairs (at most 65535; 0 does nothing).  Consecutive frames
 * of a batch: train = query advanced by one set, n_pairs = n - 1; the seam between two batches is a one-pair call.
 * Asynchronous on the context stream, never waits on the host (the counts are read on the device); scratch belongs to the
 * context and is sized from the capacities before the launches.  ratio2: the SQUARED ratio of Lowe's test (0.64 for 0.8).
 * VSLAM_ERR_INVALID before any launch - and before the context is looked at - for a null struct, a wrong struct_size, an
 * undersized buffer, no output at all, matches without match_counts, same_octave without points, a misaligned desc,
 * n_pairs < 0, a ratio2 that is not finite or not positive; then VSLAM_ERR_HIP when there is no usable HIP device (no
 * context can exist there, so also with a NULL context - which is VSLAM_ERR_INVALID otherwise).  Not for stream capture. */
int vslam_match_dev(vslam_ctx* ctx, const vslam_desc_sets* query, const vslam_desc_sets* train, int n_pairs, float ratio2,
                    int same_octave, const vslam_match_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call): query [nq][128], train [nt][128];
 * *_defined ([n] bytes) and *_points ([n]) as in vslam_desc_sets (NULL = all defined / required with same_octave).
 * nn [nq] and (matches [match_cap], n_matches) are each optional; *n_matches is the total, which may exceed match_cap.
 * Errors as for vslam_match_dev. */
int vslam_match_host(vslam_ctx* ctx, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                     const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt, float ratio2,
                     int same_octave, vslam_nn2* nn, vslam_match* matches, size_t match_cap, size_t* n_matches);

/* ---------------------------------------------------------------- mutual matching
 * The cross-check of a brute-force matcher, in the matcher's own pass: besides the nearest two train rows of every query row,
 * the nearest QUERY row of every train row, and the list of the accepted queries whose train row chose them back.  d2(a, b)
 * of the descriptor matching section is symmetric bit for bit (the products commute, the chain order is the same, the sum of
 * the norms commutes), so the reverse nearest of train row t IS what vslam_match_dev(train, query) writes as nn[t].index and
 * nn[t].dist2 (tests/mutualref.py restates both forms).
 *   Forward.  nn and ACCEPTED are the descriptor matching section's, verbatim.
 *   Reverse.  For a train row t that is in use and whose `defined` byte is not 0: walk the query rows q = 0 .. nq-1 ascending,
 *     skipping a query row whose `defined` byte is 0 and, with same_octave, one whose points[q].octave differs from the train
 *     row's; best = +inf, index = -1; if d2(q, t) < best then best = d2, index = q.  Ties keep the lowest query index, a NaN or
 *     +inf distance never wins, -inf can.  An undefined train row, or one with no candidate, gets {-1, +inf}.
 *   Mutual.  Query q is MUTUAL iff it is ACCEPTED and rnn[nn[q].index].index == q.  The list holds the mutual queries as
 *     {q, nn[q].index, nn[q].dist2} in ascending query order; no train row appears twice in it.
 * There is no ratio test on the reverse side (the second nearest of a train row is not kept).  The reverse minimum is an
 * integer minimum over (ordered key of d2, q), so no bit of any output depends on scheduling, and none on
 * vslam_ctx_set_f32_fused or vslam_ctx_set_matrix_path. */
typedef struct {
    int32_t index; /* query row, -1: none (dist2 = +inf) */
    float dist2;
} vslam_rnn;
typedef struct {
    size_t struct_size;     /* = sizeof(vslam_match_mutual_out) */
    vslam_nn2* nn;          /* [n_pairs][query.cap] optional: exactly what vslam_match_dev writes */
    size_t nn_bytes;
    vslam_rnn* rnn;         /* [n_pairs][train.cap] optional; rows past a train set's count are left untouched */
    size_t rnn_bytes;
    vslam_match* matches;   /* [n_pairs][match_cap] optional, needs match_counts: the MUTUAL queries, ascending query order */
    size_t matches_bytes;
    uint32_t* match_counts; /* [n_pairs] totals of the mutual list (may exceed match_cap) */
    size_t match_counts_bytes;
    uint32_t match_cap;
} vslam_match_mutual_out;
/* Pairs, sets, ratio2, same_octave as for vslam_match_dev.  Asynchronous on the context stream, never waits on the host.
 * Scratch belongs to the context: the matcher's, plus n_pairs * train.cap * 8 bytes for the reverse table, which is preset on
 * the context stream in every call.  VSLAM_ERR_INVALID before any launch as for vslam_match_dev (no output at all: none of nn,
 * rnn, match_counts), and for an undersized rnn buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for
 * stream capture. */
int vslam_match_mutual_dev(vslam_ctx* ctx, const vslam_desc_sets* query, const vslam_desc_sets* train, int n_pairs, float ratio2,
                           int same_octave, const vslam_match_mutual_out* out);
/* One pair in HOST memory, synchronous: vslam_match_host's arguments, and rnn [nt] (optional, like nn).  The list is the
 * mutual list.  Errors as for vslam_match_mutual_dev. */
int vslam_match_mutual_host(vslam_ctx* ctx, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                            const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt, float ratio2,
                            int same_octave, vslam_nn2* nn, vslam_rnn* rnn, vslam_match* matches, size_t match_cap, size_t* n_matches);

/* ---------------------------------------------------------------- two-view geometry
 * The step after matching (the reference's README: "3. 3D Reconstruction - Epipolar Geometry"): the fundamental matrix of
 * every pair, by RANSAC over the match list vslam_match_dev wrote and the point lists vslam_detect_batch_dev wrote, and the
 * inlier subset of each list.  A fixed number of hypotheses, no adaptive stop; the least-squares refit is a stage of its own (vslam_refit_dev).  The arithmetic
 * is fixed here so that a CPU can restate it bit for bit (tests/epiref.py).  Everything is IEEE f64; every + - * / sqrt is
 * rounded on its own (no fused multiply-add); a sum of more than two terms runs left to right as written, (a + b) + c.
 *
 * Coordinates of a point p, exact:  x = (p.col - p.padding) * 2^(p.octave - 1),  y = (p.row - p.padding) * 2^(p.octave - 1)
 * (octave 0 is the 2x upsampled image).  A record is TRUSTED iff query < query_cap, train < train_cap (as unsigned) and both
 * points' octave is in 0 .. 31; a record that is not trusted is never read through, is never an inlier, and a sample that
 * contains one is invalid.  m = n_matches = min(match_counts[j], match_cap) records are considered.
 *
 * Sampling, a counter hash without state.  mix(x) on uint32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
 * x ^= x >> 16.  Pair j, hypothesis h: base = mix(mix(seed + j) + h); draw t = 0, 1, ... gives r = mix(base + t) and the index
 * (uint64(r) * m) >> 32, kept if it is not among the indices kept so far; the sample is the first 8 kept indices, in that
 * order.  Fewer than 8 after 64 draws: invalid.  m < 8: every hypothesis is invalid.
 *
 * Model from the 8 records (x, y) = query, (x', y') = train - the normalised 8-point algorithm:
 *  1. Per side: cx = (x0 + x1 + ... + x7) / 8, cy likewise; d = (r0 + r1 + ... + r7) / 8 with ri = sqrt(dx*dx + dy*dy),
 *     dx = xi - cx, dy = yi - cy; d == 0: invalid; s = 1.4142135623730951 / d; normalised point ((xi - cx) * s, (yi - cy) * s).
 *  2. Row i of the 8 x 9 matrix a, from the normalised (x, y), (x', y'): [x'*x, x'*y, x', y'*x, y'*y, y', x, y, 1].
 *  3. Gauss-Jordan with full pivoting, steps k = 0 .. 7: the pivot is the entry of largest |a[r][c]| over rows r >= k and the
 *     columns no earlier step chose, scanned r ascending, then c ascending, a later entry replacing the choice only when
 *     strictly larger than it - which starts at 0: a zero or a NaN is never chosen; no choice, or an infinite pivot: invalid.
 *     Rows k and r are swapped; every entry of row k is divided by the pivot; for every other row i, with g = a[i][c]:
 *     a[i][c'] = a[i][c'] - g * a[k][c'] for all nine c'.  c_k = c.  With `free` the column no step chose:
 *     f[free] = 1, f[c_k] = -a[k][free]; F = f row-major.
 *  4. Rank 2.  S = F^T F, S[i][j] = (F[0][i]*F[0][j] + F[1][i]*F[1][j]) + F[2][i]*F[2][j]; V = identity.  Six sweeps over the
 *     pairs (p, q) = (0,1), (0,2), (1,2), r the third index; a pair with S[p][q] == 0 is skipped:
 *       theta = (S[q][q] - S[p][p]) / (2 * S[p][q]);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta*theta + 1));
 *       c = 1 / sqrt(t*t + 1);  s = t * c;   then, all from the old values:
 *       S[p][p] -= t * S[p][q];  S[q][q] += t * S[p][q];  S[r][p] = c*S[r][p] - s*S[r][q];  S[r][q] = s*S[r][p] + c*S[r][q];
 *       S[p][q] = 0 (S stays symmetric);  for i = 0 .. 2:  V[i][p] = c*V[i][p] - s*V[i][q];  V[i][q] = s*V[i][p] + c*V[i][q].
 *     v = column k of V, k the smallest S[k][k] (lowest k on ties).  g_i = (F[i][0]*v0 + F[i][1]*v1) + F[i][2]*v2;
 *     F[i][j] = F[i][j] - g_i * v_j.
 *  5. F <- Tt^T F Tq, T = [[s, 0, a], [0, s, b], [0, 0, 1]] with a = -(s * cx), b = -(s * cy) of its side:
 *       G[i][0] = F[i][0]*sq;  G[i][1] = F[i][1]*sq;  G[i][2] = (F[i][0]*aq + F[i][1]*bq) + F[i][2];
 *       H[0][j] = st*G[0][j];  H[1][j] = st*G[1][j];  H[2][j] = (at*G[0][j] + bt*G[1][j]) + G[2][j].
 *  6. n = sqrt(H[0][0]^2 + H[0][1]^2 + ... + H[2][2]^2), row-major, left to right; n zero or not finite: invalid; F = H / n.
 *
 * Inlier test (Sampson, image pixels, no division): a_i = (F[i][0]*x + F[i][1]*y) + F[i][2]; b_j = (F[0][j]*x' + F[1][j]*y')
 * + F[2][j]; e = (x'*a0 + y'*a1) + a2; the record is an inlier iff e*e < max_dist2 * (((a0*a0 + a1*a1) + b0*b0) + b1*b1).
 * Selection: the valid hypothesis with the most inliers, the lowest h on ties.  Counts are integers, so the result does not
 * depend on how the records are split over lanes and workgroups, nor on vslam_ctx_set_f32_fused / vslam_ctx_set_matrix_path. */
typedef struct {
    double F[9];      /* all zero when not valid */
    uint32_t inliers;
    int32_t valid;
} vslam_epipolar_hyp; /* 80 bytes */
typedef struct {
    double F[9];        /* row-major; x_train^T F x_query = 0; Frobenius norm 1; all zero when best < 0 */
    uint32_t n_matches; /* min(match_counts[j], match_cap): the records considered */
    uint32_t n_inliers;
    int32_t best;       /* winning hypothesis, -1: none */
    uint32_t n_valid;   /* hypotheses that produced a model */
} vslam_epipolar;       /* 88 bytes */
typedef struct {
    uint32_t n_hypotheses; /* 1 .. 65535 */
    uint32_t seed;
    double max_dist2;      /* squared Sampson distance in pixels^2, finite and positive */
} vslam_epipolar_params;
/* Like vslam_match_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;       /* = sizeof(vslam_epipolar_out) */
    vslam_epipolar* models;   /* [n_pairs], required */
    size_t models_bytes;
    uint64_t* inlier_bits;    /* [n_pairs][(match_cap + 63) / 64] optional: bit i % 64 of word i / 64 = record i is an inlier of
                               * the winner; the first (n_matches + 63) / 64 words of a pair are written, the rest untouched */
    size_t inlier_bits_bytes;
    vslam_match* inliers;     /* [n_pairs][inlier_cap] optional: the inlier records, list order kept */
    size_t inliers_bytes;
    uint32_t* inlier_counts;  /* [n_pairs], required with inliers: totals (may exceed inlier_cap) */
    size_t inlier_counts_bytes;
    uint32_t inlier_cap;
    vslam_epipolar_hyp* hypotheses; /* [n_pairs][n_hypotheses] optional: every hypothesis with its count */
    size_t hypotheses_bytes;
} vslam_epipolar_out;
/* Pair j reads matches[j * match_cap ..], match_counts[j], query_points[j * query_cap ..] and train_points[j * train_cap ..]
 * (DEVICE pointers; consecutive frames: train_points = query_points advanced by one set, as for vslam_match_dev).
 * Asynchronous on the context stream, never waits on the host (the counts are read on the device, the grids are sized from
 * the capacities); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch - and before the context is looked
 * at - for a null pointer, a wrong struct_size, an undersized buffer, inliers without inlier_counts or with inlier_cap == 0,
 * match_cap / query_cap / train_cap == 0, n_pairs outside 0 .. 65535 (0 does nothing), n_hypotheses outside 1 .. 65535, a
 * max_dist2 that is not finite or not positive; then VSLAM_ERR_HIP when there is no usable HIP device, as for
 * vslam_match_dev.  Not for stream capture. */
int vslam_epipolar_dev(vslam_ctx* ctx, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                       const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                       int n_pairs, const vslam_epipolar_params* params, const vslam_epipolar_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call).  model is required; inlier_bits
 * [(n_matches + 63) / 64], (inliers [inlier_cap], n_inliers) and hypotheses [n_hypotheses] are each optional; *n_inliers is
 * the total, which may exceed inlier_cap.  n_query / n_train are the capacities the indices are checked against.  Errors as
 * for vslam_epipolar_dev. */
int vslam_epipolar_host(vslam_ctx* ctx, const vslam_match* matches, size_t n_matches, const vslam_point* query_points, size_t n_query,
                        const vslam_point* train_points, size_t n_train, const vslam_epipolar_params* params, vslam_epipolar* model,
                        uint64_t* inlier_bits, vslam_match* inliers, size_t inlier_cap, size_t* n_inliers,
                        vslam_epipolar_hyp* hypotheses);

/* ---------------------------------------------------------------- fundamental matrix: least-squares refit over the inliers
 * The step between vslam_epipolar_dev and vslam_pose_dev: the winning minimal hypothesis is replaced by the normalised 8-point
 * model over ALL its inliers, the inliers are classified again under the new F, and so on for a fixed number of rounds; a
 * round whose model has fewer inliers than the one before it is dropped, so the result never has fewer inliers than the
 * input.  Inputs: the `models` buffer vslam_epipolar_dev wrote, the FULL match list it read (not the inlier list: membership
 * is computed here) and the point lists.  Coordinates, "trusted" and m = min(match_counts[j], match_cap) are those of the
 * two-view geometry section.  IEEE f64, every + - * / sqrt rounded on its own, sums of a few terms left to right as written.
 * This is the first stage with a floating-point sum over the records of a pair, so the order of that sum is fixed here
 * (tests/refitref.py restates it bit for bit).
 *
 * A record is a MEMBER under F iff it is trusted and passes the inlier test of the two-view section under F with max_dist2.
 *
 * The ordered sum, written SUM(t), of a term t(i) over the records of a pair.  A record that is not a member contributes
 * +0.0.  Block b covers records 4096*b .. 4096*b + 4095.  Slot l (0 .. 255) of a block starts at +0.0 and adds, in this
 * order, the terms of records 4096*b + 256*k + l for k = 0 .. 15, skipping every record at or past m.  Then for h = 128, 64,
 * 32, 16, 8, 4, 2, 1:  s_l = s_l + s_(l+h) for every l < h, all from the values of the step before; B_b = s_0.  The pair's
 * sum is ((B_0 + B_1) + B_2) + ... over the (m + 4095) / 4096 blocks, and +0.0 for m = 0.  The result depends on m and the
 * terms only: not on match_cap, not on the grid, not on the device.
 *
 * Per pair.  F_cur = models_in[j].F, n_cur = the number of members under F_cur (an integer), n_before = n_cur, accepted = 0.
 * A pair with models_in[j].best < 0 is copied through unchanged with stop = 5 and n_before = n_after = accepted = 0.
 * Round 1 .. rounds, until a stop:
 *  1. n_cur < 8: stop = 1.
 *  2. Normalisation per side, members under F_cur, n = (double)n_cur:  cx = SUM(x) / n;  cy = SUM(y) / n;
 *     d = SUM(sqrt(dx*dx + dy*dy)) / n with dx = x - cx, dy = y - cy;  d zero or not finite (either side): stop = 2;
 *     s = 1.4142135623730951 / d; the normalised point is ((x - cx) * s, (y - cy) * s).  (Both sides' centroids come before
 *     either side's d is looked at.)
 *  3. Moment matrix.  a = the row of step 2 of the two-view model from the member's normalised (x, y), (x', y'):
 *     [x'*x, x'*y, x', y'*x, y'*y, y', x, y, 1].  M[p][q] = SUM(a_p * a_q) for p <= q - 45 sums, M[8][8] = SUM(1.0) -,
 *     mirrored below the diagonal.
 *  4. Eigenvector.  S = M, V = the 9 x 9 identity.  VSLAM_REFIT_SWEEPS sweeps of cyclic Jacobi over the pairs (p, q), p < q,
 *     row-major ((0,1), (0,2) .. (0,8), (1,2) .. (7,8)); a pair with S[p][q] == 0 is skipped; theta, t, c, s as in step 4 of
 *     the two-view model;  S[p][p] -= t * S[p][q];  S[q][q] += t * S[p][q];  for every r not in {p, q}, from the old values:
 *     S[r][p] = c*S[r][p] - s*S[r][q];  S[r][q] = s*S[r][p] + c*S[r][q]  (S stays symmetric);  S[p][q] = 0;  for i = 0 .. 8:
 *     V[i][p] = c*V[i][p] - s*V[i][q];  V[i][q] = s*V[i][p] + c*V[i][q].   f = column k of V, k the smallest S[k][k] (lowest k
 *     on ties; a NaN is never smaller).
 *  5. F_new from f (row-major) by steps 4, 5 and 6 of the two-view model verbatim - rank 2, Tt^T F Tq with the (s, cx, cy) of
 *     step 2 here, Frobenius norm 1 -; the norm zero or not finite: stop = 3.
 *  6. n_new = the number of members under F_new.  n_new >= n_cur: F_cur = F_new, n_cur = n_new, accepted += 1; otherwise
 *     stop = 4.
 * All rounds done without a stop: stop = 0.  After a stop the pair does nothing more.  Output: models[j] = models_in[j] with
 * F = F_cur and n_inliers = n_cur (n_matches, best, n_valid copied); n_after = n_cur >= n_before.  The inlier outputs are the
 * members under the output F, whatever its stop (vslam_epipolar_dev writes F = 0 with best < 0: no record is a member then).
 * VSLAM_REFIT_SWEEPS was fixed by measurement: from 6 sweeps on, every sweep count up to 20 gives the same f
 * bit for bit on every planted scene and hostile fixture of the tests; the constant is that plus two. */
#define VSLAM_REFIT_SWEEPS 8
typedef struct {
    uint32_t rounds;  /* 1 .. 8 */
    double max_dist2; /* as vslam_epipolar_params: squared Sampson distance in pixels^2, finite and positive */
} vslam_refit_params;
typedef struct {
    uint32_t n_before, n_after; /* members under the input F / under the output F */
    uint32_t accepted;          /* rounds whose refit was kept */
    int32_t stop;               /* 0: ran all rounds, 1: fewer than 8 members, 2: degenerate normalisation, 3: model invalid
                                 * (step 5), 4: the refit had fewer inliers, 5: no input model */
} vslam_refit;                  /* 16 bytes */
/* Like vslam_epipolar_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;      /* = sizeof(vslam_refit_out) */
    vslam_epipolar* models;  /* [n_pairs], required; may be the very pointer passed as models_in, must not otherwise overlap it */
    size_t models_bytes;
    vslam_refit* info;       /* [n_pairs] optional */
    size_t info_bytes;
    uint64_t* inlier_bits;   /* [n_pairs][(match_cap + 63) / 64] optional: bit i % 64 of word i / 64 = record i is a member under
                              * the output F; the first (n_matches + 63) / 64 words of a pair are written, the rest untouched */
    size_t inlier_bits_bytes;
    vslam_match* inliers;    /* [n_pairs][inlier_cap] optional: the member records, list order kept */
    size_t inliers_bytes;
    uint32_t* inlier_counts; /* [n_pairs], required with inliers: totals (may exceed inlier_cap) */
    size_t inlier_counts_bytes;
    uint32_t inlier_cap;
} vslam_refit_out;
/* Pair j reads models_in[j] and the lists as vslam_epipolar_dev does (DEVICE pointers).  Asynchronous on the context stream,
 * never waits on the host (the counts are read on the device, the grids are sized from the capacities, a stopped pair's
 * workgroups leave at once); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch - and before the context is
 * looked at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does nothing), rounds outside 1 .. 8, a
 * max_dist2 that is not finite or not positive, match_cap / query_cap / train_cap == 0, an undersized buffer, inliers without
 * inlier_counts or with inlier_cap == 0; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for stream capture. */
int vslam_refit_dev(vslam_ctx* ctx, const vslam_epipolar* models_in, const vslam_match* matches, const uint32_t* match_counts,
                    uint32_t match_cap, const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points,
                    uint32_t train_cap, int n_pairs, const vslam_refit_params* params, const vslam_refit_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call).  model_in and model are required (they
 * may be the same record); info, inlier_bits [(n_matches + 63) / 64] and (inliers [inlier_cap], n_inliers) are each optional;
 * *n_inliers is the total, which may exceed inlier_cap.  n_query / n_train are the capacities the indices are checked
 * against.  Errors as for vslam_refit_dev. */
int vslam_refit_host(vslam_ctx* ctx, const vslam_epipolar* model_in, const vslam_match* matches, size_t n_matches,
                     const vslam_point* query_points, size_t n_query, const vslam_point* train_points, size_t n_train,
                     const vslam_refit_params* params, vslam_epipolar* model, vslam_refit* info, uint64_t* inlier_bits,
                     vslam_match* inliers, size_t inlier_cap, size_t* n_inliers);

/* ---------------------------------------------------------------- guided matching
 * A second matching pass, once a pair's fundamental matrix is known: the nearest-two search of the descriptor matching section,
 * restricted for every query row to the train rows whose point lies in the query's epipolar band.  The ratio test of the first
 * pass rejects a correct match whenever a similar descriptor exists anywhere in the other frame (repeated structure); almost all
 * such look-alikes lie off the query's epipolar line and no longer count here.  Inputs per pair j: set j of `query` and of
 * `train` (points required on both sides), models[j] - a vslam_epipolar record as vslam_epipolar_dev, vslam_refit_dev or the
 * gate of vslam_homography_dev writes it - and the parameters.  The arithmetic is fixed here so that a CPU can restate it bit
 * for bit (tests/guidedref.py).
 *
 * Coordinates are the two-view section's, exact in f64: x = (p.col - p.padding) * 2^(p.octave - 1), y likewise from p.row.  A
 * row is TRUSTED iff its point's octave is in 0 .. 31.
 *
 * Train row j is IN BAND of query row i iff models[p].best >= 0, both rows are trusted, and the two-view section's inlier
 * test holds under F = models[p].F with (x, y) the query row's point and (x', y') the train row's:
 *   a_k = (F[k][0]*x + F[k][1]*y) + F[k][2];   b_k = (F[0][k]*x' + F[1][k]*y') + F[2][k];   e = (x'*a0 + y'*a1) + a2;
 *   in band iff  e*e < max_dist2 * (((a0*a0 + a1*a1) + b0*b0) + b1*b1).
 * IEEE f64, every operation rounded on its own, no fused multiply-add.  The predicate is a pure function of F, the two points
 * and max_dist2; a false comparison (a NaN, F = 0) is "not in band"; a pair with best < 0 has no row in band, whatever its F
 * holds.
 *
 * d2 is the descriptor matching section's, unchanged, and so is the sequential selection over j = 0 .. nt-1 ascending, with
 * one more skipped case: a train row that is not in band of the query row (besides a `defined` byte of 0 and, with
 * same_octave, a differing octave).  second_dist2 is therefore the second nearest IN THE BAND.  Ties, NaN and +-inf behave as
 * there.  A query row that is undefined or not trusted gets {-1, +inf, +inf}.
 *
 * A query is ACCEPTED iff index >= 0 and (second == +inf or best < ratio2 * second, the product rounded once to f32) and
 * best < max_desc_dist2.  A lone candidate in a narrow band passes the ratio clause whatever its distance: the absolute bound
 * is there for that case, and max_desc_dist2 = +inf switches it off.
 *
 * Output: vslam_match_out, layout and ordering as vslam_match_dev writes it; the list goes straight into vslam_epipolar_dev
 * and vslam_refit_dev.  Results depend neither on vslam_ctx_set_f32_fused nor on vslam_ctx_set_matrix_path. */
typedef struct {
    float ratio2;         /* the SQUARED ratio of Lowe's test, finite and positive */
    float max_desc_dist2; /* accepted only below this d2; positive, +inf = no bound */
    double max_dist2;     /* half-width of the band: squared Sampson distance in pixels^2, finite and positive */
    int32_t same_octave;  /* as vslam_match_dev */
    uint32_t reserved;    /* must be 0 */
} vslam_guided_params;    /* 24 bytes */
/* Pair j searches set j of `train` for every row of set j of `query` under models[j] (DEVICE pointers), j < n_pairs (at most
 * 65535; 0 does nothing).  Asynchronous on the context stream, never waits on the host (the counts and the models are read on
 * the device); scratch belongs to the context and is sized from the capacities before the launches.  VSLAM_ERR_INVALID before
 * any launch - and before the context is looked at - for everything vslam_match_dev rejects, null points on either side,
 * null models or params, a reserved word that is not 0, a ratio2 or max_dist2 that is not finite or not positive, a
 * max_desc_dist2 that is NaN or not positive; then VSLAM_ERR_HIP as for vslam_match_dev.  Not for stream capture. */
int vslam_match_guided_dev(vslam_ctx* ctx, const vslam_desc_sets* query, const vslam_desc_sets* train, const vslam_epipolar* models,
                           int n_pairs, const vslam_guided_params* params, const vslam_match_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call): the arguments of vslam_match_host with
 * both point lists required ([nq] and [nt]; NULL only with no rows), one model and the parameters.  nn [nq] and (matches
 * [match_cap], n_matches) are each optional; *n_matches is the total, which may exceed match_cap.  Errors as for
 * vslam_match_guided_dev. */
int vslam_match_guided_host(vslam_ctx* ctx, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                            const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt,
                            const vslam_epipolar* model, const vslam_guided_params* params, vslam_nn2* nn, vslam_match* matches,
                            size_t match_cap, size_t* n_matches);

/* ---------------------------------------------------------------- homography and the degeneracy verdict
 * Beside vslam_epipolar_dev, over the same lists: the RANSAC homography of every pair, and - given the fundamental matrices
 * of the same pairs - a verdict per pair on whether the homography explains the matches as well as F does (a planar scene, a
 * pure rotation, a pure image translation), in which case F is one arbitrary member of a family and must not be decomposed.
 * The verdict acts through a GATE: a copy of the epipolar models in which a degenerate pair is the "no model" record, which
 * vslam_refit_dev copies through, vslam_pose_dev gives no pose and vslam_chain_dev starts a new segment at.  A fixed number
 * of hypotheses, no adaptive stop; the least-squares refit of H (vslam_hrefit_dev) and the decomposition of H into R, t, n
 * (vslam_hpose_dev) are stages of their own.  Coordinates, "trusted",
 * m = min(match_counts[j], match_cap) and mix() are those of the two-view geometry section.  The arithmetic is fixed here so
 * that a CPU can restate it bit for bit (tests/homref.py): IEEE f64, every + - * / sqrt rounded on its own (no fused
 * multiply-add), sums left to right as written.  Matrices are row-major, M[i][j] = M[3*i + j].
 *
 * Sampling: base = mix(mix(seed + j) + h); draw t = 0, 1, ... gives r = mix(base + t) and the index (uint64(r) * m) >> 32, kept
 * if it is not among the indices kept so far; the sample is the first 4 kept indices, in that order.  Fewer than 4 after 64
 * draws: invalid.  m < 4: every hypothesis is invalid.  A sample that contains a record that is not trusted is invalid.
 *
 * Model from the 4 records (x, y) = query, (x', y') = train - the normalised direct linear transform:
 *  1. Per side: cx = (((x0 + x1) + x2) + x3) / 4, cy likewise; d = (((r0 + r1) + r2) + r3) / 4 with ri = sqrt(dx*dx + dy*dy),
 *     dx = xi - cx, dy = yi - cy; d == 0: invalid; s = 1.4142135623730951 / d; normalised point ((xi - cx) * s, (yi - cy) * s).
 *  2. The 8 x 9 matrix a from the normalised (x, y), (x', y') of record i = 0 .. 3:
 *       row 2i     = [x, y, 1, 0, 0, 0, -(x'*x), -(x'*y), -x'];
 *       row 2i + 1 = [0, 0, 0, x, y, 1, -(y'*x), -(y'*y), -y'].
 *  3. Step 3 of the two-view model, word for word: Gauss-Jordan with full pivoting over steps k = 0 .. 7, the same scan order
 *     (r ascending, then c ascending, strictly larger replaces, starting at 0), the same validity rules (no choice, or an
 *     infinite pivot: invalid), the same row operations.  With `free` the column no step chose: h[free] = 1,
 *     h[c_k] = -a[k][free]; Hn = h row-major.
 *  4. M = Tt^-1 Hn Tq, with aq = -(sq * cqx), bq = -(sq * cqy), r = 1 / st:
 *       G1[i][0] = Hn[i][0]*sq;  G1[i][1] = Hn[i][1]*sq;  G1[i][2] = (Hn[i][0]*aq + Hn[i][1]*bq) + Hn[i][2];
 *       M[0][j] = r*G1[0][j] + ctx*G1[2][j];  M[1][j] = r*G1[1][j] + cty*G1[2][j];  M[2][j] = G1[2][j].
 *  5. n = sqrt(M[0][0]^2 + M[0][1]^2 + ... + M[2][2]^2), row-major, left to right; n zero or not finite: invalid; H = M / n.
 *  6. Sign.  w = (H[2][0]*x0 + H[2][1]*y0) + H[2][2] with (x0, y0) the query point of the sample's first record, in pixels.
 *     Neither w > 0 nor w < 0: invalid.  w < 0: all nine entries of H are negated.
 *  7. G = adj(H), each entry one a*b - c*d (two products, one difference):
 *       G[0][0] = H[1][1]*H[2][2] - H[1][2]*H[2][1];  G[0][1] = H[0][2]*H[2][1] - H[0][1]*H[2][2];  G[0][2] = H[0][1]*H[1][2] - H[0][2]*H[1][1];
 *       G[1][0] = H[1][2]*H[2][0] - H[1][0]*H[2][2];  G[1][1] = H[0][0]*H[2][2] - H[0][2]*H[2][0];  G[1][2] = H[0][2]*H[1][0] - H[0][0]*H[1][2];
 *       G[2][0] = H[1][0]*H[2][1] - H[1][1]*H[2][0];  G[2][1] = H[0][1]*H[2][0] - H[0][0]*H[2][1];  G[2][2] = H[0][0]*H[1][1] - H[0][1]*H[1][0].
 *     wg = (G[2][0]*x'0 + G[2][1]*y'0) + G[2][2] with (x'0, y'0) the train point of the sample's first record.  wg zero or
 *     not finite: invalid.  wg < 0: all nine entries of G are negated.  (G is not scaled: the inlier test is homogeneous.)
 *
 * Inlier test (symmetric transfer, image pixels, no division):  p_i = (H[i][0]*x + H[i][1]*y) + H[i][2];
 * q_i = (G[i][0]*x' + G[i][1]*y') + G[i][2].  Forward: p2 > 0 and dx*dx + dy*dy < max_dist2 * (p2*p2) with dx = p0 - x'*p2,
 * dy = p1 - y'*p2.  Backward: q2 > 0 and ex*ex + ey*ey < max_dist2 * (q2*q2) with ex = q0 - x*q2, ey = q1 - y*q2.  A record is
 * an inlier iff it is trusted and both tests hold (max_dist2 bounds each direction's squared transfer error in pixels^2).
 * Selection: the valid hypothesis with the most inliers, the lowest h on ties.  Counts are integers, so the result does not
 * depend on how the records are split over lanes and workgroups, nor on vslam_ctx_set_f32_fused / vslam_ctx_set_matrix_path.
 *
 * Verdict, integers only.  n_epipolar = epipolar_models[j].n_inliers, and 0 without epipolar_models or when
 * epipolar_models[j].best < 0.  degenerate = best >= 0 && epipolar_models[j].best >= 0 && n_inliers >= min_inliers &&
 * uint64(n_inliers) * degenerate_den >= uint64(degenerate_num) * n_epipolar;  0 without epipolar_models.
 * Gate.  gated_models[j] = epipolar_models[j], except that a degenerate pair becomes the "no model" record: F all zero,
 * n_inliers = 0, best = -1, n_matches and n_valid kept. */
typedef struct {
    double H[9];      /* query -> train; all zero when not valid */
    double G[9];      /* train -> query: adj(H) up to sign; all zero when not valid */
    uint32_t inliers;
    int32_t valid;
} vslam_homography_hyp; /* 152 bytes */
typedef struct {
    double H[9];         /* row-major; x_train ~ H x_query; Frobenius norm 1; all zero when best < 0 */
    double G[9];         /* x_query ~ G x_train; all zero when best < 0 */
    uint32_t n_matches;  /* min(match_counts[j], match_cap): the records considered */
    uint32_t n_inliers;
    int32_t best;        /* winning hypothesis, -1: none */
    uint32_t n_valid;    /* hypotheses that produced a model */
    uint32_t n_epipolar; /* the verdict's other count */
    int32_t degenerate;  /* 1: H explains the matches as well as F does - F must not be decomposed */
} vslam_homography;      /* 168 bytes */
typedef struct {
    uint32_t n_hypotheses;   /* 1 .. 65535 */
    uint32_t seed;
    double max_dist2;        /* squared transfer error in pixels^2, each direction; finite and positive */
    uint32_t degenerate_num; /* the verdict's ratio n_inliers / n_epipolar >= degenerate_num / degenerate_den */
    uint32_t degenerate_den; /* > 0 */
    uint32_t min_inliers;    /* fewer H-inliers than this: never degenerate */
} vslam_homography_params;
/* Like vslam_epipolar_out: every pointer with the bytes behind it, checked before anything is launched.  inlier_bits,
 * inliers, inlier_counts, inlier_cap and hypotheses follow vslam_epipolar_out's rules exactly. */
typedef struct {
    size_t struct_size;        /* = sizeof(vslam_homography_out) */
    vslam_homography* models;  /* [n_pairs], required */
    size_t models_bytes;
    uint64_t* inlier_bits;     /* [n_pairs][(match_cap + 63) / 64] optional: bit i % 64 of word i / 64 = record i is an inlier of
                                * the winner; the first (n_matches + 63) / 64 words of a pair are written, the rest untouched */
    size_t inlier_bits_bytes;
    vslam_match* inliers;      /* [n_pairs][inlier_cap] optional: the inlier records, list order kept */
    size_t inliers_bytes;
    uint32_t* inlier_counts;   /* [n_pairs], required with inliers: totals (may exceed inlier_cap) */
    size_t inlier_counts_bytes;
    uint32_t inlier_cap;
    vslam_homography_hyp* hypotheses; /* [n_pairs][n_hypotheses] optional: every hypothesis with its count */
    size_t hypotheses_bytes;
    vslam_epipolar* gated_models; /* [n_pairs] optional, needs epipolar_models: the gate; may be the very pointer passed as
                                   * epipolar_models, must not otherwise overlap it */
    size_t gated_models_bytes;
} vslam_homography_out;
/* Pair j reads the lists as vslam_epipolar_dev does (DEVICE pointers) and, when given, epipolar_models[j] - the `models`
 * buffer of vslam_epipolar_dev or vslam_refit_dev over the same pairs; NULL: no verdict (n_epipolar = degenerate = 0).
 * Asynchronous on the context stream, never waits on the host (the counts are read on the device, the grids are sized from
 * the capacities); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch - and before the context is looked
 * at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does nothing), n_hypotheses outside 1 .. 65535,
 * a max_dist2 that is not finite or not positive, degenerate_den == 0, match_cap / query_cap / train_cap == 0, an undersized
 * buffer, inliers without inlier_counts or with inlier_cap == 0, gated_models without epipolar_models; then VSLAM_ERR_HIP
 * when there is no usable HIP device.  Not for stream capture. */
int vslam_homography_dev(vslam_ctx* ctx, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                         const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                         int n_pairs, const vslam_epipolar* epipolar_models, const vslam_homography_params* params,
                         const vslam_homography_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call).  model is required; epipolar_model
 * (one record, the verdict's input), inlier_bits [(n_matches + 63) / 64], (inliers [inlier_cap], n_inliers), hypotheses
 * [n_hypotheses] and gated_model (one record, needs epipolar_model) are each optional; *n_inliers is the total, which may
 * exceed inlier_cap.  n_query / n_train are the capacities the indices are checked against.  Errors as for
 * vslam_homography_dev. */
int vslam_homography_host(vslam_ctx* ctx, const vslam_match* matches, size_t n_matches, const vslam_point* query_points,
                          size_t n_query, const vslam_point* train_points, size_t n_train, const vslam_epipolar* epipolar_model,
                          const vslam_homography_params* params, vslam_homography* model, uint64_t* inlier_bits,
                          vslam_match* inliers, size_t inlier_cap, size_t* n_inliers, vslam_homography_hyp* hypotheses,
                          vslam_epipolar* gated_model);

/* ---------------------------------------------------------------- homography: least-squares refit over the inliers
 * The step after vslam_homography_dev, the sibling of vslam_refit_dev: the winning 4-point hypothesis is replaced by the
 * normalised direct linear transform over ALL its inliers, the inliers are classified again under the new (H, G), and so on
 * for a fixed number of rounds; a round whose model has fewer inliers than the one before it is dropped, so the result never
 * has fewer inliers than the input.  What reads H afterwards - vslam_match_guided_hf_dev's window, vslam_hpose_dev's
 * decomposition, the verdict against a refitted F - then reads the polished model.  Inputs: the `models` buffer
 * vslam_homography_dev wrote, the FULL match list it read and the point lists.  No non-linear refinement of the transfer
 * error.  The arithmetic is fixed here so that a CPU can restate it bit for bit (tests/hrefitref.py): IEEE f64, every
 * + - * / sqrt rounded on its own (no fused multiply-add), sums of a few terms left to right as written.  Coordinates,
 * "trusted" and m = min(match_counts[j], match_cap) are those of the two-view geometry section.  SUM(term) is the ordered sum
 * of the refit section ("fundamental matrix: least-squares refit over the inliers"), verbatim: blocks of 4096 records, 256
 * slots, the halving tree, the blocks added left to right; a record that is not a member contributes +0.0.
 *
 * A record is a MEMBER under (H, G) iff it is an inlier of the homography section's inlier test (symmetric transfer: trusted,
 * forward and backward) under (H, G) with max_dist2.
 *
 * Per pair.  (H_cur, G_cur) = (models_in[j].H, models_in[j].G), n_cur = the number of members under it (an integer),
 * n_before = n_cur, accepted = 0.  A pair with models_in[j].best < 0 is copied through unchanged with stop = 5 and
 * n_before = n_after = accepted = 0.  Round 1 .. rounds, until a stop:
 *  1. n_cur < 4: stop = 1.
 *  2. Normalisation per side, members under (H_cur, G_cur): step 2 of the refit section word for word - n = (double)n_cur;
 *     cx = SUM(x) / n; cy = SUM(y) / n; d = SUM(sqrt(dx*dx + dy*dy)) / n with dx = x - cx, dy = y - cy; d zero or not finite
 *     (either side): stop = 2; s = 1.4142135623730951 / d; the normalised point is ((x - cx) * s, (y - cy) * s).  Both sides'
 *     centroids come before either side's d is looked at.
 *  3. Moment matrix, from 24 ordered sums.  With the member's normalised (x, y), (x', y'):  w = x'*x' + y'*y';
 *     e = (x*x, x*y, x, y*y, y, 1.0), e_k for the index pairs k(a, b) = k(b, a) of (0,0), (0,1), (0,2), (1,1), (1,2), (2,2);
 *       A_k = SUM(e_k);  B_k = SUM(x' * e_k);  C_k = SUM(y' * e_k);  D_k = SUM(w * e_k).
 *     For a, b in 0 .. 2 with k = k(a, b):  M[a][b] = M[3+a][3+b] = A_k;  M[a][3+b] = +0.0;  M[a][6+b] = -B_k;
 *     M[3+a][6+b] = -C_k;  M[6+a][6+b] = D_k;  mirrored below the diagonal blocks.  (This is A^T A of the two rows per member
 *     of the homography section's step 2, written through its block structure; the definition above is the normative one,
 *     not the expanded rows: the two round differently.  A_5 = SUM(1.0) = n_cur.)
 *  4. Eigenvector.  Step 4 of the refit section verbatim on S = M: VSLAM_HREFIT_SWEEPS sweeps of the same cyclic Jacobi, a pair
 *     with S[p][q] == 0 skipped; h = column k of V, k the smallest S[k][k] (lowest k on ties; a NaN is never smaller).
 *  5. H_new from Hn = h (row-major) by steps 4 and 5 of the homography model verbatim - Tt^-1 Hn Tq with the (s, cx, cy) of step
 *     2 here, Frobenius norm 1 -; the norm zero or not finite: stop = 3.  Sign: w = (H[2][0]*cqx + H[2][1]*cqy) + H[2][2] with
 *     (cqx, cqy) the query centroid of step 2, in pixels; neither w > 0 nor w < 0: stop = 3; w < 0: all nine entries negated.
 *     G_new = adj(H_new) by the nine expressions of step 7 there; wg = (G[2][0]*ctx + G[2][1]*cty) + G[2][2] with the train
 *     centroid; wg zero or not finite: stop = 3; wg < 0: all nine entries of G negated.
 *  6. n_new = the number of members under (H_new, G_new).  n_new >= n_cur: (H_cur, G_cur) = (H_new, G_new), n_cur = n_new,
 *     accepted += 1; otherwise stop = 4.
 * All rounds done without a stop: stop = 0.  After a stop the pair does nothing more.  Output: models[j] = models_in[j] with
 * H = H_cur, G = G_cur and n_inliers = n_cur (n_matches, best, n_valid copied); n_after = n_cur >= n_before.  The inlier outputs
 * are the members under the output (H, G), whatever its stop.
 * Verdict.  With epipolar_models, n_epipolar and degenerate of models[j] are computed again by the homography section's
 * integer rule from the new n_inliers, and gated_models - optional, may be the very pointer passed as epipolar_models - is
 * the gate under that verdict.  Without epipolar_models both fields are copied from models_in[j].
 * VSLAM_HREFIT_SWEEPS was fixed by measurement, as VSLAM_REFIT_SWEEPS was: from 7 sweeps on, every sweep count
 * up to 20 gives the same h bit for bit on every planted scene and hostile fixture of the tests; the constant is that plus
 * two. */
#define VSLAM_HREFIT_SWEEPS 9
typedef struct {
    uint32_t rounds;         /* 1 .. 8 */
    double max_dist2;        /* as vslam_homography_params: squared transfer error in pixels^2, each direction; finite and positive */
    uint32_t degenerate_num; /* the verdict's ratio, as vslam_homography_params; read only with epipolar_models */
    uint32_t degenerate_den; /* > 0 with epipolar_models */
    uint32_t min_inliers;    /* fewer H-inliers than this: never degenerate */
} vslam_hrefit_params;
typedef struct {
    uint32_t n_before, n_after; /* members under the input (H, G) / under the output (H, G) */
    uint32_t accepted;          /* rounds whose refit was kept */
    int32_t stop;               /* 0: ran all rounds, 1: fewer than 4 members, 2: degenerate normalisation, 3: model invalid
                                 * (step 5), 4: the refit had fewer inliers, 5: no input model */
} vslam_hrefit;                 /* 16 bytes: the fields and stop codes of vslam_refit */
/* Like vslam_refit_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;        /* = sizeof(vslam_hrefit_out) */
    vslam_homography* models;  /* [n_pairs], required; may be the very pointer passed as models_in, must not otherwise overlap it */
    size_t models_bytes;
    vslam_hrefit* info;        /* [n_pairs] optional */
    size_t info_bytes;
    uint64_t* inlier_bits;     /* [n_pairs][(match_cap + 63) / 64] optional: bit i % 64 of word i / 64 = record i is a member under
                                * the output (H, G); the first (n_matches + 63) / 64 words of a pair are written, the rest untouched */
    size_t inlier_bits_bytes;
    vslam_match* inliers;      /* [n_pairs][inlier_cap] optional: the member records, list order kept */
    size_t inliers_bytes;
    uint32_t* inlier_counts;   /* [n_pairs], required with inliers: totals (may exceed inlier_cap) */
    size_t inlier_counts_bytes;
    uint32_t inlier_cap;
    vslam_epipolar* gated_models; /* [n_pairs] optional, needs epipolar_models: the gate under the new verdict; may be the very
                                   * pointer passed as epipolar_models, must not otherwise overlap it */
    size_t gated_models_bytes;
} vslam_hrefit_out;
/* Pair j reads models_in[j], the lists as vslam_homography_dev does (DEVICE pointers) and, when given, epipolar_models[j].
 * Asynchronous on the context stream, never waits on the host (the counts are read on the device, the grids are sized from
 * the capacities, a stopped pair's workgroups leave at once); scratch belongs to the context.  VSLAM_ERR_INVALID before any
 * launch - and before the context is looked at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does
 * nothing), rounds outside 1 .. 8, a max_dist2 that is not finite or not positive, degenerate_den == 0 with epipolar_models,
 * match_cap / query_cap / train_cap == 0, an undersized buffer, inliers without inlier_counts or with inlier_cap == 0,
 * gated_models without epipolar_models; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for stream capture. */
int vslam_hrefit_dev(vslam_ctx* ctx, const vslam_homography* models_in, const vslam_match* matches, const uint32_t* match_counts,
                     uint32_t match_cap, const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points,
                     uint32_t train_cap, int n_pairs, const vslam_epipolar* epipolar_models, const vslam_hrefit_params* params,
                     const vslam_hrefit_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call).  model_in and model are required (they
 * may be the same record); epipolar_model (one record, the verdict's input), info, inlier_bits [(n_matches + 63) / 64],
 * (inliers [inlier_cap], n_inliers) and gated_model (one record, needs epipolar_model) are each optional; *n_inliers is the
 * total, which may exceed inlier_cap.  n_query / n_train are the capacities the indices are checked against.  Errors as for
 * vslam_hrefit_dev. */
int vslam_hrefit_host(vslam_ctx* ctx, const vslam_homography* model_in, const vslam_match* matches, size_t n_matches,
                      const vslam_point* query_points, size_t n_query, const vslam_point* train_points, size_t n_train,
                      const vslam_epipolar* epipolar_model, const vslam_hrefit_params* params, vslam_homography* model,
                      vslam_hrefit* info, uint64_t* inlier_bits, vslam_match* inliers, size_t inlier_cap, size_t* n_inliers,
                      vslam_epipolar* gated_model);

/* ---------------------------------------------------------------- guided matching under H or F
 * The guided pass for every pair of a batch, under the model that applies to it.  A pair the gate above judged degenerate - a
 * planar scene, a pure rotation, a pure image translation - carries the "no model" record, and vslam_match_guided_dev finds
 * nothing for it; but for such a pair H predicts a position, not a line, and a window around H x is a far narrower search than
 * the epipolar band.  Everything that is not named here is the guided matching section's, unchanged: d2, the sequential
 * nearest-two selection, ties, NaN and +-inf, "trusted", the coordinates, the acceptance rule with ratio2 and max_desc_dist2,
 * and vslam_match_out with its ordering.  The arithmetic is fixed here so that a CPU can restate it bit for bit
 * (tests/guidedhfref.py).
 *
 * KIND of pair p, read on the device:  F iff epipolar_models != NULL and epipolar_models[p].best >= 0;  otherwise H iff
 * homography_models != NULL and homography_models[p].best >= 0;  otherwise NONE: every query row gets {-1, +inf, +inf} and
 * the count is 0.  At least one of the two arrays must be given.  With the gate's gated_models as epipolar_models, H applies
 * to the degenerate pairs and to the pairs RANSAC gave no F; with epipolar_models = NULL, H applies to every pair; with
 * homography_models = NULL, the call is vslam_match_guided_dev.
 *
 * Kind F.  Train row j is a candidate of query row i iff it is IN BAND: the guided matching section's predicate under
 * params.max_dist2, operation for operation.
 *
 * Kind H.  Train row j is a candidate iff it is IN WINDOW.  With (x, y) the query row's point, (x', y') the train row's and
 * H = homography_models[p].H:
 *   p_k = (H[k][0]*x + H[k][1]*y) + H[k][2]  for k = 0, 1, 2;   L = max_transfer2 * (p2*p2);
 *   dx = p0 - x'*p2;   dy = p1 - y'*p2;
 *   in window iff both rows are trusted, p2 > 0 and dx*dx + dy*dy < L.
 * IEEE f64, every operation rounded on its own, no fused multiply-add.  A false comparison (a NaN, overflow to inf on both
 * sides, H = 0) is "not in window".  This is the FORWARD clause of the homography section's inlier test, word for word; G is
 * not read.  Forward only: it is what "predicted position" means, and the symmetric form changed at most 2 matches per scene
 * on the planted scenes of the tests.  Whoever wants the symmetric test gets it from vslam_homography_dev on the guided list.
 *
 * The selection skips a train row that is not a candidate, exactly where the guided matching section skips one that is not
 * in band; second_dist2 is the second nearest AMONG THE CANDIDATES.  Results depend neither on vslam_ctx_set_f32_fused nor on
 * vslam_ctx_set_matrix_path. */
typedef struct {
    float ratio2;         /* the SQUARED ratio of Lowe's test, finite and positive */
    float max_desc_dist2; /* accepted only below this d2; positive, +inf = no bound */
    double max_dist2;     /* kind F: half-width of the band, squared Sampson distance in pixels^2; finite and positive - checked
                           * only when epipolar_models is given */
    double max_transfer2; /* kind H: radius^2 of the window, squared transfer error in pixels^2; finite and positive - checked
                           * only when homography_models is given */
    int32_t same_octave;  /* as vslam_match_dev */
    uint32_t reserved;    /* must be 0 */
} vslam_guided_hf_params; /* 32 bytes */
/* Pair j searches set j of `train` for every row of set j of `query` under epipolar_models[j] or homography_models[j] (DEVICE
 * pointers, either array may be NULL), j < n_pairs (at most 65535; 0 does nothing).  Asynchronous on the context stream, never
 * waits on the host (the counts, the models and with them every pair's kind are read on the device); scratch belongs to the
 * context and is sized from the capacities before the launches.  VSLAM_ERR_INVALID before any launch - and before the context
 * is looked at - for everything vslam_match_guided_dev rejects (max_dist2 only with epipolar_models), both model arrays NULL,
 * and with homography_models a max_transfer2 that is not finite or not positive; then VSLAM_ERR_HIP as for vslam_match_dev.
 * Not for stream capture. */
int vslam_match_guided_hf_dev(vslam_ctx* ctx, const vslam_desc_sets* query, const vslam_desc_sets* train,
                              const vslam_epipolar* epipolar_models, const vslam_homography* homography_models, int n_pairs,
                              const vslam_guided_hf_params* params, const vslam_match_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call): the arguments of vslam_match_guided_host
 * with two model records, each optional, not both NULL.  Errors as for vslam_match_guided_hf_dev. */
int vslam_match_guided_hf_host(vslam_ctx* ctx, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                               const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt,
                               const vslam_epipolar* epipolar_model, const vslam_homography* homography_model,
                               const vslam_guided_hf_params* params, vslam_nn2* nn, vslam_match* matches, size_t match_cap,
                               size_t* n_matches);

/* ---------------------------------------------------------------- relative pose and triangulation
 * The step after the fundamental matrix: the camera motion of every pair and the 3-D point of every match record, from the
 * `models` buffer vslam_epipolar_dev wrote (only F and best are read), a match list (any list; the intended one is the
 * inliers / inlier_counts / inlier_cap of vslam_epipolar_dev) and the point lists.  One pinhole camera for both frames, no
 * skew, no distortion.  Convention: x_train ~ R * x_query + t with |t| = 1 (the scale of a two-view reconstruction is free);
 * a point X is in the QUERY camera's frame.  No degeneracy handling of its own: a planar scene or a pure rotation gets whatever the
 * decomposition gives - unless `models` is the gated_models buffer of vslam_homography_dev, where such a pair has best < 0.  Records are trusted, and their coordinates (x, y) = query, (x', y') = train computed, exactly as in
 * the two-view geometry section; m = min(match_counts[j], match_cap) records are considered.  The arithmetic is fixed here so
 * that a CPU can restate it bit for bit (tests/poseref.py): IEEE f64, every + - * / sqrt rounded on its own, sums left to
 * right as written.  Matrices are row-major, M[i][j] = M[3*i + j].
 *
 *  1. Essential matrix E = K^T F K, K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]:
 *       G[i][0] = F[i][0]*fx;  G[i][1] = F[i][1]*fy;  G[i][2] = (F[i][0]*cx + F[i][1]*cy) + F[i][2];
 *       E[0][j] = fx*G[0][j];  E[1][j] = fy*G[1][j];  E[2][j] = (cx*G[0][j] + cy*G[1][j]) + G[2][j];
 *     then E = E / n, n the Frobenius norm as in step 6 of the two-view model (row-major, left to right); n zero or not
 *     finite: the pair is INVALID.  A pair with models[j].best < 0 is invalid.
 *  2. Right singular vectors: S = E^T E and the six Jacobi sweeps of step 4 of the two-view model, verbatim, give S and V.
 *     k = the index of the smallest S[k][k] (lowest on ties), p < q the other two indices;  v1 = V[:, p], v2 = V[:, q],
 *     v3 = v1 x v2, the cross product being (a x b)_0 = a1*b2 - a2*b1, (a x b)_1 = a2*b0 - a0*b2, (a x b)_2 = a0*b1 - a1*b0.
 *  3. Left singular vectors: w1_i = (E[i][0]*v1_0 + E[i][1]*v1_1) + E[i][2]*v1_2;  n = sqrt((w1_0*w1_0 + w1_1*w1_1) + w1_2*w1_2);
 *     n zero or not finite: invalid;  u1_i = w1_i / n.  w2 likewise from v2;  d = (u1_0*w2_0 + u1_1*w2_1) + u1_2*w2_2;
 *     w2_i = w2_i - d*u1_i;  u2 = w2 / |w2| with the same norm and the same rule;  u3 = u1 x u2.
 *  4. Candidates:  Ra[i][j] = (u2_i*v1_j - u1_i*v2_j) + u3_i*v3_j;   Rb[i][j] = (u1_i*v2_j - u2_i*v1_j) + u3_i*v3_j;
 *     c = 0: (Ra, u3), 1: (Ra, -u3), 2: (Rb, u3), 3: (Rb, -u3).
 *  5. Cheirality of one record under (R, t):  q = ((x - cx)/fx, (y - cy)/fy, 1),  b = ((x' - cx)/fx, (y' - cy)/fy, 1);
 *     a_i = (R[i][0]*q0 + R[i][1]*q1) + R[i][2];   aa = (a0*a0 + a1*a1) + a2*a2, and bb = b.b, ab = a.b, at = a.t, bt = b.t of
 *     the same shape;  det = aa*bb - ab*ab;  n1 = ab*bt - bb*at;  n2 = aa*bt - ab*at.  The record is IN FRONT (of both
 *     cameras) iff det > 0 && n1 > 0 && n2 > 0; a record with NaN coordinates is not.  front[c] = the number of such records,
 *     an integer: no order of summation matters.  (Negating t negates n1 and n2 exactly.)
 *  6. Selection: the candidate with the largest front, the lowest c on ties; every count 0, or an invalid pair: best = -1
 *     and R, t all zero.  valid: steps 1 - 3 produced candidates (an invalid pair's candidates are all zero).
 *  7. The point of record i under the winner, the midpoint of the two rays' closest points:  l1 = n1/det;  l2 = n2/det;
 *     c_i = l2*b_i - t_i;   P_j = (R[0][j]*c0 + R[1][j]*c1) + R[2][j]*c2;   X_j = 0.5 * (l1*q_j + P_j).   X is written as
 *     computed for every considered record: NaN for one that is not trusted, whatever IEEE gives when det == 0 - except
 *     that every NaN is written as the quiet NaN 0x7ff8000000000000 (IEEE fixes neither the sign nor the payload of a NaN).
 * The result depends neither on how the records are split over lanes and workgroups nor on vslam_ctx_set_f32_fused /
 * vslam_ctx_set_matrix_path. */
typedef struct {
    double fx, fy, cx, cy; /* all finite, fx and fy positive */
} vslam_pose_params;
typedef struct {
    double R[9];
    double t[3];
    uint32_t front; /* records in front of both cameras under this candidate */
    int32_t valid;
} vslam_pose_cand; /* 104 bytes */
typedef struct {
    double R[9];        /* the winner; all zero when best < 0 */
    double t[3];
    uint32_t n_matches; /* min(match_counts[j], match_cap): the records considered */
    uint32_t n_front;   /* the winner's count, 0 when best < 0 */
    int32_t best;       /* winning candidate 0 .. 3, -1: none */
    int32_t valid;      /* steps 1 - 3 produced candidates */
} vslam_pose;           /* 112 bytes */
/* Like vslam_epipolar_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;          /* = sizeof(vslam_pose_out) */
    vslam_pose* poses;           /* [n_pairs], required */
    size_t poses_bytes;
    vslam_pose_cand* candidates; /* [n_pairs][4] optional */
    size_t candidates_bytes;
    double* points;              /* [n_pairs][match_cap][3] optional: X of record i; rows i < n_matches of a pair with best >= 0
                                  * are written, every other row is left untouched */
    size_t points_bytes;
    uint64_t* front_bits;        /* [n_pairs][(match_cap + 63) / 64] optional: bit i % 64 of word i / 64 = record i is in front
                                  * under the winner; the first (n_matches + 63) / 64 words of a pair are written (all zero when
                                  * best < 0), the rest untouched */
    size_t front_bits_bytes;
} vslam_pose_out;
/* Pair j reads models[j] and the lists as vslam_epipolar_dev does (DEVICE pointers).  Asynchronous on the context stream,
 * never waits on the host (the counts are read on the device, the grids are sized from the capacities); scratch belongs to
 * the context.  VSLAM_ERR_INVALID before any launch - and before the context is looked at - for a null pointer, a wrong
 * struct_size, an undersized buffer, match_cap / query_cap / train_cap == 0, n_pairs outside 0 .. 65535 (0 does nothing), an
 * intrinsic that is not finite, fx or fy not positive; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for
 * stream capture. */
int vslam_pose_dev(vslam_ctx* ctx, const vslam_epipolar* models, const vslam_match* matches, const uint32_t* match_counts,
                   uint32_t match_cap, const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points,
                   uint32_t train_cap, int n_pairs, const vslam_pose_params* params, const vslam_pose_out* out);
/* One pair in HOST memory, synchronous (a convenience path: device buffers per call).  model and pose are required;
 * candidates [4], points [n_matches][3] and front_bits [(n_matches + 63) / 64] are each optional (NULL).  n_query / n_train are
 * the capacities the indices are checked against.  Errors as for vslam_pose_dev. */
int vslam_pose_host(vslam_ctx* ctx, const vslam_epipolar* model, const vslam_match* matches, size_t n_matches,
                    const vslam_point* query_points, size_t n_query, const vslam_point* train_points, size_t n_train,
                    const vslam_pose_params* params, vslam_pose* pose, vslam_pose_cand* candidates, double* points,
                    uint64_t* front_bits);

/* ---------------------------------------------------------------- pose from homography: planar pairs get R, t and points
 * The pairs the degeneracy gate took away from vslam_pose_dev.  For a pair whose matches a homography explains, H itself
 * holds the motion: H ~ K (R + t n^T / d) K^-1 for a plane with unit normal n at distance d in the query frame.  This stage
 * decomposes models[j].H (the `models` buffer of vslam_homography_dev) into its four (R, t, n) candidates, votes on them with
 * the records H supports, and writes the SAME buffers vslam_pose_dev writes - poses, points, front_bits, same shapes, same
 * rules - for the pairs it selects, and for no other pair: passed the very buffers vslam_pose_dev just wrote from the gated
 * models, the call fills exactly the holes the gate made, and vslam_chain_dev, vslam_resect_dev, vslam_tracks_dev and
 * vslam_bundle_dev read on without a new code path.  The match list must be the list the pose stage of the batch read (the
 * intended one is the inliers / inlier_counts / inlier_cap of vslam_epipolar_dev, which the gate leaves in place): row i of
 * points and bit i of front_bits then mean the same record for every pair, however it got its pose.  A pure rotation has no
 * baseline to triangulate from: it gets its rotation in `info`, the "no pose" record in poses, and still breaks the
 * trajectory's segment.  H is decomposed as it is given (vslam_hrefit_dev refits it first), no plane carried from pair to pair.
 * Convention, coordinates, "trusted" and
 * m = min(match_counts[j], match_cap) are the relative pose section's; the arithmetic is fixed here so that a CPU can restate
 * it bit for bit (tests/hposeref.py): IEEE f64, every + - * / sqrt rounded on its own (no fused multiply-add), sums left to
 * right as written.  Matrices are row-major, M[i][j] = M[3*i + j]; V[:, k] is column k.
 *
 * Pair j is SELECTED iff models[j].best >= 0 && (!only_degenerate || models[j].degenerate != 0).  A pair that is not
 * selected has kind NONE, and its poses[j], its point rows and its front words are left untouched.
 *
 *  1. Euclidean homography A = K^-1 H K, the right factor first, as step 1 of the relative pose section forms F K:
 *       G[i][0] = H[i][0]*fx;  G[i][1] = H[i][1]*fy;  G[i][2] = (H[i][0]*cx + H[i][1]*cy) + H[i][2];
 *       A[0][j] = (G[0][j] - cx*G[2][j]) / fx;  A[1][j] = (G[1][j] - cy*G[2][j]) / fy;  A[2][j] = G[2][j].
 *     No sign step: the sign rule of the homography section makes (H x)_2 > 0 on H's inliers, and the third row of K^-1 is
 *     (0, 0, 1), so (A q)_2 > 0 for the ray q of every inlier already.
 *  2. Eigenvalues and scaling: S = A^T A and the six Jacobi sweeps of step 4 of the two-view model, verbatim, give the
 *     diagonal d and V.  Three conditional exchanges bring them into descending order - positions (0, 1), then (1, 2), then
 *     (0, 1): d[a] and d[b], and columns a and b of V, change places iff d[b] > d[a] (a stable sort: on ties the lower index
 *     stays first; a NaN never moves).  L1 = d[0], L2 = d[1], L3 = d[2] and v1 = V[:, 0], v2 = V[:, 1], v3 = V[:, 2] afterwards.
 *     L2 not finite or not positive: the pair is INVALID - kind NONE, and poses[j] is the "no pose" record.  s = sqrt(L2);
 *     A[i][j] = A[i][j] / s;  l1 = L1 / L2;  l3 = L3 / L2;  spread = l1 - l3.  (The ordering gives l3 <= 1 <= l1 exactly.)
 *  3. Kind.  !(spread >= min_spread): ROTATION.  With c1, c2 the first two columns of the scaled A, by the rules of step 3
 *     of the relative pose section: r1 = c1 / |c1|, |c| = sqrt((c_0*c_0 + c_1*c_1) + c_2*c_2);  g = (r1_0*c2_0 + r1_1*c2_1) +
 *     r1_2*c2_2;  w_i = c2_i - g*r1_i;  r2 = w / |w|;  r3 = r1 x r2 (the cross product of that section);  R[i][0] = r1_i,
 *     R[i][1] = r2_i, R[i][2] = r3_i.  A norm that is zero or not finite: the pair is invalid.  poses[j] is the "no pose"
 *     record, the front words are zero, no point row is written; the rotation is in info[j].  Otherwise the kind is PLANE.
 *  4. PLANE candidates (Ma, Soatto, Kosecka, Sastry: products, square roots and cross products only).
 *     a = sqrt(1 - l3);  b = sqrt(l1 - 1);  c = sqrt(spread);  u+_i = (a*v1_i + b*v3_i) / c;  u-_i = (a*v1_i - b*v3_i) / c.
 *     For u = u+ and for u = u-:  m1_i = (A[i][0]*v2_0 + A[i][1]*v2_1) + A[i][2]*v2_2;  m2_i likewise from u;  m3 = m1 x m2;
 *     n = v2 x u;  R[i][j] = (m1_i*v2_j + m2_i*u_j) + m3_i*n_j;  An_i = (A[i][0]*n_0 + A[i][1]*n_1) + A[i][2]*n_2;  Rn_i
 *     likewise from R;  T_i = An_i - Rn_i;  |T| = sqrt((T_0*T_0 + T_1*T_1) + T_2*T_2);  t = T / |T|.  |T| zero or not finite:
 *     both candidates of that sign are invalid (all zero, never voted for).
 *     c = 0: (R+, t+, n+), 1: (R+, -t+, -n+), 2: (R-, t-, n-), 3: (R-, -t-, -n-).
 *  5. Vote.  A record is SUPPORTED iff it passes the inlier test of the homography section (trusted, forward and backward)
 *     under models[j].H, models[j].G and params.max_dist2, word for word.  n_support counts them (kinds PLANE and ROTATION).
 *     front[c] = the number of supported records that are IN FRONT by step 5 of the relative pose section under (R_c, t_c)
 *     with K, and have nq = (n_0*q0 + n_1*q1) + n_2 > 0 for n = n_c (q the query ray of that step).  Negating (t, n) negates
 *     n1, n2 and nq exactly, so for c = 1 and c = 3 the test is det > 0 && n1 < 0 && n2 < 0 && nq < 0 with the values of c - 1.
 *  6. Selection.  The WINNER w is the valid candidate with the largest front, the lowest c on ties; every count 0: best = -1
 *     and poses[j] is the "no pose" record.  runner = the largest front[c] over c != w.
 *     ambiguous = uint64(runner) * ambiguous_den >= uint64(ambiguous_num) * front[w].  An ambiguous pair with priors != NULL
 *     and priors[j].best >= 0 is RESOLVED: over the valid candidates with uint64(front[c]) * ambiguous_den >= uint64(ambiguous_num) *
 *     front[w], c ascending, the score is s_c = (((P[0]*R_c[0] + P[1]*R_c[1]) + P[2]*R_c[2]) + ... ) + P[8]*R_c[8] with
 *     P = priors[j].R; the first such candidate is kept, and a later one replaces it iff its score is > the kept score (a
 *     NaN never replaces and is never replaced).  The kept candidate is then `best`, otherwise best = w.
 *     poses[j] carries candidate `best` (R, t, n_front = front[best], best, valid = 1) iff the pair is not ambiguous or is
 *     resolved; an ambiguous pair that is not resolved gets the "no pose" record, and info[j] reports the vote either way: a
 *     coin flip never enters the trajectory.  The "no pose" record: R, t zero, n_front = 0, best = -1, n_matches = m, valid =
 *     1 for kind PLANE and 0 otherwise.
 *  7. Points and bits of a selected pair with poses[j].best >= 0: for a supported record, step 7 of the relative pose section
 *     verbatim under (poses[j].R, poses[j].t), and its front bit is "in front" by step 5 of that section; a record that is
 *     not supported gets front bit 0 and the quiet NaN in all three coordinates, as an untrusted record does there.  Rows
 *     i < m are written; with best < 0 no row is written and the first (m + 63) / 64 front words are zero.
 * Every NaN this stage writes is the quiet NaN 0x7ff8000000000000.  Every count is an integer and no floating-point sum
 * crosses records: the result depends neither on how the records are split over lanes and workgroups nor on
 * vslam_ctx_set_f32_fused / vslam_ctx_set_matrix_path. */
#define VSLAM_HPOSE_NONE 0
#define VSLAM_HPOSE_PLANE 1
#define VSLAM_HPOSE_ROTATION 2
typedef struct {
    vslam_pose_params K;
    double max_dist2;       /* H's symmetric transfer bound (the max_dist2 vslam_homography_dev ran with); finite and positive */
    double min_spread;      /* spread below this: a pure rotation; finite and positive */
    uint32_t ambiguous_num; /* ambiguous: runner / front[w] >= ambiguous_num / ambiguous_den */
    uint32_t ambiguous_den; /* > 0 */
    int32_t only_degenerate; /* 0: every pair with an H; 1: only the pairs the verdict judged degenerate */
    uint32_t reserved;      /* must be 0 */
} vslam_hpose_params;       /* 64 bytes */
typedef struct {
    double R[9];
    double t[3];
    double n[3];    /* the plane's unit normal in the query frame */
    uint32_t front; /* supported records in front of both cameras and of the plane under this candidate */
    int32_t valid;
} vslam_hpose_cand; /* 128 bytes */
typedef struct {
    double R[9];           /* PLANE: the rotation of candidate `best` (zero when best < 0); ROTATION: the pair's rotation */
    double n[3];           /* PLANE: the unit normal of candidate `best` in the query frame */
    double inv_d;          /* PLANE: |T| of candidate `best`, the baseline over the plane's distance */
    double spread;         /* l1 - l3 (PLANE and ROTATION) */
    uint32_t n_matches;    /* min(match_counts[j], match_cap): the records considered */
    uint32_t n_support;    /* the records H supports */
    uint32_t front;        /* the vote's winner's count */
    uint32_t front_runner; /* the runner-up's count */
    int32_t kind;          /* VSLAM_HPOSE_NONE / _PLANE / _ROTATION; NONE: the whole record is zero */
    int32_t best;          /* the candidate chosen, 0 .. 3 (the vote's winner unless resolved); -1: none */
    int32_t ambiguous;
    int32_t resolved;
} vslam_hpose;             /* 144 bytes */
/* Like vslam_pose_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;           /* = sizeof(vslam_hpose_out) */
    vslam_pose* poses;            /* [n_pairs], required; written for selected pairs only */
    size_t poses_bytes;
    vslam_hpose* info;            /* [n_pairs], required; written for every pair */
    size_t info_bytes;
    vslam_hpose_cand* candidates; /* [n_pairs][4] optional; written for every pair (all zero unless the kind is PLANE) */
    size_t candidates_bytes;
    double* points;               /* [n_pairs][match_cap][3] optional: as vslam_pose_out's, selected pairs only */
    size_t points_bytes;
    uint64_t* front_bits;         /* [n_pairs][(match_cap + 63) / 64] optional: as vslam_pose_out's, selected pairs only */
    size_t front_bits_bytes;
} vslam_hpose_out;
/* Pair j reads models[j] (H, G, best, degenerate), the lists as vslam_pose_dev does and, when given, priors[j] (R and best;
 * DEVICE pointers, priors may be NULL; priors must not overlap poses or any other output: pair j's prior is read while other
 * pairs' poses are written - to use the previous pairs' poses, pass a copy).  Asynchronous on the context stream, never waits on the host (the counts, the models
 * and with them every pair's kind are read on the device, the grids are sized from the capacities); scratch belongs to the
 * context.  VSLAM_ERR_INVALID before any launch - and before the context is looked at - for a null pointer, a wrong
 * struct_size, n_pairs outside 0 .. 65535 (0 does nothing), an intrinsic that is not finite, fx or fy not positive, a max_dist2
 * or min_spread that is not finite or not positive, ambiguous_den == 0, only_degenerate outside 0 .. 1, reserved != 0,
 * match_cap / query_cap / train_cap == 0, an undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for
 * stream capture. */
int vslam_hpose_dev(vslam_ctx* ctx, const vslam_homography* models, const vslam_match* matches, const uint32_t* match_counts,
                    uint32_t match_cap, const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points,
                    uint32_t train_cap, int n_pairs, const vslam_pose* priors, const vslam_hpose_params* params,
                    const vslam_hpose_out* out);
/* The same call over HOST memory, synchronous (a convenience path: device buffers per call): matches [n_pairs][match_cap],
 * query_points [n_pairs][query_cap], train_points [n_pairs][train_cap].  poses, points and front_bits go up before the call, so
 * what it leaves untouched comes back as it went in.  Errors as for vslam_hpose_dev. */
int vslam_hpose_host(vslam_ctx* ctx, const vslam_homography* models, const vslam_match* matches, const uint32_t* match_counts,
                     uint32_t match_cap, const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points,
                     uint32_t train_cap, int n_pairs, const vslam_pose* priors, const vslam_hpose_params* params,
                     const vslam_hpose_out* out);

/* ---------------------------------------------------------------- trajectory: pair poses chained into one world frame
 * The step after the relative pose.  vslam_pose_dev leaves every pair with |t| = 1 and its points in its own query camera's
 * frame and unit; this step recovers the scale of pair j relative to pair j - 1 from the points both pairs triangulated and
 * chains the poses into one frame of coordinates.  The inputs are exactly what vslam_pose_dev read and wrote for n_pairs
 * CONSECUTIVE pairs (pair j: query frame j, train frame j + 1): poses [n_pairs], matches [n_pairs][match_cap], match_counts,
 * points [n_pairs][match_cap][3], front_bits [n_pairs][(match_cap + 63) / 64], and point_cap, the capacity of the frames' point
 * lists: pair j's train indices and pair j + 1's query indices address the same set.  The point lists themselves are not
 * read - the link is made by index.  The arithmetic is fixed here so that a CPU can restate it bit for bit
 * (tests/chainref.py): IEEE f64, every + - * / sqrt rounded on its own, sums left to right as written, matrices row-major.
 *
 * m_j = min(match_counts[j], match_cap).  Record i of pair j is LIVE iff i < m_j, poses[j].best >= 0, bit i of the pair's
 * front_bits is set, and query < point_cap and train < point_cap (as unsigned).  A record that is not live is never read
 * through.
 *
 *  1. Link.  For pair j >= 1 and point index k < point_cap, prev_j[k] is the LOWEST i such that record i of pair j - 1 is live
 *     and its train == k.  A live record b of pair j with query == q is linked to a = prev_j[q] if that exists.  Pair 0 has
 *     no links.
 *  2. Ratio of a linked record, with (R, t) = poses[j - 1], X = points[j - 1][a], Z = points[j][b]:
 *       Y_i = ((R[i][0]*X0 + R[i][1]*X1) + R[i][2]*X2) + t_i;   dY = sqrt((Y0*Y0 + Y1*Y1) + Y2*Y2), dZ likewise from Z;
 *       r = dY / dZ.   The ratio is USABLE iff r > 0 && r < +inf (a NaN fails both).
 *  3. Median.  n_links[j] = the number of usable ratios of pair j (n_links[0] = 0); ratio[j] = the usable ratio of 0-based
 *     rank (n_links[j] - 1) >> 1 in ascending order - the lower median -, 0.0 when n_links[j] == 0.  A value of the multiset:
 *     no arithmetic, so neither the record order nor the split over workgroups plays a part.
 *  4. Walk, sequential over j = 0 .. n_pairs - 1.  valid_j = poses[j].best >= 0;  linked_j = j >= 1 && valid_{j-1} && valid_j
 *     && n_links[j] >= min_links.  Not linked - a segment starts: segment = j, scale = 1, W = I, w = 0.  Linked, with
 *     (R, t, s) = (poses[j - 1].R, poses[j - 1].t, scale_{j-1}):  segment_j = segment_{j-1};  scale_j = scale_{j-1} * ratio[j];
 *       W_j[i][k] = (R[i][0]*W[0][k] + R[i][1]*W[1][k]) + R[i][2]*W[2][k]   (W = W_{j-1});
 *       w_j[i] = ((R[i][0]*w0 + R[i][1]*w1) + R[i][2]*w2) + s*t_i           (w = w_{j-1}).
 *     Convention: x_camera_j = W_j x_world + w_j; the world is the query camera of the segment's first pair, in that pair's
 *     unit.  The query camera's centre: C_i = -((W[0][i]*w0 + W[1][i]*w1) + W[2][i]*w2) (the negation is exact: -0.0 at a
 *     segment start).  Ct: the same expression for the train camera (R_j W_j, R_j w_j + scale_j t_j), formed by the two
 *     product rules above with (R, t, s) = (poses[j].R, poses[j].t, scale_j).  An invalid pair gets W = I, w = C = Ct = 0,
 *     scale = 1, segment = j, linked = 0, valid = 0.  ratio and n_links are those of step 3 whether the pair is linked or not.
 *  5. Map.  For a valid pair j and every i < m_j: record i live: c_k = scale_j*X_k - w_k, X = points[j][i];
 *     M_i = (W[0][i]*c0 + W[1][i]*c1) + W[2][i]*c2, the point in world coordinates; not live: the quiet NaN three times.  Rows
 *     past m_j, and all rows of an invalid pair, are left untouched.
 * Every NaN in a double output of this section is written as 0x7ff8000000000000.
 *
 * Scratch (the context's): the link table, (n_pairs - 1) * point_cap * 4 bytes - 67 MB at 255 x 65536 -, and the ratio keys,
 * (n_pairs - 1) * match_cap * 8 bytes - 134 MB at 255 x 65536; an allocation that fails is VSLAM_ERR_NOMEM. */
typedef struct {
    uint32_t min_links; /* >= 1: the usable ratios a pair needs to be chained to the pair before it */
} vslam_chain_params;
typedef struct {
    double W[9], w[3]; /* x_camera_j = W x_world + w (the query camera of pair j) */
    double C[3], Ct[3]; /* centres of the query and the train camera in the world */
    double scale;      /* pair j's unit of length in the segment's: world length = scale * pair length */
    double ratio;      /* step 3 */
    uint32_t n_links;  /* step 3 */
    int32_t segment;   /* the pair the segment started at */
    int32_t linked;
    int32_t valid;
} vslam_chain; /* 176 bytes */
/* Like vslam_pose_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size; /* = sizeof(vslam_chain_out) */
    vslam_chain* chain; /* [n_pairs], required: the walk's records */
    size_t chain_bytes;
    double* map;        /* [n_pairs][match_cap][3] optional: step 5 */
    size_t map_bytes;
    int32_t* links;     /* [n_pairs][match_cap] optional: for i < m_j the linked a, or -1; the rest untouched */
    size_t links_bytes;
    double* ratios;     /* [n_pairs][match_cap] optional: for i < m_j r as computed when linked, the quiet NaN otherwise */
    size_t ratios_bytes;
} vslam_chain_out;
/* DEVICE pointers, all required.  Asynchronous on the context stream, never waits on the host (the counts are read on the
 * device, the grids are sized from the capacities).  VSLAM_ERR_INVALID before any launch - and before the context is looked
 * at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does nothing; 1 is one segment with no links),
 * min_links == 0, match_cap or point_cap == 0, an undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP device.
 * Not for stream capture. */
int vslam_chain_dev(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                    uint32_t match_cap, const double* points, const uint64_t* front_bits, uint32_t point_cap, int n_pairs,
                    const vslam_chain_params* params, const vslam_chain_out* out);
/* The same call over HOST arrays, all n_pairs pairs at once, synchronous (a convenience path: device buffers per call).  The
 * rows the device call leaves untouched keep the caller's bytes.  Errors as for vslam_chain_dev. */
int vslam_chain_host(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                     uint32_t match_cap, const double* points, const uint64_t* front_bits, uint32_t point_cap, int n_pairs,
                     const vslam_chain_params* params, const vslam_chain_out* out);

/* ---------------------------------------------------------------- resection: camera pose from the previous pair's 3-D points
 * Beside the two-view pose: the camera of frame j + 1 relative to frame j, estimated from the points pair j - 1 triangulated
 * (3-D) and their observations in frame j + 1 (2-D) - a RANSAC absolute pose.  The translation comes out in pair j - 1's unit,
 * so |t| estimates the trajectory's ratio[j] directly, and a pair whose F is degenerate (vslam_homography_dev's gate) still
 * gets a pose.  A fixed number of hypotheses, no adaptive stop; the refinement over all inliers is a stage of its own
 * (vslam_resect_refine_dev); the result is not fed into vslam_chain_dev.  n_pairs CONSECUTIVE pairs (pair j: query frame j, train frame j + 1).
 *   Structure side: exactly what vslam_chain_dev reads - poses, matches, match_counts, match_cap, points, front_bits, point_cap -
 *   and the LIVE rule of the trajectory section, verbatim.
 *   Observation side: obs_matches [n_pairs][obs_cap] with obs_counts - any match list of the pair: the same buffers as the
 *   structure side (the F inliers), or the raw list vslam_match_dev wrote, which is the one to use for a pair the gate left
 *   without a model -, train_points [n_pairs][train_cap] laid out as for vslam_epipolar_dev (set j = frame j + 1), and the
 *   intrinsics.  n_obs = min(obs_counts[j], obs_cap) records are considered.
 * The arithmetic is fixed here so that a CPU can restate it bit for bit (tests/resectref.py): IEEE f64, every + - * / sqrt
 * rounded on its own (no fused multiply-add), sums left to right as written, matrices row-major.  mix() and the Gauss-Jordan
 * step are those of the two-view geometry section, the Jacobi sweeps and the cross product those of the pose section.
 *
 *  1. Link.  Step 1 of the trajectory section, unchanged: for pair j >= 1, prev_j[k] is the lowest live record of pair j - 1
 *     whose train == k.  Pair 0 has no links and no correspondences.
 *  2. Correspondence of observation record b < n_obs of pair j >= 1, (query, train) its indices as unsigned.  link_b =
 *     prev_j[query] when query < point_cap and that exists, else -1 (a pair j - 1 with poses[j - 1].best < 0 has no live
 *     record, so no links).  The record is a CANDIDATE iff link_b >= 0, train < train_cap and the train point's octave is in
 *     0 .. 31.  With a = link_b, (R, t) = poses[j - 1], X = points[j - 1][a]:
 *       Y_i = ((R[i][0]*X0 + R[i][1]*X1) + R[i][2]*X2) + t_i     (the point in frame j's camera, in pair j - 1's unit);
 *       (x', y') the exact coordinate of the train point (two-view section);  u = (x' - cx)/fx;  v = (y' - cy)/fy.
 *     The record is USABLE iff it is a candidate and Y0, Y1, Y2 are all finite.  The usable records, in list order, are the
 *     pair's dense list of n_corr correspondences {Y, u, v, b}.
 *  3. Sample.  base = mix(mix(seed + j) + h); draw d = 0, 1, ... gives r = mix(base + d) and the index (uint64(r) * n_corr) >> 32
 *     into the dense list, kept if it is not among the indices kept so far; the sample is the first 6 kept, in that order.
 *     Fewer than 6 after 64 draws: invalid.  n_corr < 6: every hypothesis is invalid.
 *  4. Model from the 6 correspondences - a calibrated direct linear transform.
 *     a. c_k = (((((Y0_k + Y1_k) + Y2_k) + Y3_k) + Y4_k) + Y5_k) / 6 for k = 0, 1, 2 (Yi the i-th sample point);
 *        r_i = sqrt((e0*e0 + e1*e1) + e2*e2) with e_k = Yi_k - c_k;  d = (((((r0 + r1) + r2) + r3) + r4) + r5) / 6;  d == 0: invalid;
 *        s = 1.7320508075688772 / d;  the normalised point N_k = (Yi_k - c_k) * s.
 *     b. The 12 x 12 matrix a, unknowns p = the 3 x 4 matrix [Mn | mn] row-major:
 *          row 2i     = [N0, N1, N2, 1,  0, 0, 0, 0,  -(u*N0), -(u*N1), -(u*N2), -u];
 *          row 2i + 1 = [0, 0, 0, 0,  N0, N1, N2, 1,  -(v*N0), -(v*N1), -(v*N2), -v].
 *     c. Step 3 of the two-view model over 12 rows and 12 columns, steps k = 0 .. 10: the same scan (rows r >= k ascending, then
 *        the columns no earlier step chose ascending, strictly larger replaces, starting at 0), the same validity rules (no
 *        choice, or an infinite pivot: invalid), the same row operations over all twelve columns and all twelve rows.  With
 *        `free` the column no step chose: p[free] = 1, p[c_k] = -a[k][free].
 *     d. The normalisation undone:  M[i][k] = p[4i + k] * s;   m_i = p[4i + 3] - ((M[i][0]*c0 + M[i][1]*c1) + M[i][2]*c2).
 *     e. det = (M[0][0]*(M[1][1]*M[2][2] - M[1][2]*M[2][1]) - M[0][1]*(M[1][0]*M[2][2] - M[1][2]*M[2][0]))
 *              + M[0][2]*(M[1][0]*M[2][1] - M[1][1]*M[2][0]).   det zero or not finite: invalid.  det < 0: all twelve entries of
 *        M and m are negated.
 *  5. Rotation - steps 2 and 3 of the pose section applied to M.  S = M^T M and the six Jacobi sweeps, verbatim, give S and V;
 *     k = the index of the smallest S[k][k] (lowest on ties), p < q the other two;  v1 = V[:, p], v2 = V[:, q], v3 = v1 x v2.
 *     w1_i = (M[i][0]*v1_0 + M[i][1]*v1_1) + M[i][2]*v1_2;  n1 = sqrt((w1_0*w1_0 + w1_1*w1_1) + w1_2*w1_2);  n1 zero or not
 *     finite: invalid;  u1 = w1 / n1.  w2 likewise from v2;  g = (u1_0*w2_0 + u1_1*w2_1) + u1_2*w2_2;  w2_i = w2_i - g*u1_i;
 *     n2 = the norm of that w2, same rule;  u2 = w2 / n2;  u3 = u1 x u2.  w3 from v3 as w1 from v1, n3 its norm (no rule).
 *       R[i][j] = (u1_i*v1_j + u2_i*v2_j) + u3_i*v3_j;   lambda = ((n1 + n2) + n3) / 3;   lambda zero or not finite: invalid;
 *       t_i = m_i / lambda.   A hypothesis any of whose twelve R, t is not finite is invalid.
 *  6. Inlier test of a correspondence under (R, t), no division:
 *       Z_i = ((R[i][0]*Y0 + R[i][1]*Y1) + R[i][2]*Y2) + t_i;   ex = (u*Z2 - Z0)*fx;   ey = (v*Z2 - Z1)*fy;
 *     an inlier iff Z2 > 0 && (ex*ex + ey*ey) < max_dist2 * (Z2*Z2): the squared reprojection error in pixels^2.
 *  7. Selection: the valid hypothesis with the most inliers, the lowest h on ties.  Counts are integers, so the result does
 *     not depend on how the correspondences are split over lanes and workgroups.
 * Convention: x_{j+1} = R x_j + t.  Every NaN in a double output of this section is written as 0x7ff8000000000000.
 *
 * Scratch (the context's): the link table, (n_pairs - 1) * point_cap * 4 bytes, 24 bytes per observation record of capacity
 * (n_pairs * obs_cap), 48 more without a correspondences buffer, and n_pairs * n_hypotheses * 104 bytes without a hypotheses
 * buffer; an allocation that fails is VSLAM_ERR_NOMEM. */
typedef struct {
    uint32_t n_hypotheses; /* 1 .. 65535 */
    uint32_t seed;
    double max_dist2;      /* squared reprojection error in pixels^2, finite and positive */
    vslam_pose_params K;   /* all finite, fx and fy positive */
} vslam_resect_params;
typedef struct {
    double R[9];      /* all zero when not valid */
    double t[3];
    uint32_t inliers;
    int32_t valid;
} vslam_resect_hyp; /* 104 bytes */
typedef struct {
    double Y[3];       /* step 2: the point in frame j's camera */
    double u, v;       /* the calibrated observation in frame j + 1 */
    uint32_t b;        /* the observation record it came from */
    uint32_t reserved; /* 0 */
} vslam_resect_corr; /* 48 bytes */
typedef struct {
    double R[9];        /* the winner; all zero when best < 0 */
    double t[3];        /* in pair j - 1's unit */
    uint32_t n_obs;     /* min(obs_counts[j], obs_cap): the records considered */
    uint32_t n_corr;    /* usable correspondences, 0 for pair 0 */
    uint32_t n_inliers; /* the winner's count, 0 when best < 0 */
    int32_t best;       /* winning hypothesis, -1: none (always for pair 0) */
    uint32_t n_valid;   /* hypotheses that produced a model */
    uint32_t reserved;  /* 0 */
} vslam_resect;         /* 120 bytes */
/* Like vslam_chain_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;       /* = sizeof(vslam_resect_out) */
    vslam_resect* models;     /* [n_pairs], required */
    size_t models_bytes;
    uint64_t* inlier_bits;    /* [n_pairs][(obs_cap + 63) / 64] optional: bit b % 64 of word b / 64 = observation record b is
                               * usable and an inlier of the winner; the first (n_obs + 63) / 64 words of a pair are written
                               * (all zero when best < 0), the rest untouched */
    size_t inlier_bits_bytes;
    vslam_resect_hyp* hypotheses; /* [n_pairs][n_hypotheses] optional: every hypothesis with its count */
    size_t hypotheses_bytes;
    vslam_resect_corr* correspondences; /* [n_pairs][obs_cap] optional: the first n_corr rows of a pair are written */
    size_t correspondences_bytes;
    int32_t* links;           /* [n_pairs][obs_cap] optional: for b < n_obs link_b of step 2 (-1 in pair 0); the rest untouched */
    size_t links_bytes;
} vslam_resect_out;
/* DEVICE pointers, all inputs required.  Asynchronous on the context stream, never waits on the host (the counts are read on
 * the device, the grids are sized from the capacities); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch -
 * and before the context is looked at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does nothing),
 * n_hypotheses outside 1 .. 65535, a max_dist2 that is not finite or not positive, an intrinsic that is not finite, fx or fy
 * not positive, match_cap / point_cap / obs_cap / train_cap == 0, an undersized buffer; then VSLAM_ERR_HIP when there is no
 * usable HIP device.  Not for stream capture. */
int vslam_resect_dev(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                     uint32_t match_cap, const double* points, const uint64_t* front_bits, uint32_t point_cap,
                     const vslam_match* obs_matches, const uint32_t* obs_counts, uint32_t obs_cap, const vslam_point* train_points,
                     uint32_t train_cap, int n_pairs, const vslam_resect_params* params, const vslam_resect_out* out);
/* The same call over HOST arrays, all n_pairs pairs at once, synchronous (a convenience path: device buffers per call).  The
 * rows the device call leaves untouched keep the caller's bytes.  Errors as for vslam_resect_dev. */
int vslam_resect_host(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                      uint32_t match_cap, const double* points, const uint64_t* front_bits, uint32_t point_cap,
                      const vslam_match* obs_matches, const uint32_t* obs_counts, uint32_t obs_cap, const vslam_point* train_points,
                      uint32_t train_cap, int n_pairs, const vslam_resect_params* params, const vslam_resect_out* out);

/* ---------------------------------------------------------------- resection: Gauss-Newton refinement over all inliers
 * The step after vslam_resect_dev: the winning minimal hypothesis is refined by Gauss-Newton on the reprojection error of ALL
 * its inliers (a motion-only bundle adjustment), the inliers are classified again under the new pose, and so on for a fixed
 * number of rounds; a round whose pose has fewer inliers - or as many and no lower cost - is dropped, so the result never has
 * fewer inliers than the input.  Inputs: the `models` buffer vslam_resect_dev wrote and the dense `correspondences` list of
 * the same call ([n_pairs][obs_cap], 16-byte aligned); the link, the gather and the calibration are not repeated.  Pair j
 * reads n_corr = min(models_in[j].n_corr, obs_cap) rows {Y, u, v, b} and n_obs = min(models_in[j].n_obs, obs_cap).  IEEE f64,
 * every + - * / rounded on its own (no fused multiply-add, no sqrt, no sin / cos), sums of a few terms left to right as
 * written, matrices row-major (tests/resectrefineref.py restates it bit for bit).
 *
 * A row is a MEMBER under (R, t) iff it passes the inlier test of step 6 of the resection section under (R, t) with max_dist2:
 *   Z_i = ((R[i][0]*Y0 + R[i][1]*Y1) + R[i][2]*Y2) + t_i;   ex = (u*Z2 - Z0)*fx;   ey = (v*Z2 - Z1)*fy;
 *   Z2 > 0 && (ex*ex + ey*ey) < max_dist2 * (Z2*Z2).
 *
 * The ordered sum SUM(term) is that of the refit section, verbatim, over the dense rows r < n_corr instead of the records i <
 * m: a row that is not a member contributes +0.0; block b covers rows 4096*b .. 4096*b + 4095; slot l (0 .. 255) starts at
 * +0.0 and adds the terms of rows 4096*b + 256*k + l, k = 0 .. 15, skipping every row at or past n_corr; then for h = 128, 64,
 * 32, 16, 8, 4, 2, 1: s_l = s_l + s_(l+h) for every l < h, all from the values of the step before; B_b = s_0; the pair's sum is
 * ((B_0 + B_1) + B_2) + ... over the (n_corr + 4095) / 4096 blocks, and +0.0 for n_corr = 0.  It depends on n_corr and the terms
 * only: not on obs_cap, not on the grid, not on the device.
 *
 * EVALUATE (R, t) - 29 ordered sums.  Per member, with Z as above:
 *   iz = 1 / Z2;   px = Z0*iz;   py = Z1*iz;   rx = (px - u)*fx;   ry = (py - v)*fy;   pxy = px*py;
 *   Jx = { fx*(-pxy),  fx*(1 + px*px),  fx*(-py),  fx*iz,  fx*0.0,  fx*(-(px*iz)) };
 *   Jy = { fy*(-(1 + py*py)),  fy*pxy,  fy*px,  fy*0.0,  fy*iz,  fy*(-(py*iz)) }
 * - the rows of the Jacobian of (rx, ry) for the left perturbation Z' = Z + w x Z + tau, unknowns (w0, w1, w2, tau0, tau1, tau2).
 *   H[p][q] = SUM(Jx_p*Jx_q + Jy_p*Jy_q) for p <= q, row-major (21 sums), mirrored below the diagonal;
 *   g_p = SUM(Jx_p*rx + Jy_p*ry) (6 sums);   cost = SUM(rx*rx + ry*ry);   n = SUM(1.0), the member count, exact.
 *
 * STEP from (R, t), H, g:
 *  a. The 6 x 7 matrix a = [H | -g].  Step 3 of the two-view model over 6 rows, steps k = 0 .. 5: the pivot is the entry of
 *     largest |a[r][c]| over rows r >= k and the columns c < 6 no earlier step chose, the same scan (r ascending, then c
 *     ascending, strictly larger replaces, starting at 0: a zero or a NaN is never chosen), the same validity rules (no choice,
 *     or an infinite pivot: invalid); rows k and r are swapped; every entry of row k is divided by the pivot; for every other
 *     row i, with g = a[i][c]: a[i][c'] = a[i][c'] - g * a[k][c'] for all seven c'.  c_k = c.  d[c_k] = a[k][6].  Any of the six
 *     d not finite: invalid.  w = (d0, d1, d2), tau = (d3, d4, d5).
 *  b. The Cayley rotation of w.  a_i = w_i / 2;   q = (a0*a0 + a1*a1) + a2*a2;   e = 1 - q;   den = 1 + q;
 *       D[i][i] = (e + 2*(a_i*a_i)) / den;
 *       D[0][1] = (2*(a0*a1) - 2*a2) / den;   D[1][0] = (2*(a1*a0) + 2*a2) / den;   D[0][2] = (2*(a0*a2) + 2*a1) / den;
 *       D[2][0] = (2*(a2*a0) - 2*a1) / den;   D[1][2] = (2*(a1*a2) - 2*a0) / den;   D[2][1] = (2*(a2*a1) + 2*a0) / den.
 *  c. R_new[i][j] = (D[i][0]*R[0][j] + D[i][1]*R[1][j]) + D[i][2]*R[2][j];
 *     t_new_i = ((D[i][0]*t0 + D[i][1]*t1) + D[i][2]*t2) + tau_i.   Any of the twelve not finite: invalid.
 *
 * Per pair.  A pair with models_in[j].best < 0 is copied through, byte for byte, with stop = 5 and n_before = n_after =
 * accepted = 0, cost_before = cost_after = 0.  Otherwise (R, t)_cur = models_in[j]'s; EVALUATE it: n_cur = n, cost_cur = cost,
 * n_before = n_cur, cost_before = cost_cur, accepted = 0.  Round 1 .. rounds, until a stop:
 *  1. n_cur < 6: stop = 1.
 *  2. STEP from (R, t)_cur with the H and g of its evaluation; invalid: stop = 3.
 *  3. EVALUATE (R, t)_new.  It is kept iff n_new > n_cur, or n_new == n_cur && cost_new < cost_cur: then (R, t)_cur = (R,
 *     t)_new with its n, cost, H and g, and accepted += 1; otherwise stop = 4.
 * All rounds done without a stop: stop = 0.  After a stop the pair does nothing more.  Output: models[j] = models_in[j] with
 * R, t = (R, t)_cur and n_inliers = n_cur (every other field copied); n_after = n_cur >= n_before, cost_after = cost_cur.  Every
 * NaN in a double output of a pair with best >= 0 is written as 0x7ff8000000000000.  inlier_bits: bit b % 64 of word b / 64 is
 * set iff best >= 0, b < n_obs and a row r < n_corr with corr.b == b is a member under the output pose.
 *
 * Scratch (the context's): n_pairs * ((obs_cap + 4095) / 4096) * 232 bytes of block sums and n_pairs * 344 bytes of state; an
 * allocation that fails is VSLAM_ERR_NOMEM. */
typedef struct {
    uint32_t rounds;     /* 1 .. 8 */
    double max_dist2;    /* as vslam_resect_params: squared reprojection error in pixels^2, finite and positive */
    vslam_pose_params K; /* all finite, fx and fy positive (fx, fy enter the arithmetic) */
} vslam_resect_refine_params;
typedef struct {
    uint32_t n_before, n_after;     /* members under the input pose / under the output pose */
    uint32_t accepted;              /* rounds whose pose was kept */
    int32_t stop;                   /* 0: ran all rounds, 1: fewer than 6 members, 3: the step was invalid, 4: the new pose was
                                     * not better, 5: no input model */
    double cost_before, cost_after; /* SUM(rx*rx + ry*ry) in pixels^2 under the input pose / under the output pose */
} vslam_resect_refine;              /* 32 bytes */
/* Like vslam_resect_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;        /* = sizeof(vslam_resect_refine_out) */
    vslam_resect* models;      /* [n_pairs], required; may be the very pointer passed as models_in, must not otherwise overlap it */
    size_t models_bytes;
    vslam_resect_refine* info; /* [n_pairs] optional */
    size_t info_bytes;
    uint64_t* inlier_bits;     /* [n_pairs][(obs_cap + 63) / 64] optional: indexed by observation record b as
                                * vslam_resect_out.inlier_bits; the first (n_obs + 63) / 64 words of a pair are written (all zero
                                * when best < 0), the rest untouched */
    size_t inlier_bits_bytes;
} vslam_resect_refine_out;
/* DEVICE pointers.  Asynchronous on the context stream, never waits on the host (the counts are read on the device, the grids
 * are sized from the capacity, a stopped pair's workgroups leave at once); scratch belongs to the context.  VSLAM_ERR_INVALID
 * before any launch - and before the context is looked at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535
 * (0 does nothing), rounds outside 1 .. 8, a max_dist2 that is not finite or not positive, an intrinsic that is not finite, fx
 * or fy not positive, obs_cap == 0, correspondences not 16-byte aligned, an undersized buffer, models overlapping models_in
 * without being equal to it; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for stream capture. */
int vslam_resect_refine_dev(vslam_ctx* ctx, const vslam_resect* models_in, const vslam_resect_corr* correspondences, uint32_t obs_cap,
                            int n_pairs, const vslam_resect_refine_params* params, const vslam_resect_refine_out* out);
/* The same call over HOST arrays, all n_pairs pairs at once, synchronous (a convenience path: device buffers per call; the
 * alignment rule does not apply).  The words of inlier_bits the device call leaves untouched keep the caller's bytes.  Errors
 * as for vslam_resect_refine_dev. */
int vslam_resect_refine_host(vslam_ctx* ctx, const vslam_resect* models_in, const vslam_resect_corr* correspondences, uint32_t obs_cap,
                             int n_pairs, const vslam_resect_refine_params* params, const vslam_resect_refine_out* out);

/* ---------------------------------------------------------------- tracks: points linked across pairs, triangulated from all views
 * The step after vslam_chain_dev.  The trajectory links pair j to pair j - 1 by index for one distance ratio and forgets the
 * link; this step keeps it: a TRACK is one scene point, the records of consecutive pairs that saw it, and one 3-D position
 * computed from all of its views at once (the point that is closest, in the least-squares sense, to every view's ray).  The
 * inputs are what vslam_chain_dev read, minus `points` - poses [n_pairs], matches [n_pairs][match_cap], match_counts, front_bits
 * [n_pairs][(match_cap + 63) / 64], point_cap -, the chain records [n_pairs] that call wrote, and the frames' point lists
 * frame_points [n_pairs + 1][point_cap]: frame j is the query of pair j and the train of pair j - 1.  The arithmetic is fixed here
 * so that a CPU can restate it bit for bit (tests/tracksref.py): IEEE f64, every + - * / rounded on its own (no fused
 * multiply-add), sums left to right as written, matrices row-major.
 *
 *  1. Live records and prev_j: m_j, the LIVE rule and step 1 of the trajectory section, verbatim.  For pair j >= 1 and point
 *     index k < point_cap, prev_j[k] is the lowest live record of pair j - 1 whose train == k.
 *  2. Continuation, one-to-one.  For j >= 1 with chain[j].linked != 0: a live record b of pair j for which a = prev_j[query_b]
 *     exists is a CANDIDATE for a.  next_{j-1}[a] is the LOWEST candidate b for a (an integer minimum: the same in any order).
 *     Record b CONTINUES a iff next_{j-1}[a] == b.  A live record that continues nothing is a HEAD.  A track is a head and
 *     the chain of records that continue it: record (j0, i0), then (j0 + 1, next_{j0}[i0]), and so on while that exists.  A
 *     record has at most one successor and at most one predecessor, so a track is a path, never a tree - also on lists where
 *     several records share a query or a train index; every live record lies on exactly one track.  A track never crosses a
 *     pair with linked == 0: it lies in one segment, one world frame.
 *     A track of L records (j0, i0) .. (j0 + L - 1, i_{L-1}) has n_views = L + 1 VIEWS, in this order:
 *       view p < L: the query side of record p: pixel = frame_points[j][query], camera (W, w) = (chain[j].W, chain[j].w), centre
 *         C = chain[j].C, with j = j0 + p;
 *       view L: the train side of the last record, j = j0 + L - 1: pixel = frame_points[j + 1][train], camera
 *         W[i][k] = (R[i][0]*Wj[0][k] + R[i][1]*Wj[1][k]) + R[i][2]*Wj[2][k],   w_i = ((R[i][0]*wj0 + R[i][1]*wj1) + R[i][2]*wj2) + s*t_i
 *         with (R, t) = (poses[j].R, poses[j].t), (Wj, wj, s) = (chain[j].W, chain[j].w, chain[j].scale) - the trajectory's two
 *         product rules -, centre C = chain[j].Ct.
 *  3. Normal equations.  Six sums A00, A01, A02, A11, A12, A22 and three sums g0, g1, g2, each starting at 0.0, each view
 *     added in the order of step 2.  Per view:
 *       (x, y): the exact coordinate of the view's point record p (two-view geometry section) when p.octave is in 0 .. 31; NaN,
 *         NaN otherwise, carried through;
 *       q0 = (x - cx)/fx;  q1 = (y - cy)/fy;
 *       d_i = (W[0][i]*q0 + W[1][i]*q1) + W[2][i]           (the ray W^T (q0, q1, 1) in the world);
 *       dd = (d0*d0 + d1*d1) + d2*d2;   e_i = d_i / dd;
 *       P_ii = 1.0 - e_i*d_i;   P_ik = 0.0 - e_i*d_k for i < k, and P_ki = P_ik           (the projector I - d d^T / dd);
 *       A_ik = A_ik + P_ik for i <= k;   g_i = g_i + ((P_i0*C0 + P_i1*C1) + P_i2*C2).
 *  4. Point.  The cofactors of the symmetric A:
 *       c00 = A11*A22 - A12*A12;   c01 = A02*A12 - A01*A22;   c02 = A01*A12 - A02*A11;
 *       c11 = A00*A22 - A02*A02;   c12 = A01*A02 - A00*A12;   c22 = A00*A11 - A01*A01;       c_ki = c_ik;
 *       det = (A00*c00 + A01*c01) + A02*c02;    X_i = ((c_i0*g0 + c_i1*g1) + c_i2*g2) / det.
 *     SOLVED iff det > 0 && det < +inf && X0, X1, X2 are all finite.  X and det are written as computed.
 *  5. Reprojection, per view under that view's camera and with (u, v) = (q0, q1) of step 3, no division:
 *       Z_i = ((W[i][0]*X0 + W[i][1]*X1) + W[i][2]*X2) + w_i;    ex = (u*Z2 - Z0)*fx;    ey = (v*Z2 - Z1)*fy;
 *     the view is OK iff Z2 > 0 && (ex*ex + ey*ey) < max_dist2 * (Z2*Z2).  n_ok = the number of ok views, an integer: no
 *     order matters.  GOOD iff solved && n_ok == n_views && n_views >= min_views.
 * Every NaN in a double output of this section is written as 0x7ff8000000000000.  Nothing here refines X (vslam_bundle_dev
 * does) or lists the tracks densely: a track lives at its head's slot.
 *
 * Scratch (the context's): the two tables prev and next, (n_pairs - 1) * (point_cap + match_cap) * 4 bytes; an allocation that
 * fails is VSLAM_ERR_NOMEM. */
typedef struct {
    vslam_pose_params K; /* all finite, fx and fy positive */
    double max_dist2;    /* squared reprojection error in pixels^2, finite and positive */
    uint32_t min_views;  /* >= 2: the views a good track needs */
    uint32_t reserved;   /* not read */
} vslam_tracks_params;
typedef struct {
    double X[3];       /* step 4, in the world frame of the track's segment */
    double det;        /* step 4 */
    uint32_t n_views;  /* records on the track + 1 */
    uint32_t n_ok;     /* step 5 */
    uint32_t status;   /* bit 0: solved, bit 1: good */
    uint32_t reserved; /* 0 */
} vslam_track;         /* 48 bytes */
typedef struct {
    uint32_t head_record; /* the record of pair j - pos the track starts at */
    uint32_t pos;         /* this record's position on the track: j - the head's pair */
} vslam_track_ref;        /* 8 bytes */
typedef struct {
    uint32_t n_heads;   /* tracks that start in pair j */
    uint32_t n_good;    /* of those, the good ones */
    uint32_t max_views; /* the most views of a track that starts in pair j, 0 without one */
    uint32_t reserved;  /* 0 */
} vslam_track_summary;  /* 16 bytes */
/* Like vslam_chain_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;  /* = sizeof(vslam_tracks_out) */
    vslam_track* tracks; /* [n_pairs][match_cap], required: row i < m_j of pair j holds the track whose head is record i; a record
                          * that is not a head gets X = det = the quiet NaN and n_views = n_ok = status = 0; rows past m_j are
                          * left untouched */
    size_t tracks_bytes;
    vslam_track_ref* refs; /* [n_pairs][match_cap] optional, the observation -> track table: for i < m_j the track record i lies
                            * on, all ones in both fields for a record that is not live; the rest untouched */
    size_t refs_bytes;
    uint64_t* good_bits; /* [n_pairs][(match_cap + 63) / 64] optional: bit i % 64 of word i / 64 = record i is the head of a good
                          * track; the first (m_j + 63) / 64 words of a pair are written, the rest untouched */
    size_t good_bits_bytes;
    vslam_track_summary* summary; /* [n_pairs] optional: integer counts, every record written */
    size_t summary_bytes;
} vslam_tracks_out;
/* DEVICE pointers, all inputs required.  Asynchronous on the context stream, never waits on the host (the counts are read on
 * the device, the grids are sized from the capacities); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch -
 * and before the context is looked at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does nothing; 1
 * gives tracks of two views), an intrinsic that is not finite, fx or fy not positive, a max_dist2 that is not finite or not
 * positive, min_views < 2, match_cap or point_cap == 0, an undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP
 * device.  Not for stream capture. */
int vslam_tracks_dev(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                     uint32_t match_cap, const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain,
                     const vslam_point* frame_points, const vslam_tracks_params* params, const vslam_tracks_out* out);
/* The same call over HOST arrays, all n_pairs pairs at once, synchronous (a convenience path: device buffers per call).  The
 * rows the device call leaves untouched keep the caller's bytes.  Errors as for vslam_tracks_dev. */
int vslam_tracks_host(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                      uint32_t match_cap, const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain,
                      const vslam_point* frame_points, const vslam_tracks_params* params, const vslam_tracks_out* out);

/* ---------------------------------------------------------------- bundle adjustment: alternating point and camera Gauss-Newton
 * The step after vslam_tracks_dev: cameras and track points are moved together, by resection-intersection.  Given the
 * cameras, every track's point takes one Gauss-Newton step on the reprojection error of its member views (A); given the points,
 * every camera takes one Gauss-Newton step on the reprojection error of its member rows (B); this repeats `sweeps` times.
 * Points are independent of each other given the cameras and cameras given the points, so each half-sweep is an exact block
 * step: no coupled linear system, no damping, no robust kernel.  Inputs: everything vslam_tracks_dev read - poses, matches,
 * match_counts, match_cap, front_bits, point_cap, n_pairs, chain, frame_points -, tracks_in [n_pairs][match_cap], the rows that
 * call wrote, refs [n_pairs][match_cap], the table it wrote (required here), and optionally cams_in [n_pairs].  IEEE f64,
 * every + - * / rounded on its own (no fused multiply-add, no sqrt), sums of a few terms left to right as written, matrices
 * row-major (tests/bundleref.py restates it bit for bit).
 *
 * Cameras.  Pair j is VALID iff poses[j].best >= 0.  The unknowns are the train cameras T_j = (W, w) of the valid pairs: T_j is
 * the camera of frame j + 1 in the world of pair j's segment, x_camera = W x_world + w.  The QUERY CAMERA of pair j is T_{j-1}
 * when j >= 1 and chain[j].linked != 0, and the held camera (I, 0) of a segment start otherwise: that is the gauge, the first
 * camera of every segment never moves.  The overall scale of a segment is left free: the cost does not depend on it and every
 * block step is well posed without fixing it.  T_j starts as cams_in[j]'s W, w when cams_in is given (so the cams of one call
 * feed the next; resect-refined poses can come in the same way), and otherwise as view L of the tracks section, step 2, formed
 * from chain[j] and poses[j] by the trajectory's two product rules - chain[j + 1].W, w bit for bit where pair j + 1 is linked.
 * An invalid pair's camera is (I, 0), takes no step and is read by nothing that is live.
 *
 * Tracks and views.  m_j, LIVE, prev, next, HEAD and the path of a track: the tracks section, steps 1 and 2, verbatim.  The
 * track headed by live head record (j0, i0) is ACTIVE iff tracks_in[j0][i0] has status bit 0 set and n_views >= min_views.  Its
 * point X starts as that row's X.  Its L records give L + 1 views in the order of step 2: view 0 has the query camera of pair
 * j0 and the pixel frame_points[j0][query]; view p, 1 <= p < L, has T_{j0+p-1} and frame_points[j0 + p][query of record p];
 * view L has T_{j0+L-1} and frame_points[j0 + L][train of the last record].  (u, v) = (q0, q1) of step 3 of the tracks section
 * (NaN for an untrusted point record).  A view is a MEMBER under (camera, X) iff it passes step 5 of the tracks section:
 *   Z_i = ((W[i][0]*X0 + W[i][1]*X1) + W[i][2]*X2) + w_i;   ex = (u*Z2 - Z0)*fx;   ey = (v*Z2 - Z1)*fy;
 *   Z2 > 0 && (ex*ex + ey*ey) < max_dist2 * (Z2*Z2)       (a NaN pixel fails it).
 *
 * One sweep, `sweeps` times:
 *  A. Point step, per active track, under the cameras as they stand.  EVALUATE-POINT (X): ten sums H00, H01, H02, H11, H12,
 *     H22, g0, g1, g2, cost, each starting at +0.0, and the integer n, the views added in track order, a view that is not a
 *     member skipped.  Per member, with Z as above:
 *       iz = 1 / Z2;   px = Z0*iz;   py = Z1*iz;   rx = (px - u)*fx;   ry = (py - v)*fy;   sx = fx*iz;   sy = fy*iz;
 *       ax_k = sx*(W[0][k] - px*W[2][k]);   ay_k = sy*(W[1][k] - py*W[2][k])       (k = 0, 1, 2: the Jacobian of (rx, ry) by X);
 *       H_kl = H_kl + (ax_k*ax_l + ay_k*ay_l) for k <= l;   g_k = g_k + (ax_k*rx + ay_k*ry);   cost = cost + (rx*rx + ry*ry);   n += 1.
 *     1. EVALUATE-POINT (X) gives n_cur, cost_cur (in the first sweep also n_before, cost_before).
 *     2. n_cur < 2: skipped += 1.
 *     3. Otherwise the cofactors c_ik and det of the symmetric H by the expressions of the tracks section, step 4 (A = H), and
 *        delta_i = -(((c_i0*g0 + c_i1*g1) + c_i2*g2) / det).  det not > 0, det not < +inf or a delta not finite: invalid += 1.
 *     4. Otherwise X_new_i = X_i + delta_i; EVALUATE-POINT (X_new) gives n_new, cost_new; X = X_new iff n_new > n_cur, or n_new
 *        == n_cur && cost_new < cost_cur (the refinement's rule): accepted += 1; otherwise rejected += 1.
 *  B. Camera step, per valid pair j, all cameras from the points step A left.  The ROWS of camera T_j, n_rows = m_j + h_j of them:
 *       r < m_j: the train side of record r of pair j: pixel frame_points[j + 1][train];
 *       m_j <= r < m_j + h_j, with h_j = m_{j+1} when j + 1 < n_pairs and chain[j + 1].linked != 0, else 0: the query side of
 *       record r - m_j of pair j + 1, counted only if that record is a head: pixel frame_points[j + 1][query].
 *     The row of record i of pair jj COUNTS iff the record is live, (h, pos) = refs[jj][i] has pos <= jj and h < m_{jj-pos} (and
 *     pos == 0 where a head is required), and the row (jj - pos, h) of the output tracks - the rows of tracks_in, X as step A
 *     left it - has status bit 0 set and n_views >= min_views; its Y is that row's X, its (u, v) the pixel's.  So every (track,
 *     frame) observation is one row of exactly one camera, or a held camera's view 0.  A row that does not count adds +0.0.
 *     EVALUATE (W, w) is the 29 ordered sums of the resect-refine section, verbatim, with (R, t) = (W, w) over these rows: n_rows
 *     in place of n_corr, blocks of 4096 rows, the same slots and tree, block sums left to right.  STEP is that section's, on (W, w).
 *     1. EVALUATE (T_j) gives n_cur, cost_cur, H, g (the first sweep's are n_before, cost_before).
 *     2. n_cur < 6: skipped += 1.
 *     3. Otherwise STEP; invalid: invalid += 1.
 *     4. Otherwise EVALUATE the candidate; T_j = the candidate iff n_new > n_cur, or n_new == n_cur && cost_new < cost_cur:
 *        accepted += 1; otherwise rejected += 1.
 * A camera or point that was rejected tries again in the next sweep - the other block has moved; there are no permanent stops.
 * After the last sweep: EVALUATE (T_j) once more gives the camera's n_after, cost_after; EVALUATE-POINT (X) gives the point's.
 *
 * Outputs.  tracks: rows i < m_j of every pair are the rows of tracks_in, byte for byte, except the head rows of active tracks:
 * X = the refined point, n_ok = the point's n_after (the ok views of step 5 of the tracks section under the final cameras),
 * status = (solved ? 1 : 0) | (good ? 2 : 0) with solved = det > 0 && det < +inf && X0, X1, X2 all finite and good = solved &&
 * n_ok == n_views && n_views >= min_views, and det, n_views, reserved copied.  cams[j]: W, w, the centre C_i = -((W[0][i]*w0 +
 * W[1][i]*w1) + W[2][i]*w2) (the trajectory's expression), the counters and costs; an invalid pair gets W = I, w = C = +0.0,
 * skipped = sweeps and every other field 0.  point_info: the row at the head slot of every active track; nothing else is
 * written.  member_bits: for record i < m_j, bit i % 64 of word i / 64 of half 0 = the row "query side of record i" counts
 * (no head required) and is a member under the query camera of pair j and the output; of half 1 the same for the train side
 * under T_j; an invalid pair's words are zero.  Every NaN in a double output written by this section is 0x7ff8000000000000.
 * Nothing here is fed back into vslam_chain_dev or the resection.
 *
 * Scratch (the context's): the two tables of the tracks stage, n_pairs * ((2 * match_cap + 4095) / 4096) * 232 bytes of block
 * sums and n_pairs * 240 bytes of camera state; an allocation that fails is VSLAM_ERR_NOMEM. */
typedef struct {
    vslam_pose_params K; /* all finite, fx and fy positive (fx, fy enter the arithmetic) */
    double max_dist2;    /* squared reprojection error in pixels^2, finite and positive */
    uint32_t min_views;  /* >= 2: the views an active track needs */
    uint32_t sweeps;     /* 1 .. 64 */
} vslam_bundle_params;   /* 48 bytes */
typedef struct {
    double W[9], w[3];              /* T_j: x_camera = W x_world + w */
    double C[3];                    /* its centre in the world */
    uint32_t n_before, n_after;     /* member rows at the first evaluation / under the output */
    uint32_t accepted, rejected, invalid, skipped; /* sweeps by outcome: they add up to `sweeps` */
    double cost_before, cost_after; /* SUM(rx*rx + ry*ry) in pixels^2 at the first evaluation / under the output */
} vslam_bundle_cam;                 /* 160 bytes, a multiple of 8 */
typedef struct {
    uint32_t n_before, n_after;     /* member views at the first evaluation / under the output */
    uint32_t accepted, rejected, invalid, skipped; /* sweeps by outcome */
    double cost_before, cost_after;
} vslam_bundle_point;               /* 40 bytes */
/* Like vslam_tracks_out: every pointer with the bytes behind it, checked before anything is launched. */
typedef struct {
    size_t struct_size;           /* = sizeof(vslam_bundle_out) */
    vslam_track* tracks;          /* [n_pairs][match_cap], required; may be the very pointer passed as tracks_in, must not otherwise
                                   * overlap it; rows past m_j are left untouched */
    size_t tracks_bytes;
    vslam_bundle_cam* cams;       /* [n_pairs], required */
    size_t cams_bytes;
    vslam_bundle_point* point_info; /* [n_pairs][match_cap] optional: written at the head slots of active tracks only */
    size_t point_info_bytes;
    uint64_t* member_bits;        /* [n_pairs][2][(match_cap + 63) / 64] optional: the first (m_j + 63) / 64 words of each half of
                                   * a pair are written, the rest untouched */
    size_t member_bits_bytes;
} vslam_bundle_out;
/* DEVICE pointers; cams_in may be NULL, every other input is required.  Asynchronous on the context stream, never waits on
 * the host (the counts are read on the device, the grids are sized from the capacities; the number of launches depends on
 * `sweeps` alone); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch - and before the context is looked at -
 * for a null required pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does nothing), sweeps outside 1 .. 64,
 * min_views < 2, a max_dist2 that is not finite or not positive, an intrinsic that is not finite, fx or fy not positive,
 * match_cap or point_cap == 0, an undersized buffer, tracks overlapping tracks_in without being equal to it; then VSLAM_ERR_HIP
 * when there is no usable HIP device.  Not for stream capture. */
int vslam_bundle_dev(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                     uint32_t match_cap, const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain,
                     const vslam_point* frame_points, const vslam_track* tracks_in, const vslam_track_ref* refs,
                     const vslam_bundle_cam* cams_in, const vslam_bundle_params* params, const vslam_bundle_out* out);
/* The same call over HOST arrays, all n_pairs pairs at once, synchronous (a convenience path: device buffers per call).  The
 * rows and words the device call leaves untouched keep the caller's bytes.  Errors as for vslam_bundle_dev. */
int vslam_bundle_host(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                      uint32_t match_cap, const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain,
                      const vslam_point* frame_points, const vslam_track* tracks_in, const vslam_track_ref* refs,
                      const vslam_bundle_cam* cams_in, const vslam_bundle_params* params, const vslam_bundle_out* out);

/* ---------------------------------------------------------------- place recognition
 * The first question of loop closure: which EARLIER frame shows the same place as this one?  Three calls answer it from the
 * descriptor buffers of vslam_detect_batch_dev: a vocabulary of K descriptor rows sampled from the data (vslam_vocab_sample_dev),
 * the nearest vocabulary row - the "visual word" - of every descriptor with a histogram of words per frame (vslam_words_dev), and a
 * short list of loop candidates per frame from the histograms (vslam_place_dev).  The word search is the matcher's arithmetic; all
 * that follows it is unsigned integer arithmetic, so a CPU restates every byte (tests/placeref.py).  Verifying a candidate is the
 * caller's: a one-pair vslam_match_dev / vslam_epipolar_dev call on the two sets.  No output depends on vslam_ctx_set_f32_fused or
 * vslam_ctx_set_matrix_path, or on scheduling (the histogram is built with integer atomic adds only).
 *
 *   Vocabulary.  Word k < K is a copy of one row of the n_sets descriptor sets: the set is s = k % n_sets, the row is
 *     r = (((k / n_sets) * 2654435761) mod 2^32) % rows_s with rows_s = min(counts[s], cap).  The word is DEFINED iff rows_s > 0
 *     and the row's `defined` byte is not 0 (a set without `defined`: every row is).  vocab[k] is the row's 512 bytes, or 128 times
 *     +0.0 for a word that is not defined.  Duplicate words and NaN words are allowed: the word rule never selects the second of
 *     two equal words, and never a NaN word.
 *   Words.  For every set f < n_sets and row q < min(counts[f], cap): word = `index` of the descriptor matching section's
 *     selection, with the K vocabulary rows as the train rows of every set - d2 as defined there, word index ascending, strict <,
 *     so ties keep the lowest index and a NaN or +inf distance never wins; a word whose vocab_defined byte is 0 is skipped; a query
 *     row whose `defined` byte is 0 gets -1.  There is no second nearest and no ratio test.  word_dist2 is that d2 (+inf with -1).
 *     REAL DESCRIPTORS CONTAIN ALL-NaN ROWS WHOSE `defined` BYTE IS SET: every distance of such a row is NaN, so it gets word -1
 *     and counts in no histogram bin.  A vocabulary row that holds a NaN is a dead word: no row ever gets it, its bin stays 0.
 *     hist[f][k] = the number of rows q of set f with word k; the call zeroes all of hist first.
 *   Place.  hist_q [nq][K] are the histograms of the frames q_first + i, hist_db [nd][K] those of the frames db_first + j (the
 *     two may be one buffer: a batch searched in itself; or a running database of earlier batches with its own offset).
 *       df_k    = the number of db frames j with hist_db[j][k] > 0
 *       w_k     = 0 if df_k == 0, else the bit length of nd / df_k (integer division): 1 .. 32, an integer idf
 *       S(i, j) = sum over k of w_k * min(hist_q[i][k], hist_db[j][k]);  Sq_i = sum of w_k * hist_q[i][k];  Sd_j likewise:
 *                 each sum is formed in uint64 (it cannot wrap: 2^16 words * 32 * 2^32) and then saturated to 2^31 - 1
 *       j is ELIGIBLE for i iff db_first + j + min_gap <= q_first + i, in uint64
 *       with N = max(Sq_i, Sd_j), an eligible j is ACCEPTED iff N > 0 and S >= min_score and S * den >= num * N (uint64)
 *       candidate a RANKS BEFORE b iff S_a * N_b > S_b * N_a (uint64), equal products: the lower db frame first
 *     candidates[i] holds the first min(accepted, max_candidates) accepted frames of i in rank order as {db_first + j, S, N}.
 *     The norm is the LARGER self-score: under the smaller one a frame with few descriptors is swallowed by any frame with many. */
typedef struct {
    size_t struct_size;  /* = sizeof(vslam_words_out) */
    int32_t* words;      /* [n_sets][cap] optional; rows past a set's count are left untouched */
    size_t words_bytes;
    float* word_dist2;   /* [n_sets][cap] optional; rows past a set's count are left untouched */
    size_t word_dist2_bytes;
    uint32_t* hist;      /* [n_sets][K] optional; written whole */
    size_t hist_bytes;
} vslam_words_out;
typedef struct {
    int32_t frame;        /* db_first + j */
    uint32_t score, norm; /* S(i, j), N */
} vslam_place_cand;      /* 12 bytes */
typedef struct {
    uint32_t min_gap;
    uint32_t max_candidates; /* c, 1 .. 8 */
    uint32_t num, den;       /* den > 0 */
    uint32_t min_score;
    uint32_t reserved;       /* 0 */
} vslam_place_params;       /* 24 bytes */
typedef struct {
    size_t struct_size;           /* = sizeof(vslam_place_out) */
    vslam_place_cand* candidates; /* [nq][c] optional, needs cand_counts; slots past a frame's count are left untouched */
    size_t candidates_bytes;
    uint32_t* cand_counts;        /* [nq] optional, <= c */
    size_t cand_counts_bytes;
    uint32_t* weights;            /* [K] optional */
    size_t weights_bytes;
    uint32_t* self_q;             /* [nq] optional */
    size_t self_q_bytes;
    uint32_t* self_db;            /* [nd] optional */
    size_t self_db_bytes;
    uint32_t* scores;             /* [nq][nd] optional: S(i, j) of EVERY (i, j), eligible or not */
    size_t scores_bytes;
} vslam_place_out;
/* sets: DEVICE pointers, as for vslam_match_dev (points are not read); vocab [K][128] f32, 16-byte aligned, and vocab_defined [K]
 * are DEVICE outputs, both required.  1 <= n_sets <= 65535, 1 <= K <= 65536.  Asynchronous on the context stream, never waits on
 * the host.  VSLAM_ERR_INVALID before any launch - and before the context is looked at - for a null pointer, a set without
 * desc, counts or a capacity, a misaligned desc or vocab, n_sets or K out of range, an undersized buffer; then VSLAM_ERR_HIP when
 * there is no usable HIP device.  Not for stream capture. */
int vslam_vocab_sample_dev(vslam_ctx* ctx, const vslam_desc_sets* sets, int n_sets, uint32_t K, float* vocab, size_t vocab_bytes,
                           uint8_t* vocab_defined, size_t vocab_defined_bytes);
/* sets, vocab [K][128] (16-byte aligned) and vocab_defined [K] (NULL = every word defined): DEVICE pointers, the vocabulary a
 * caller's own or vslam_vocab_sample_dev's.  0 <= n_sets <= 65535 (0 does nothing), 1 <= K <= 65536; at least one output.
 * Asynchronous on the context stream, never waits on the host (the counts are read on the device, the grids are sized from the
 * capacities); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch - and before the context is looked at - for
 * a null struct, a wrong struct_size, n_sets or K out of range, a set without desc, counts or a capacity, a misaligned desc or
 * vocab, no output at all, an undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for stream capture. */
int vslam_words_dev(vslam_ctx* ctx, const vslam_desc_sets* sets, int n_sets, const float* vocab, const uint8_t* vocab_defined,
                    uint32_t K, const vslam_words_out* out);
/* The same call over HOST arrays, synchronous (a convenience path: device buffers per call): desc [n_sets][cap][128], defined
 * [n_sets][cap] or NULL, counts [n_sets], vocab [K][128], vocab_defined [K] or NULL, and the pointers of `out`.  The rows the
 * device call leaves untouched keep the caller's bytes.  Errors as for vslam_words_dev (no alignment is asked of host arrays). */
int vslam_words_host(vslam_ctx* ctx, const float* desc, const uint8_t* defined, const uint32_t* counts, uint32_t cap, int n_sets,
                     const float* vocab, const uint8_t* vocab_defined, uint32_t K, const vslam_words_out* out);
/* DEVICE pointers.  nq, nd <= 65535 (nq == 0 does nothing; nd == 0: an empty database, every weight and count 0), 1 <= K <=
 * 65536, q_first + nq and db_first + nd at most 2^31 (a frame id fits `frame`).  Asynchronous on the context stream, never
 * waits on the host; scratch belongs to the context (nq * nd scores when `scores` is absent, K weights, nq + nd self-scores).
 * A 16 x 16 tile of (i, j) without an eligible pair is not scored when `scores` is absent.  VSLAM_ERR_INVALID before any launch
 * - and before the context is looked at - for a null struct or histogram, a wrong struct_size, nq, nd, K or a frame id out of
 * range, max_candidates outside 1 .. 8, den == 0, reserved != 0, no output at all, candidates without cand_counts, an
 * undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for stream capture. */
int vslam_place_dev(vslam_ctx* ctx, const uint32_t* hist_q, uint32_t nq, uint32_t q_first, const uint32_t* hist_db, uint32_t nd,
                    uint32_t db_first, uint32_t K, const vslam_place_params* params, const vslam_place_out* out);
/* The same call over HOST arrays, synchronous.  The candidate slots the device call leaves untouched keep the caller's bytes.
 * Errors as for vslam_place_dev. */
int vslam_place_host(vslam_ctx* ctx, const uint32_t* hist_q, uint32_t nq, uint32_t q_first, const uint32_t* hist_db, uint32_t nd,
                     uint32_t db_first, uint32_t K, const vslam_place_params* params, const vslam_place_out* out);

/* ---------------------------------------------------------------- vocabulary training
 * A sampled word (place recognition, above) is one noisy observation of one landmark.  vslam_vocab_kmeans_dev trains a vocabulary
 * by Lloyd's algorithm: `rounds` times, every descriptor row goes to its nearest word and every word becomes the mean of its rows.
 * The assignment is the Words rule above, unchanged; the mean is an f64 sum in a fixed order, every operation rounded on its own
 * (no fused multiply-add, no reassociation), so a CPU restates every byte (tests/kmeansref.py).  No output depends on
 * vslam_ctx_set_f32_fused or vslam_ctx_set_matrix_path, on scheduling, on the grid or on the scratch layout.
 *
 *   Rows in use: (f, q) with f < n_sets and q < min(counts[f], cap).  V_0 = vocab_in.  vocab_defined is an input, the same in every
 *   round, and is never written; NULL: every word is defined.  Round t = 1 .. rounds:
 *     1. Assign.  w_t(f, q) = the word of row (f, q) by the Words paragraph of the place recognition section against V_(t-1) and
 *        vocab_defined: -1 for a row whose `defined` byte is 0 or whose every distance is NaN or +inf.
 *     2. Report.  assigned = the rows in use with w_t >= 0.  changed = the rows in use with w_t != w_(t-1); in round 1 every row in
 *        use counts, assigned or not.  If t > 1 and changed == 0 the call has CONVERGED: this round writes its record with ran = 1
 *        and `empty` by step 6 from this round's assignment (which is the previous round's), updates nothing, and every later
 *        round writes {0, 0, 0, 0}.  (The same assignment would give the same sums, so stopping changes no byte of the vocabulary.)
 *     3. Members.  The members of word k are the rows in use with w_t == k, ordered by set ascending, then by row ascending; N_k is
 *        their number.  A row with w_t == -1 is a member of no word.
 *     4. Ordered sum.  For each word k and each d < 128: block b holds the members 256 b .. min(256 b + 255, N_k - 1).
 *        B_b = +0.0, then B_b = B_b + (double)x[d] for the block's members x in member order; sum = B_0, then sum = sum + B_b for
 *        b = 1, 2, .. in ascending order.  Every f64 addition is rounded to nearest even on its own.  The sum depends on the
 *        member list alone.
 *     5. Update.  N_k == 0: V_t[k] = V_(t-1)[k], byte for byte (an undefined word, a dead word, the second of two equal words
 *        and a word no row is nearest to all keep their bytes in that round; once the first of two equal words has moved, the
 *        second is a word of its own).  Otherwise V_t[k][d] = (float)(sum / (double)N_k): one f64 division, one rounding to f32
 *        (nearest even; a subnormal result is kept).  The arithmetic is plain IEEE: a NaN or infinite sum would give a NaN or
 *        infinite entry, and by the Words rule such a word is dead from the next round on - no row gets it, so it keeps those
 *        bytes.  No row can bring that about: a member has a finite d2, so its norm and with it every entry is finite, and the
 *        mean of finite f32 values is finite.  A word is dead only if vocab_in made it so.
 *     6. empty = the words k whose vocab_defined byte is not 0 (NULL: every k) with N_k == 0; a dead word counts.
 *   out->vocab = V_t and out->sizes[k] = N_k of the last round t that updated (round 1 always updates).  The rows are never
 *   written.  n_sets == 0: vocab = vocab_in, every size 0, every report record {0, 0, 0, 0}. */
typedef struct {
    uint32_t rounds;   /* 1 .. 64 */
    uint32_t reserved; /* 0 */
} vslam_kmeans_params; /* 8 bytes */
typedef struct {
    uint32_t assigned, changed, empty, ran;
} vslam_kmeans_round;  /* 16 bytes */
typedef struct {
    size_t struct_size;         /* = sizeof(vslam_kmeans_out) */
    float* vocab;               /* [K][128] required, 16-byte aligned; may be vocab_in itself (in place), no other overlap */
    size_t vocab_bytes;
    uint32_t* sizes;            /* [K] optional */
    size_t sizes_bytes;
    vslam_kmeans_round* report; /* [rounds] optional */
    size_t report_bytes;
} vslam_kmeans_out;
/* sets, vocab_in [K][128] (16-byte aligned), vocab_defined [K] or NULL and the pointers of `out`: DEVICE pointers.  0 <= n_sets <=
 * 65535, 1 <= K <= 65536, n_sets * cap <= 2^32 - 1 (row ids and row counts fit 32 bits).  Asynchronous on the context stream, never waits on the
 * host: convergence is decided on the device, and the launches of the rounds after it return at once.  Scratch belongs to the
 * context: per row 12 bytes beside the word search's, per (set, word) 4 bytes, and 1 KiB per block of step 4, of which there are
 * at most n_sets * cap / 256 + K.  VSLAM_ERR_INVALID before any launch - and before the context is looked at - for a null struct
 * or vocabulary, a wrong struct_size, rounds outside 1 .. 64, reserved != 0, n_sets or K out of range, a set without desc, counts
 * or a capacity, row ids past 32 bits, a misaligned desc, vocab_in or vocab, an undersized buffer, vocab overlapping vocab_in other
 * than exactly; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for stream capture. */
int vslam_vocab_kmeans_dev(vslam_ctx* ctx, const vslam_desc_sets* sets, int n_sets, const float* vocab_in, const uint8_t* vocab_defined,
                           uint32_t K, const vslam_kmeans_params* params, const vslam_kmeans_out* out);
/* The same call over HOST arrays, synchronous (a convenience path: device buffers per call): desc [n_sets][cap][128], defined
 * [n_sets][cap] or NULL, counts [n_sets], vocab_in [K][128], vocab_defined [K] or NULL, and the pointers of `out`.  Errors as for
 * vslam_vocab_kmeans_dev (no alignment is asked of host arrays). */
int vslam_vocab_kmeans_host(vslam_ctx* ctx, const float* desc, const uint8_t* defined, const uint32_t* counts, uint32_t cap, int n_sets,
                            const float* vocab_in, const uint8_t* vocab_defined, uint32_t K, const vslam_kmeans_params* params,
                            const vslam_kmeans_out* out);

/* ---------------------------------------------------------------- loop verification
 * A loop candidate of the place recognition section is a bag-of-words coincidence until geometry confirms it.  Four calls take the
 * device-resident candidate list through the exact matcher and the RANSAC of the two-view section in one asynchronous pass: a table
 * of (query set, train set) pairs from the candidates (vslam_loop_pairs_dev), the matcher over that table (vslam_match_pairs_dev),
 * the points of the matched records gathered per pair (vslam_pair_points_dev) so that vslam_epipolar_dev and every stage after it
 * run on the pairs unchanged, and the verdict (vslam_loop_verdict_dev).  The table serves any pairing a caller writes itself:
 * keyframe against keyframe, frame j against j + 2.  Everything but the matcher's d2 is integer arithmetic and copies, so a CPU
 * restates every byte (tests/loopref.py); no output depends on scheduling, vslam_ctx_set_f32_fused or vslam_ctx_set_matrix_path.
 *
 *   Pair.  Slot p of a table names set pairs[p].query_set of `query` and set pairs[p].train_set of `train`.  It is EMPTY iff
 *     (uint32)query_set >= n_query_sets or (uint32)train_set >= n_train_sets (so {-1, -1} is empty against any sets).  Nothing is
 *     read through an empty pair.  The two sides may be one buffer, a pair may name one set on both sides, and a set may appear in
 *     any number of slots on either side.
 *   Table from candidates.  candidates [nq][c] and cand_counts [nq] are vslam_place_dev's outputs for c = max_candidates; the query
 *     sets are the nq query frames, the train sets the nd database frames.  Slot i * c + r is {i, candidates[i][r].frame - db_first}
 *     iff r < min(cand_counts[i], c) and the difference, formed in int64, lies in 0 .. nd - 1; otherwise it is {-1, -1}.  A slot
 *     past the count is not read.  Every one of the nq * c slots is written.
 *   Match.  Pair p searches the rows of query set pairs[p].query_set among the rows of train set pairs[p].train_set: d2, the
 *     selection, the skipped rows and ACCEPTED are the descriptor matching section's.  nn, matches and match_counts are indexed by
 *     p exactly as vslam_match_dev indexes them by its pair.  An empty pair: match_counts[p] = 0, its nn and matches rows are left
 *     untouched.
 *   Gather.  For pair p that is not empty, with qs / ts its sets, and record i < min(match_counts[p], match_cap), m = matches[p][i]:
 *       query_points_out[p][i] = query_points[qs][m.query]   if (uint32)m.query < query_cap, else 24 bytes of 0xff
 *       train_points_out[p][i] = train_points[ts][m.train]   if (uint32)m.train < train_cap, else 24 bytes of 0xff
 *       local[p][i]            = {i, i, m.dist2}
 *     (the all-ones record has octave -1: the two-view section does not trust it).  Rows past the count and the rows of an empty
 *     pair are left untouched.  Record i of `local` is record i of `matches`, and vslam_epipolar_dev(local, match_counts, match_cap,
 *     query_points_out, match_cap, train_points_out, match_cap, n_pairs, ..) sees, record for record, the coordinates and the trust
 *     that the pair's own lists give - so model, inlier bits and counts are those of the pair at index p of a batched call.
 *   Verdict.  models [nq * c] are the models of the slots, n_train_sets the nd of the table.  Slot p = i * c + r is VERIFIED iff it
 *     is not empty against (nq, n_train_sets), models[p].best >= 0, models[p].n_inliers >= min_inliers and
 *     (uint64)n_inliers * den >= (uint64)num * n_matches.  The loop of query frame i is its verified slot with the most inliers,
 *     equal counts: the lower r.  loops[i] = {pairs[p].query_set, pairs[p].train_set, p, n_matches, n_inliers} of that slot, or
 *     {i, -1, -1, 0, 0} for a frame without one.  loop_list holds the frames i that have a loop, ascending, in its first n_loops
 *     entries; the entries after them are left untouched. */
typedef struct {
    int32_t query_set, train_set;
} vslam_set_pair;           /* 8 bytes */
typedef struct {
    uint32_t min_inliers;   /* >= 1 */
    uint32_t num, den;      /* den > 0 */
    uint32_t reserved;      /* 0 */
} vslam_loop_params;        /* 16 bytes */
typedef struct {
    int32_t query_set, train_set, slot; /* slot = -1 and train_set = -1: no loop */
    uint32_t n_matches, n_inliers;
} vslam_loop;               /* 20 bytes */
typedef struct {
    size_t struct_size;     /* = sizeof(vslam_loop_out) */
    vslam_loop* loops;      /* [nq] optional */
    size_t loops_bytes;
    int32_t* loop_list;     /* [nq] optional, needs n_loops */
    size_t loop_list_bytes;
    uint32_t* n_loops;      /* [1] optional */
    size_t n_loops_bytes;
} vslam_loop_out;
/* DEVICE pointers.  nq <= 65535, 1 <= c <= 8, nd <= 65535; pairs [nq * c] is written whole (nq == 0 does nothing).  Asynchronous
 * on the context stream, never waits on the host.  VSLAM_ERR_INVALID before any launch - and before the context is looked at - for
 * a null pointer, nq, c or nd out of range, an undersized pairs buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not
 * for stream capture. */
int vslam_loop_pairs_dev(vslam_ctx* ctx, const vslam_place_cand* candidates, const uint32_t* cand_counts, uint32_t nq, uint32_t c,
                         uint32_t db_first, uint32_t nd, vslam_set_pair* pairs, size_t pairs_bytes);
/* query (n_query_sets sets), train (n_train_sets sets), pairs [n_pairs] and the pointers of `out` ([n_pairs] rows each): DEVICE
 * pointers.  0 <= n_pairs <= 65535 (0 does nothing), 0 <= n_query_sets, n_train_sets <= 65535.  The norms are computed once per set,
 * not once per pair.  Asynchronous on the context stream, never waits on the host (the counts and the table are read on the device,
 * the grids are sized from the capacities); scratch belongs to the context.  VSLAM_ERR_INVALID before any launch - and before the
 * context is looked at - for a null argument, a wrong struct_size, n_pairs or a set count out of range, a ratio2 that is not finite
 * or not positive, a set without desc, counts or a capacity, a misaligned desc, same_octave without points, no output at all, matches
 * without match_counts, an undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for stream capture. */
int vslam_match_pairs_dev(vslam_ctx* ctx, const vslam_desc_sets* query, int n_query_sets, const vslam_desc_sets* train, int n_train_sets,
                          const vslam_set_pair* pairs, int n_pairs, float ratio2, int same_octave, const vslam_match_out* out);
/* The same call over HOST arrays, synchronous (a convenience path: device buffers per call): the pointers of query and train
 * ([n][cap][128], [n][cap] or NULL, [n][cap] or NULL, [n]), pairs [n_pairs] and the pointers of `out` are host pointers.  The rows
 * the device call leaves untouched keep the caller's bytes.  Errors as for vslam_match_pairs_dev (no alignment is asked of host
 * arrays). */
int vslam_match_pairs_host(vslam_ctx* ctx, const vslam_desc_sets* query, int n_query_sets, const vslam_desc_sets* train, int n_train_sets,
                           const vslam_set_pair* pairs, int n_pairs, float ratio2, int same_octave, const vslam_match_out* out);
/* DEVICE pointers: matches [n_pairs][match_cap] and match_counts [n_pairs] as vslam_match_pairs_dev wrote them, pairs [n_pairs],
 * query_points [n_query_sets][query_cap], train_points [n_train_sets][train_cap]; the three outputs are [n_pairs][match_cap] each and
 * all required.  0 <= n_pairs <= 65535 (0 does nothing).  Asynchronous on the context stream, never waits on the host.
 * VSLAM_ERR_INVALID before any launch - and before the context is looked at - for a null pointer, n_pairs or a set count out of
 * range, match_cap / query_cap / train_cap == 0, an undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for
 * stream capture. */
int vslam_pair_points_dev(vslam_ctx* ctx, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                          const vslam_set_pair* pairs, int n_pairs, const vslam_point* query_points, uint32_t query_cap, int n_query_sets,
                          const vslam_point* train_points, uint32_t train_cap, int n_train_sets, vslam_point* query_points_out,
                          size_t query_points_out_bytes, vslam_point* train_points_out, size_t train_points_out_bytes, vslam_match* local,
                          size_t local_bytes);
/* DEVICE pointers: models [nq * c], pairs [nq * c].  nq <= 65535 (0: n_loops = 0, nothing else is written), 1 <= c <= 8,
 * n_train_sets <= 65535.  Asynchronous on the context stream, never waits on the host.  VSLAM_ERR_INVALID before any launch - and
 * before the context is looked at - for a null argument, a wrong struct_size, nq, c or n_train_sets out of range, min_inliers == 0,
 * den == 0, reserved != 0, no output at all, loop_list without n_loops, an undersized buffer; then VSLAM_ERR_HIP when there is no
 * usable HIP device.  Not for stream capture. */
int vslam_loop_verdict_dev(vslam_ctx* ctx, const vslam_epipolar* models, const vslam_set_pair* pairs, uint32_t nq, uint32_t c,
                           uint32_t n_train_sets, const vslam_loop_params* params, const vslam_loop_out* out);
/* The same call over HOST arrays, synchronous.  The loop_list entries the device call leaves untouched keep the caller's bytes.
 * Errors as for vslam_loop_verdict_dev. */
int vslam_loop_verdict_host(vslam_ctx* ctx, const vslam_epipolar* models, const vslam_set_pair* pairs, uint32_t nq, uint32_t c,
                            uint32_t n_train_sets, const vslam_loop_params* params, const vslam_loop_out* out);

/* ---------------------------------------------------------------- frame structure: the trajectory's output seen per frame
 * vslam_chain_dev keeps its cameras and world points per PAIR and per record; a loop names FRAMES.  This step gives each of the
 * n_frames = n_pairs + 1 frames of a chained run one camera and one table from feature index to world point, without copying a
 * point.  The inputs are what vslam_chain_dev read and wrote for n_pairs consecutive pairs: poses, matches, match_counts,
 * match_cap, front_bits, point_cap, and chain [n_pairs].  The LIVE rule is the trajectory section's, verbatim.  A CPU restates
 * every byte (tests/sim3ref.py): the arithmetic is the two product rules of the trajectory's step 4.
 *
 *   Source of frame f: pair f, query side (side 0), iff f < n_pairs and chain[f].valid != 0; else pair f - 1, train side (side 1),
 *     iff f >= 1 and chain[f - 1].valid != 0; else none.
 *   cams[f], query side:  W = chain[f].W, w = chain[f].w, segment = chain[f].segment, pair = f, side = 0, valid = 1  (copies).
 *   cams[f], train side, with (R, t, s) = (poses[f - 1].R, poses[f - 1].t, chain[f - 1].scale) and (W, w) of chain[f - 1]:
 *       W'[i][k] = (R[i][0]*W[0][k] + R[i][1]*W[1][k]) + R[i][2]*W[2][k];
 *       w'[i]    = ((R[i][0]*w0 + R[i][1]*w1) + R[i][2]*w2) + s*t_i;
 *     segment = chain[f - 1].segment, pair = f - 1, side = 1, valid = 1.  Every NaN is written as 0x7ff8000000000000.
 *   cams[f], no source:  all twelve doubles 0.0, segment = pair = -1, side = 0, valid = 0.
 *   index[f][k], k < point_cap: the LOWEST record i of the source pair that is live and whose query == k (query side) or
 *     train == k (train side); -1 where there is none, and -1 for every k of a frame without a source.  Every entry of index is
 *     written.  (An integer minimum: the same in any order.)  An entry is the record number as int32: with match_cap above 2^31 a
 *     record i >= 2^31 reads back negative, and the loop alignment section, which asks for 0 <= entry < map_cap, does not use it.
 * The world point of feature k of frame f is then map[cams[f].pair][index[f][k]] of vslam_chain_dev's `map` output. */
typedef struct {
    double W[9], w[3]; /* x_camera = W x_world + w, in the segment's world frame and unit */
    int32_t segment;   /* the pair the segment started at: two frames share a world frame iff their segments are equal; -1: none */
    int32_t pair;      /* the pair whose map rows hold this frame's points; -1: none */
    int32_t side;      /* 0: the pair's query frame, 1: its train frame */
    int32_t valid;
} vslam_frame_cam; /* 112 bytes */
typedef struct {
    size_t struct_size;    /* = sizeof(vslam_frame_world_out) */
    vslam_frame_cam* cams; /* [n_pairs + 1], required */
    size_t cams_bytes;
    int32_t* index;        /* [n_pairs + 1][point_cap], required */
    size_t index_bytes;
} vslam_frame_world_out;
/* DEVICE pointers, all required.  Asynchronous on the context stream, never waits on the host (the counts are read on the
 * device, the grids are sized from the capacities).  VSLAM_ERR_INVALID before any launch - and before the context is looked
 * at - for a null pointer, a wrong struct_size, n_pairs outside 0 .. 65535 (0 does nothing: without a pair there is no
 * trajectory), match_cap or point_cap == 0, an undersized buffer; then VSLAM_ERR_HIP when there is no usable HIP device.  Not for
 * stream capture. */
int vslam_frame_world_dev(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                          uint32_t match_cap, const uint64_t* front_bits, uint32_t point_cap, const vslam_chain* chain, int n_pairs,
                          const vslam_frame_world_out* out);
/* The same call over HOST arrays, synchronous (a convenience path: device buffers per call).  Errors as for vslam_frame_world_dev. */
int vslam_frame_world_host(vslam_ctx* ctx, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts,
                           uint32_t match_cap, const uint64_t* front_bits, uint32_t point_cap, const vslam_chain* chain, int n_pairs,
                           const vslam_frame_world_out* out);

/* ---------------------------------------------------------------- loop alignment: RANSAC Sim(3) between the two ends of a loop
 * The two ends of a verified loop lie in world frames that have drifted apart, or in two segments with a world frame and a unit
 * of their own.  This step estimates, per slot of a set-pair table, the similarity (s, R, t) that maps the 3-D structure seen
 * from the query frame onto the structure seen from the train frame:  y_train_world = s R x_query_world + t  - the edge a pose
 * graph needs, and the quantity that re-links two segments.  A RANSAC over 3-point samples (Horn's closed form with the symmetric
 * scale), scored by reprojection into both cameras; a fixed number of hypotheses, no adaptive stop, no refit over the inliers.
 * Slot p names query frame qs = pairs[p].query_set of `query` and train frame ts = pairs[p].train_set of `train`; the EMPTY rule
 * is the loop verification section's, against (query->n_frames, train->n_frames).  Nothing is read through an empty slot.
 *   A side is one vslam_sim3_side: cams and index as vslam_frame_world_dev wrote them, map as vslam_chain_dev wrote it
 *   ([n_map_pairs][map_cap][3]), and points [n_frames][points_cap], the vslam_point lists of the frames.  Both sides may be the
 *   same buffers, a slot may name one frame on both sides, and a frame may appear in any number of slots.
 *   matches [n_pairs][match_cap] and match_counts [n_pairs] are vslam_match_pairs_dev's, with real feature indices;
 *   m_p = min(match_counts[p], match_cap), 0 for an empty slot.  select_bits [n_pairs][(match_cap + 63) / 64], optional: record b
 *   is SELECTED iff there are no select_bits or bit b % 64 of word b / 64 of the slot is set (the inlier_bits vslam_epipolar_dev
 *   wrote over vslam_pair_points_dev's `local` list are exactly that).
 * The arithmetic is fixed here so that a CPU can restate it bit for bit (tests/sim3ref.py): IEEE f64, every + - * / sqrt rounded
 * on its own (no fused multiply-add), sums left to right as written, matrices row-major.  mix() is the two-view section's.
 *
 *  1. Correspondence of record b < m_p, (query, train) its indices as unsigned.  A camera cams[f] is TRUSTED iff valid != 0 and
 *     (uint32)pair < n_map_pairs of its side.  link_q = index_q[qs][query] iff query < min(point_cap, points_cap) of the query
 *     side, else -1; link_t likewise from train and the train side.  The record is USABLE iff it is selected, both cameras are
 *     trusted, 0 <= link_q < map_cap of the query side and 0 <= link_t < map_cap of the train side, the octaves of
 *     points_q[qs][query] and points_t[ts][train] are in 0 .. 31, and all six coordinates of X = map_q[cams_q[qs].pair][link_q]
 *     and Y = map_t[cams_t[ts].pair][link_t] are finite.  With (x, y) the exact coordinate of a point (two-view section):
 *       uq = (x_q - cx)/fx;  vq = (y_q - cy)/fy;  ut = (x_t - cx)/fx;  vt = (y_t - cy)/fy.
 *     The usable records, in list order, are the slot's dense list of n_corr correspondences {X, Y, uq, vq, ut, vt, b}.
 *  2. Sample.  Step 3 of the resection section with 3 kept indices: base = mix(mix(seed + p) + h); draw d = 0, 1, ... gives
 *     r = mix(base + d) and the index (uint64(r) * n_corr) >> 32, kept if it is not among the indices kept so far; the sample is
 *     the first 3 kept, in that order.  Fewer than 3 after 64 draws: invalid.  n_corr < 3: every hypothesis is invalid.
 *  3. Model from the 3 correspondences (Xi, Yi):
 *       cX_k = ((X0_k + X1_k) + X2_k) / 3, cY_k likewise;   A_i = Xi - cX,  B_i = Yi - cY   (componentwise);
 *       |A_i|^2 = (A_i0*A_i0 + A_i1*A_i1) + A_i2*A_i2;   a2 = (|A_0|^2 + |A_1|^2) + |A_2|^2,  b2 likewise from B;
 *       a2 or b2 zero or not finite: invalid;   s = sqrt(b2 / a2);   si = 1 / s;
 *       M[r][c] = (B_0r*A_0c + B_1r*A_1c) + B_2r*A_2c.
 *     R is step 5 of the resection section applied to this M, verbatim up to and including R[i][j] (the rules for n1 and n2
 *     stay; there is no lambda): the two leading eigen-directions of M^T M, so the rank-2 M of a 3-point sample is its normal
 *     case, and R is a proper rotation whatever the sign of det(M).
 *       t_i = cY_i - s * ((R[i][0]*cX_0 + R[i][1]*cX_1) + R[i][2]*cX_2).
 *     Any of s, si, the nine R, the three t not finite: invalid.  An invalid hypothesis has s = R = t = 0 and no inliers.
 *  4. Composition, once per hypothesis, with (Wq, wq) = cams_q[qs] and (Wt, wt) = cams_t[ts]:
 *       P[i][k] = (Wt[i][0]*R[0][k] + Wt[i][1]*R[1][k]) + Wt[i][2]*R[2][k];     Af[i][k] = s * P[i][k];
 *       af_i = ((Wt[i][0]*t_0 + Wt[i][1]*t_1) + Wt[i][2]*t_2) + wt_i;
 *       Q[i][k] = (Wq[i][0]*R[k][0] + Wq[i][1]*R[k][1]) + Wq[i][2]*R[k][2];     Ab[i][k] = si * Q[i][k]   (si = 1 / s);
 *       ab_i = wq_i - ((Ab[i][0]*t_0 + Ab[i][1]*t_1) + Ab[i][2]*t_2).
 *     (Af, af) takes a query-world point into the train camera, (Ab, ab) a train-world point into the query camera.
 *  5. Inlier test.  A correspondence is an inlier iff step 6 of the resection section holds both ways: under (R, t) = (Af, af)
 *     for the point X against (u, v) = (ut, vt), and under (Ab, ab) for the point Y against (uq, vq).
 *  6. Selection: the valid hypothesis with the most inliers, the lowest h on ties.  Counts are integers, so the result does not
 *     depend on how the correspondences are split over lanes and workgroups.
 * Every double of a model or a hypothesis is finite or 0.0; every double of a correspondence is finite.
 *
 * Scratch (the context's): 24 bytes per record of capacity (n_pairs * match_cap), 88 more without a correspondences buffer,
 * and n_pairs * n_hypotheses * 112 bytes without a hypotheses buffer; an allocation that fails is VSLAM_ERR_NOMEM. */
typedef struct {
    const vslam_frame_cam* cams; /* [n_frames] */
    const int32_t* index;        /* [n_frames][point_cap] */
    const double* map;           /* [n_map_pairs][map_cap][3]: vslam_chain_dev's map */
    const vslam_point* points;   /* [n_frames][points_cap] */
    uint32_t map_cap;            /* the match capacity of the chained pairs */
    uint32_t point_cap;          /* the row pitch of index */
    uint32_t points_cap;
    uint32_t n_map_pairs;        /* 1 .. 65535: the rows of map */
    int32_t n_frames;            /* 0 .. 65536 */
    int32_t reserved;            /* 0 */
} vslam_sim3_side;               /* 56 bytes */
typedef struct {
    uint32_t n_hypotheses; /* 1 .. 65535 */
    uint32_t seed;
    double max_dist2;      /* squared reprojection error in pixels^2, finite and positive */
    vslam_pose_params K;   /* all finite, fx and fy positive */
} vslam_sim3_params;
typedef struct {
    double s;         /* 0 when not valid, like R and t */
    double R[9];
    double t[3];
    uint32_t inliers;
    int32_t valid;
} vslam_sim3_hyp; /* 112 bytes */
typedef struct {
    double X[3];       /* the query frame's world point */
    double Y[3];       /* the train frame's world point */
    double uq, vq;     /* the calibrated observation in the query frame */
    double ut, vt;     /* ... in the train frame */
    uint32_t b;        /* the match record it came from */
    uint32_t reserved; /* 0 */
} vslam_sim3_corr; /* 88 bytes */
typedef struct {
    double s;              /* the winner; s, R and t all zero when best < 0 */
    double R[9];
    double t[3];
    uint32_t n_matches;    /* m_p */
    uint32_t n_corr;       /* usable correspondences */
    uint32_t n_inliers;    /* the winner's count, 0 when best < 0 */
    int32_t best;          /* winning hypothesis, -1: none (always for an empty slot) */
    uint32_t n_valid;      /* hypotheses that produced a model */
    int32_t query_segment; /* cams_q[qs].segment and cams_t[ts].segment, copied; -1 both for an empty slot */
    int32_t train_segment;
    uint32_t reserved;     /* 0 */
} vslam_sim3;              /* 136 bytes */
typedef struct {
    size_t struct_size;      /* = sizeof(vslam_sim3_out) */
    vslam_sim3* models;      /* [n_pairs], required */
    size_t models_bytes;
    uint64_t* inlier_bits;   /* [n_pairs][(match_cap + 63) / 64] optional: bit b % 64 of word b / 64 = record b is usable and an
                              * inlier of the winner; the first (m_p + 63) / 64 words of a slot are written (all zero when
                              * best < 0), the rest untouched */
    size_t inlier_bits_bytes;
    vslam_sim3_hyp* hypotheses; /* [n_pairs][n_hypotheses] optional: every hypothesis with its count */
    size_t hypotheses_bytes;
    vslam_sim3_corr* correspondences; /* [n_pairs][match_cap] optional: the first n_corr rows of a slot are written */
    size_t correspondences_bytes;
    int32_t* links;          /* [n_pairs][match_cap][2] optional: for b < m_p {link_q, link_t} of step 1; the rest untouched */
    size_t links_bytes;
} vslam_sim3_out;
/* query, train, params and out are HOST structs whose pointers, like pairs, matches, match_counts and select_bits, are DEVICE
 * pointers; all but select_bits and the optional outputs are required.  Asynchronous on the context stream, never waits on the
 * host (the counts and the tables are read on the device, the grids are sized from the capacities); scratch belongs to the
 * context.  VSLAM_ERR_INVALID before any launch - and before the context is looked at - for a null argument, a wrong
 * struct_size, n_pairs outside 0 .. 65535 (0 does nothing), n_hypotheses outside 1 .. 65535, a max_dist2 that is not finite or not
 * positive, an intrinsic that is not finite, fx or fy not positive, a side with a null pointer, a zero capacity, n_frames outside
 * 0 .. 65536, n_map_pairs outside 1 .. 65535 or reserved != 0, match_cap == 0, an undersized buffer; then VSLAM_ERR_HIP when
 * there is no usable HIP device.  Not for stream capture. */
int vslam_sim3_dev(vslam_ctx* ctx, const vslam_sim3_side* query, const vslam_sim3_side* train, const vslam_set_pair* pairs,
                   const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap, const uint64_t* select_bits,
                   int n_pairs, const vslam_sim3_params* params, const vslam_sim3_out* out);
/* The same call over HOST arrays, synchronous (a convenience path: device buffers per call): the pointers of query and train are
 * host arrays of the sizes above (a side given twice - query == train, or two equal structs - goes up once).  The rows the device
 * call leaves untouched keep the caller's bytes.  Errors as for vslam_sim3_dev. */
int vslam_sim3_host(vslam_ctx* ctx, const vslam_sim3_side* query, const vslam_sim3_side* train, const vslam_set_pair* pairs,
                    const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap, const uint64_t* select_bits,
                    int n_pairs, const vslam_sim3_params* params, const vslam_sim3_out* out);

/* Timing hook for bench.py: when enabled, the context brackets every launch of the
 * named kernel with HIP events on the stream the launch goes to (the context's stream or one of the
 * batched path's side streams); vslam_kernel_timing_read synchronises and returns launches and total
 * milliseconds since the last reset.  "name@N" restricts the hook to the launches of octave N
 * ("k_pyr_octave@0", "k_gauss_h_strip@3", "k_extrema_w3@1"); NULL or "" switches it off. */
int vslam_kernel_timing_enable(vslam_ctx* ctx, const char* kernel_name);
int vslam_kernel_timing_read(vslam_ctx* ctx, int* launches, double* total_ms);
/* Names of the kernels a batch launches, '\n'-separated (for profiles and the hook). */
const char* vslam_kernel_names(void);

#ifdef __cplusplus
}
#endif
#endif
