// C++17 mirror of the reference's detector API for the hot path, implemented over the C ABI
// of include/vslam.h (hand-written HIP kernels; no CPU compute here).  Same names, argument
// meaning and return types as the reference's free functions / class, so its callers compile
// against this header unchanged (paths relative to /root/reference/KeyPointDetection/):
//
//   Mat HarrisCorner(Mat& Ix, Mat& Iy)                         Harris_corners.cpp:31
//   Mat NonMaximumSuppression(Mat& response, int windowSize)   Harris_corners.cpp:70
//   Mat NMS2(Mat& response, int windowSize)                    Harris_corners.cpp:83
//   class GaussPyramid                                         include/src/GaussPyramid/GaussPyramid.hpp:14
//   struct SLAM::point                                         Diff_of_Gauss.cpp:27
//   void initialKeypointDetection(std::vector<SLAM::point>&, GaussPyramid&, int, int)
//   bool FeaturePointLocalization(std::vector<Mat>&, std::vector<SLAM::point>&, int, SLAM::point&)
//   float computeEdgeResponse(const SLAM::point&, const Mat&, const Mat&)
//   void filterKeypoints(GaussPyramid&, int, std::vector<SLAM::point>&, std::vector<SLAM::point>&)
//                                                              Diff_of_Gauss.cpp:254
//   void SIFT(std::vector<SLAM::point>&, std::vector<std::vector<float>>&, GaussPyramid&, int)
//                                                              Diff_of_Gauss.cpp:561
//   class SLAM::Rotation (the members the descriptor stage uses)   include/src/Rotation/rotation.h:11
// plus the OpenCV calls on the path (vslamcv::GaussianBlur / Sobel / convertScaleAbs / resize).
// StructureMatrix (:10) is also provided as a per-pixel call; HarrisCorner itself runs the whole
// image in one kernel.  Errors of the C ABI surface as vslam::Error (the reference relies on cv::Exception).
// The per-level gradient getters (octaveGradX/Y/Mag/Orient, processGradients, SURVEY.md section 8f
// row 1) are computed on the GPU on first access instead of in the constructor.
#pragma once
#include <cmath>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "cvlite.hpp"

namespace vslam {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& what) : std::runtime_error(what), status(s) {}
};

// One process-wide context per device (the reference is single-threaded: SURVEY 8b).
vslam_ctx* default_context(int device = 0);
void check(int status, vslam_ctx* ctx, const char* what);

}  // namespace vslam

namespace SLAM {
struct point {  // Diff_of_Gauss.cpp:27-35
    point(int row_, int col_, int value_, int padding_, int octave_, int level_)
        : row(row_), col(col_), value(value_), padding(padding_), octave(octave_), level(level_) {}
    point() = default;
    int row = 0, col = 0, value = 0, padding = 0, octave = 0, level = 0;
};
static_assert(sizeof(point) == sizeof(vslam_point), "SLAM::point must stay six ints");
}  // namespace SLAM

namespace SLAM {
// include/src/Rotation/rotation.h:8-24: the members on the descriptor path (SIFT -> getRotatedWindowPoints
// -> rotate_pt_CW -> cos_sin_of_angle).  Host arithmetic, identical to the C ABI's
// vslam_cos_sin_deg / vslam_rotated_window_points.
class Transform {};
class Rotation : public Transform {
public:
    static float convertToRadians(float theta);
    static const cv::Point2f cos_sin_of_angle(float theta, bool degrees = true);
    static cv::Point2i rotate_pt_CW(const cv::Point2i& pt, const cv::Point2i& center, const cv::Point2f& angles);
    static cv::Point2i rotate_pt_CW(const cv::Point2i& pt, const cv::Point2i& center, float theta, bool degrees = true);
    static std::vector<cv::Point2i> getRotatedWindowPoints(cv::Mat& I, const cv::Point2i& center, int windowSize, float theta,
                                                           bool degrees = true);
};
}  // namespace SLAM

namespace vslamcv {  // the OpenCV call sites of the hot path
enum { BORDER_DEFAULT = 4, INTER_NEAREST = 0, INTER_LINEAR = 1 };
void GaussianBlur(const cv::Mat& src, cv::Mat& dst, cv::Size ksize, double sigmaX, double sigmaY = 0,
                  int borderType = BORDER_DEFAULT);
void Sobel(const cv::Mat& src, cv::Mat& dst, int ddepth, int dx, int dy, int ksize = 1, double scale = 1,
           double delta = 0, int borderType = BORDER_DEFAULT);
void convertScaleAbs(const cv::Mat& src, cv::Mat& dst);
void resize(const cv::Mat& src, cv::Mat& dst, cv::Size dsize, double fx, double fy, int interpolation);
}  // namespace vslamcv

// void StructureMatrix(Mat& M, Mat& Ix, Mat& Iy, int padding, int i, int j), Harris_corners.cpp:10-29:
// gathers the (2*padding+1)^2 window on the host, sums on the GPU (vslam_structure_matrix_windows).
// HarrisCorner does not call it per pixel - it runs the whole image in one kernel.
void StructureMatrix(cv::Mat& M, cv::Mat& Ix, cv::Mat& Iy, int padding, int i, int j);
cv::Mat HarrisCorner(cv::Mat& Ix, cv::Mat& Iy);
cv::Mat NonMaximumSuppression(cv::Mat& response, int windowSize);
cv::Mat NMS2(cv::Mat& response, int windowSize);
// Whole Harris front end on the 8-bit frame in one fused kernel (Harris_corners.cpp:158-182).
std::vector<vslam_kp> HarrisKeypoints(const cv::Mat& gray, float k = 0.04f);

class GaussPyramid {
public:
    GaussPyramid(cv::Mat& img, int numOctaves, double sigma);
    GaussPyramid(cv::Mat& img, double sigma);
    ~GaussPyramid();
    GaussPyramid(const GaussPyramid&) = delete;
    GaussPyramid& operator=(const GaussPyramid&) = delete;
    int getNumOctaves() const { return info_.n_octaves; }
    int getNumLevels() const { return info_.n_levels; }
    int getNumScaleSamples() const { return info_.n_levels - 3; }
    double getSigmaAt(int octave, int level) const;
    double calculateSigma(int octave, int level) const;
    const cv::Mat& octaveImage(int octave);
    const std::vector<double>& octaveSigma(int octave);
    const std::vector<cv::Mat>& octaveBlur(int octave);
    const std::vector<cv::Mat>& octaveDiff(int octave);
    // processGradients results (GaussPyramid.hpp:33-36), computed on the GPU on first access
    const std::vector<cv::Mat>& octaveGradX(int octave) { return grads(octave, 0); }
    const std::vector<cv::Mat>& octaveGradY(int octave) { return grads(octave, 1); }
    const std::vector<cv::Mat>& octaveGradMag(int octave) { return grads(octave, 2); }
    const std::vector<cv::Mat>& octaveGradOrient(int octave) { return grads(octave, 3); }
    const std::vector<cv::Mat>& imagePyramid();
    const std::map<int, std::vector<cv::Mat>>& pyramidGauss();
    const std::map<int, std::vector<cv::Mat>>& pyramidDiff();
    // GaussPyramid.hpp:41-44.  These materialise every level of every octave (96 bytes per pyramid
    // pixel, 1.06 GB for a 1080p frame) exactly as the reference's constructor does.
    const std::map<int, std::vector<cv::Mat>>& pyramidGradX() { return allGrads(0); }
    const std::map<int, std::vector<cv::Mat>>& pyramidGradY() { return allGrads(1); }
    const std::map<int, std::vector<cv::Mat>>& pyramidGradMag() { return allGrads(2); }
    const std::map<int, std::vector<cv::Mat>>& pyramidGradOrient() { return allGrads(3); }
    static std::vector<cv::Mat> padOctave(int padding, const std::vector<cv::Mat>& images);
    const vslam_pyramid* handle() const { return pyr_; }  // the HBM-resident pyramid
    // The reference runs processGradients INSIDE the constructor (GaussPyramid.cpp:118): every level's gradX / gradY /
    // magnitude / orientation exist when it returns.  Here they are formed on first access (same values through the same
    // getters; 96 bytes per pyramid pixel saved for callers that never ask).  A caller that wants the reference's timing -
    // all the work in the constructor, getters free - switches this on before constructing (or sets VSLAM_EAGER_GRADIENTS=1).
    static void setEagerGradients(bool on);
    static bool eagerGradients();

private:
    void build(cv::Mat& img, int numOctaves, double sigma);
    void checkOctave(int octave) const;
    vslam_pyramid* pyr_ = nullptr;
    vslam_pyramid_info info_{};
    // host copies are fetched lazily, one octave at a time (the stacks stay in HBM)
    std::vector<cv::Mat> img_pyramid_;
    std::map<int, std::vector<double>> sigmas_;
    std::map<int, std::vector<cv::Mat>> gauss_, diff_, grad_[4];
    const std::vector<cv::Mat>& grads(int octave, int kind);
    const std::map<int, std::vector<cv::Mat>>& allGrads(int kind);
};

// void initialKeypointDetection(...), Diff_of_Gauss.cpp:254-297, as the reference runs it: every
// lattice candidate goes through FeaturePointLocalization (:290) and the survivors are appended
// in the reference's loop order with the value rewritten at :246 (vslam_dog_keypoints).
void initialKeypointDetection(std::vector<SLAM::point>& keypoints, GaussPyramid& pyramid, int octave, int windowSize);
// The candidate stage alone (up to :287): candidates with DoG value >= minContrast (SURVEY 8a;
// 8 = the contrast test for the degenerate, exactly-singular cases).
void scaleSpaceCandidates(std::vector<SLAM::point>& candidates, GaussPyramid& pyramid, int octave, int windowSize,
                          int minContrast = 8);
// EXTENSION (no reference counterpart; SURVEY.md section 8a, note): the dense 3x3x3 scale-space test on
// every pixel of levels 1..3 - rule of :282-287, replicate border of :260, points in (level, row, col)
// order with padded coordinates like :289 (vslam_dog_extrema_dense).
void scaleSpaceExtremaDense(std::vector<SLAM::point>& candidates, GaussPyramid& pyramid, int octave, int minContrast = 8);
// bool FeaturePointLocalization(...), Diff_of_Gauss.cpp:223-251: reads the three finite
// differences from the padded DoG stack (:226-228) on the host, evaluates the contrast test on
// the GPU (vslam_localize_points), updates point.value and appends the point when kept.
bool FeaturePointLocalization(std::vector<cv::Mat>& dogs_padded, std::vector<SLAM::point>& keypoints, int level,
                              SLAM::point& point);
// float computeEdgeResponse(const SLAM::point&, const Mat& grad_x, const Mat& grad_y),
// Diff_of_Gauss.cpp:79-109: gathers the keypoint's window from the two CV_32F gradient images
// on the host (:93-94) and evaluates tr^2/det on the GPU (vslam_edge_response_windows).
float computeEdgeResponse(const SLAM::point& keypoint, const cv::Mat& grad_x, const cv::Mat& grad_y);
// void filterKeypoints(GaussPyramid&, int octave, vector<SLAM::point>& keypoints,
// vector<SLAM::point>& reducedKeypoints), Diff_of_Gauss.cpp:301-372 (vslam_filter_keypoints).
void filterKeypoints(GaussPyramid& pyramid, int octave, std::vector<SLAM::point>& keypoints,
                     std::vector<SLAM::point>& reducedKeypoints);
// void SIFT(vector<SLAM::point>& reducedKeypoints, vector<vector<float>>& featureDescriptors_vec,
// GaussPyramid&, int octave), Diff_of_Gauss.cpp:561-693 (vslam_sift_descriptors): appends one
// 128-float descriptor per oriented keypoint.  A keypoint whose rotated window leaves the padded level
// (the reference then reads foreign memory, :541) throws vslam::Error(VSLAM_ERR_RANGE) unless
// `defined` is given, in which case it receives one flag per keypoint and the descriptor is all zero.
void SIFT(std::vector<SLAM::point>& reducedKeypoints, std::vector<std::vector<float>>& featureDescriptors_vec,
          GaussPyramid& pyramid, int octave, std::vector<unsigned char>* defined = nullptr);
// featureDescriptors.dat exactly as Diff_of_Gauss.cpp:837-863 writes it (vslam_descriptor_file_write).
void writeFeatureDescriptors(const std::string& file_name, const std::vector<std::vector<float>>& featureDescriptors_vec);

// The step Diff_of_Gauss.cpp:687 leaves open ("final step is graphing and comparing two images with each other"): every
// query descriptor's nearest and second-nearest train descriptor and Lowe's ratio test, exact, on the GPU (vslam_match_host;
// the arithmetic is stated in include/vslam.h).  The two vectors are what SIFT() fills; `ratio` is squared once in f32.
// *_defined: the flags SIFT() returns (null = all defined; undefined rows neither match nor are matched).
namespace vslam {
struct Matches {
    std::vector<vslam_nn2> nn;         // one per query descriptor: {train index or -1, dist2, second_dist2}
    std::vector<vslam_match> matches;  // the accepted queries, ascending query order
    std::vector<vslam_rnn> rnn;        // matchMutual only - one per train descriptor: {query index or -1, dist2}
};
Matches matchDescriptors(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train, float ratio = 0.8f,
                         const std::vector<unsigned char>* query_defined = nullptr, const std::vector<unsigned char>* train_defined = nullptr);

// matchDescriptors with the cross-check of a brute-force matcher in the same pass, on the GPU (vslam_match_mutual_host;
// include/vslam.h, "mutual matching"): Matches::nn is matchDescriptors', Matches::rnn the nearest query descriptor of every train
// descriptor, and Matches::matches holds only the accepted queries whose train descriptor chose them back - no train index twice.
Matches matchMutual(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train, float ratio = 0.8f,
                    const std::vector<unsigned char>* query_defined = nullptr, const std::vector<unsigned char>* train_defined = nullptr);

// The step after matching (the reference's README, "3. 3D Reconstruction - Epipolar Geometry"): the fundamental matrix of the
// pair by RANSAC over the accepted matches, and their inlier subset, on the GPU (vslam_epipolar_host; sampling, the 8-point
// model and the Sampson test are stated in include/vslam.h).  `matches` is Matches::matches; the two point vectors are the
// oriented keypoints SIFT() described, all octaves of an image in the order of its descriptors.
struct Epipolar {
    vslam_epipolar model;              // F row-major with x_train^T F x_query = 0 in image pixels; best = -1: none
    std::vector<vslam_match> inliers;  // the matches the model accepts, list order kept
};
Epipolar fundamentalRansac(const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                           const std::vector<SLAM::point>& trainPoints, const vslam_epipolar_params& params = {512, 1, 4.0});

// Between the two: the least-squares refit of the model over all its inliers, the inliers classified again, for `rounds`
// rounds, on the GPU (vslam_refit_host; the ordered sums, the 9 x 9 Jacobi and the acceptance rule are stated in
// include/vslam.h).  `matches` is the FULL list fundamentalRansac read, not its inliers.  The result never has fewer inliers
// than `model`; feed Refit::model and Refit::inliers to relativePose.
struct Refit {
    vslam_epipolar model;              // `model` with the refitted F and its inlier count
    vslam_refit info;                  // inliers before and after, rounds kept, why it stopped
    std::vector<vslam_match> inliers;  // the matches the refitted model accepts, list order kept
};
Refit refitFundamental(const vslam_epipolar& model, const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                       const std::vector<SLAM::point>& trainPoints, const vslam_refit_params& params = {4, 4.0});

// Beside fundamentalRansac, over the same lists: the homography of the pair by RANSAC and - given the fundamental matrix - the
// verdict whether H explains the matches as well as F does (a plane, a pure rotation, a pure translation of the image), on the
// GPU (vslam_homography_host; the 4-point DLT, the transfer test and the integer verdict are stated in include/vslam.h).
// Feed Homography::gated to refitFundamental / relativePose in place of the model: a degenerate pair is "no model" there.
struct Homography {
    vslam_homography model;            // H row-major with x_train ~ H x_query, G the way back; best = -1: none; the verdict
    vslam_epipolar gated;              // *epipolarModel, made "no model" when the pair is degenerate; all zero without one
    std::vector<vslam_match> inliers;  // the matches H accepts, list order kept
};
Homography findHomography(const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                          const std::vector<SLAM::point>& trainPoints, const vslam_epipolar* epipolarModel = nullptr,
                          const vslam_homography_params& params = {512, 1, 4.0, 1, 2, 16});

// After findHomography: the least-squares refit of H over all its inliers, the inliers classified again, for params.rounds
// rounds, on the GPU (vslam_hrefit_host; the 24 ordered sums, the 9 x 9 Jacobi, the signs and the acceptance rule are stated in
// include/vslam.h, "homography: least-squares refit over the inliers").  The result never has fewer inliers than `model`.
// With `epipolarModel` the verdict is computed again from the new inlier count and `gated` is the gate under it; feed
// HomographyRefit::model to matchGuidedHF / poseFromHomography and HomographyRefit::gated to refitFundamental / relativePose.
struct HomographyRefit {
    vslam_homography model;            // `model` with the refitted H, G, their inlier count and - with epipolarModel - the new verdict
    vslam_hrefit info;                 // inliers before and after, rounds kept, why it stopped
    vslam_epipolar gated;              // *epipolarModel, made "no model" when the pair is degenerate; all zero without one
    std::vector<vslam_match> inliers;  // the matches the refitted model accepts, list order kept
};
HomographyRefit refitHomography(const vslam_homography& model, const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                                const std::vector<SLAM::point>& trainPoints, const vslam_hrefit_params& params = {4, 4.0, 1, 2, 16},
                                const vslam_epipolar* epipolarModel = nullptr);

// A second matching pass once the pair has a model: matchDescriptors restricted, per query descriptor, to the train descriptors
// whose keypoint lies in the query keypoint's epipolar band under model.F, on the GPU (vslam_match_guided_host; the band, the
// selection and the acceptance with its absolute bound are stated in include/vslam.h, "guided matching").  On repeated structure
// it recovers the matches the global ratio test rejects; feed Matches::matches to fundamentalRansac / refitFundamental again.
// `model`: Epipolar::model, Refit::model or Homography::gated.  One keypoint per descriptor on both sides.
Matches matchGuided(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train,
                    const std::vector<SLAM::point>& queryPoints, const std::vector<SLAM::point>& trainPoints, const vslam_epipolar& model,
                    const vslam_guided_params& params = {0.64f, HUGE_VALF, 4.0, 0, 0}, const std::vector<unsigned char>* query_defined = nullptr,
                    const std::vector<unsigned char>* train_defined = nullptr);

// The same pass under the model that applies to the pair: the epipolar band where `epipolarModel` has an F, a window of
// params.max_transfer2 around H x where only `homographyModel` has an H - the degenerate pair, for which Homography::gated is "no
// model" and matchGuided finds nothing -, nothing where neither has (vslam_match_guided_hf_host; include/vslam.h, "guided matching
// under H or F").  Either record may be null, not both; the intended ones are &Homography::gated and &Homography::model.
Matches matchGuidedHF(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train,
                      const std::vector<SLAM::point>& queryPoints, const std::vector<SLAM::point>& trainPoints, const vslam_epipolar* epipolarModel,
                      const vslam_homography* homographyModel, const vslam_guided_hf_params& params = {0.64f, HUGE_VALF, 4.0, 4.0, 0, 0},
                      const std::vector<unsigned char>* query_defined = nullptr, const std::vector<unsigned char>* train_defined = nullptr);

// The step after that: the camera motion of the pair (x_train ~ R x_query + t, |t| = 1) and the 3-D point of every record of
// `matches` - the intended list is Epipolar::inliers - from the model fundamentalRansac found, on the GPU (vslam_pose_host;
// the decomposition, the cheirality vote and the triangulation are stated in include/vslam.h).  One pinhole camera
// {fx, fy, cx, cy} for both frames.
struct Pose {
    vslam_pose pose;                 // R row-major, t, the winner's count; best = -1: none
    vslam_pose_cand candidates[4];   // the four (R, t) with their counts
    std::vector<double> points;      // [matches][3], query-camera frame; empty when best < 0
    std::vector<uint64_t> frontBits; // bit i % 64 of word i / 64: record i is in front of both cameras under the winner
};
Pose relativePose(const vslam_epipolar& model, const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                  const std::vector<SLAM::point>& trainPoints, const vslam_pose_params& camera);

// The pose of a pair the gate took away from relativePose: the homography findHomography found, decomposed into (R, t, n), on
// the GPU (vslam_hpose_host, one pair; the candidates, the vote, the ambiguity rule and the prior are stated in include/vslam.h,
// "pose from homography").  `pose` is what relativePose gave for Homography::gated over the same `matches`: when the pair is
// selected (model.best >= 0, and model.degenerate with params.only_degenerate) its record, points and front bits are replaced
// - points empty when the new record has best < 0 -, otherwise it is left exactly as it was.  prior: a pose whose R resolves an
// ambiguous pair, e.g. the pair before; may be null.  The default min_spread and ratio are the tools' (DESIGN 5.24).
struct HomographyPose {
    vslam_hpose info;                // kind, the vote, the plane's normal and baseline over distance; all zero: not selected
    vslam_hpose_cand candidates[4];  // the four (R, t, n) with their counts
};
HomographyPose poseFromHomography(const vslam_homography& model, const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                                  const std::vector<SLAM::point>& trainPoints, const vslam_pose_params& camera, Pose& pose,
                                  const vslam_pose* prior = nullptr, double maxDist2 = 4.0, double minSpread = 0.0288, uint32_t ambiguousNum = 9,
                                  uint32_t ambiguousDen = 10, bool onlyDegenerate = true);

// The step after that over a sequence: the poses and points of consecutive pairs (pair j: frames j and j + 1) chained with the
// recovered scale into one world frame per segment, on the GPU (vslam_chain_host; the link, the median ratio, the walk and the
// map are stated in include/vslam.h).  The inputs are what relativePose gave for every pair, laid side by side at one
// capacity: matches [pairs][matchCap], matchCounts [pairs], points [pairs][matchCap][3], frontBits [pairs][(matchCap + 63) / 64];
// pointCap is the capacity of the frames' point lists.
struct Trajectory {
    std::vector<vslam_chain> chain;  // [pairs]: W, w (x_camera = W x_world + w), the camera centres, scale, segment
    std::vector<double> map;         // [pairs][matchCap][3], world coordinates; NaN: the record is not live; 0: past the count
    std::vector<int32_t> links;      // [pairs][matchCap]: the linked record of the pair before, or -1
    std::vector<double> ratios;      // [pairs][matchCap]: the distance ratio of a linked record, NaN otherwise
};
Trajectory chainPoses(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                      uint32_t matchCap, const std::vector<double>& points, const std::vector<uint64_t>& frontBits, uint32_t pointCap,
                      const vslam_chain_params& params = {16});

// The step after the chain: the records of consecutive pairs that saw one scene point linked into tracks, and every track's
// point triangulated from all of its views, on the GPU (vslam_tracks_host; the continuation rule, the normal equations, the
// cofactor solve and the reprojection test are stated in include/vslam.h).  The inputs are what chainPoses took, minus the
// points, the chain records it gave, and the frames' point lists framePoints [pairs + 1][pointCap].
struct Tracks {
    std::vector<vslam_track> tracks;          // [pairs][matchCap]: at the head's slot; NaN and 0 for a record that is not a head; 0: past the count
    std::vector<vslam_track_ref> refs;        // [pairs][matchCap]: the track a record lies on; all ones: not live, or past the count
    std::vector<uint64_t> goodBits;           // [pairs][(matchCap + 63) / 64]: the heads of good tracks
    std::vector<vslam_track_summary> summary; // [pairs]
};
Tracks buildTracks(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                   uint32_t matchCap, const std::vector<uint64_t>& frontBits, uint32_t pointCap, const std::vector<vslam_chain>& chain,
                   const std::vector<SLAM::point>& framePoints, const vslam_tracks_params& params);

// After buildTracks: cameras and track points moved together by an alternating bundle adjustment, on the GPU (vslam_bundle_host;
// the views, the point step, the camera rows, the sweeps and the outputs are stated in include/vslam.h).  The inputs are what
// buildTracks took and the tracks and refs it gave; camsIn is empty (the cameras start from the chain) or one record per pair.
struct Bundle {
    std::vector<vslam_track> tracks;           // [pairs][matchCap]: the input rows, the heads of active tracks refined
    std::vector<vslam_bundle_cam> cams;        // [pairs]: the train cameras, their centres, counters and costs
    std::vector<vslam_bundle_point> pointInfo; // [pairs][matchCap]: at the head slots of active tracks; 0 elsewhere
    std::vector<uint64_t> memberBits;          // [pairs][2][(matchCap + 63) / 64]: the member views by record, query side then train side
};
Bundle bundleAdjust(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                    uint32_t matchCap, const std::vector<uint64_t>& frontBits, uint32_t pointCap, const std::vector<vslam_chain>& chain,
                    const std::vector<SLAM::point>& framePoints, const std::vector<vslam_track>& tracksIn, const std::vector<vslam_track_ref>& refs,
                    const std::vector<vslam_bundle_cam>& camsIn, const vslam_bundle_params& params);

// Beside the chain: the camera of frame j + 1 relative to frame j resected against the points pair j - 1 triangulated, on the
// GPU (vslam_resect_host; the link, the calibrated 6-point DLT, the reprojection test and the selection are stated in
// include/vslam.h).  The structure side is what chainPoses takes; the observation side is any match list of the pairs -
// obsMatches [pairs][obsCap] with obsCounts, the same lists or the raw matches - and the train frames' points, trainPoints
// [pairs][trainCap].  t comes out in pair j - 1's unit; pair 0 has no model.
struct Resection {
    std::vector<vslam_resect> models;              // [pairs]: R, t, the counts; best = -1: none
    std::vector<uint64_t> inlierBits;              // [pairs][(obsCap + 63) / 64]: observation record b is an inlier of the winner
    std::vector<vslam_resect_corr> correspondences; // [pairs][obsCap]: the first n_corr rows of a pair hold {Y, u, v, b}; 0: past them
    std::vector<int32_t> links;                    // [pairs][obsCap]: the linked record of the pair before, or -1
};
Resection resectPoses(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                      uint32_t matchCap, const std::vector<double>& points, const std::vector<uint64_t>& frontBits, uint32_t pointCap,
                      const std::vector<vslam_match>& obsMatches, const std::vector<uint32_t>& obsCounts, uint32_t obsCap,
                      const std::vector<SLAM::point>& trainPoints, uint32_t trainCap, const vslam_resect_params& params);

// After resectPoses: every pair's pose refined by Gauss-Newton over all its inliers, on the GPU (vslam_resect_refine_host; the
// residual, the Jacobian, the ordered sums, the elimination, the Cayley update and the acceptance rule are stated in
// include/vslam.h).  models and correspondences are Resection's; the result never has fewer inliers than its input.
struct RefinedResection {
    std::vector<vslam_resect> models;       // [pairs]: R, t and n_inliers of the refined pose, the other fields copied
    std::vector<vslam_resect_refine> info;  // [pairs]: counts and costs before and after, kept rounds, stop
    std::vector<uint64_t> inlierBits;       // [pairs][(obsCap + 63) / 64]: observation record b is a member under the refined pose
};
RefinedResection refineResection(const std::vector<vslam_resect>& models, const std::vector<vslam_resect_corr>& correspondences, uint32_t obsCap,
                                 const vslam_resect_refine_params& params);

// Place recognition (include/vslam.h, "place recognition"): which earlier frame shows the same place?  A frame is the descriptor
// vector SIFT() fills, with its optional defined flags.
using DescriptorSets = std::vector<std::vector<std::vector<float>>>;  // [frame][descriptor][128]
using DefinedSets = std::vector<std::vector<unsigned char>>;         // [frame][descriptor]
struct Vocabulary {
    std::vector<float> words;            // [K][128]
    std::vector<unsigned char> defined;  // [K]
    uint32_t size() const { return (uint32_t)defined.size(); }
};
// K words copied from the frames' descriptors by the header's rule (set k % n, row ((k / n) * 2654435761 mod 2^32) % rows): the rule
// is a gather, restated on the host here; vslam_vocab_sample_dev is the same rule over device buffers.
Vocabulary sampleVocabulary(const DescriptorSets& frames, uint32_t K, const DefinedSets* defined = nullptr);
struct Words {
    std::vector<std::vector<int32_t>> word;  // [frame][descriptor]: the nearest word, -1: none
    std::vector<std::vector<float>> dist2;   // [frame][descriptor]: its d2, +inf with -1
    std::vector<uint32_t> hist;              // [frames][K]
    uint32_t K = 0;
};
// The nearest word of every descriptor and the histogram of words per frame, on the GPU (vslam_words_host).
Words assignWords(const DescriptorSets& frames, const Vocabulary& vocabulary, const DefinedSets* defined = nullptr);
// Vocabulary training (include/vslam.h, "vocabulary training"): `rounds` rounds of Lloyd's algorithm over the frames' descriptors
// from the words of `vocabulary` (sampleVocabulary's, say), on the GPU (vslam_vocab_kmeans_host).  The defined flags of the words
// do not change.
struct TrainedVocabulary {
    Vocabulary vocabulary;
    std::vector<uint32_t> sizes;             // [K]: the members of every word in the last round that updated
    std::vector<vslam_kmeans_round> report;  // [rounds]
};
TrainedVocabulary trainVocabulary(const DescriptorSets& frames, const Vocabulary& vocabulary, uint32_t rounds, const DefinedSets* defined = nullptr);
struct LoopCandidates {
    std::vector<std::vector<vslam_place_cand>> candidates;  // [query frame]: at most params.max_candidates, rank order
    std::vector<uint32_t> weights, selfQuery, selfDb;       // [K], [nq], [nd]
};
// Loop candidates of the frames qFirst + i (histQ [nq][K]) among the frames dbFirst + j (histDb [nd][K]), on the GPU
// (vslam_place_host).  One batch searched in itself: the same vector twice.
LoopCandidates findLoopCandidates(const std::vector<uint32_t>& histQ, uint32_t qFirst, const std::vector<uint32_t>& histDb, uint32_t dbFirst, uint32_t K,
                                  const vslam_place_params& params = {4, 3, 1, 5, 0, 0});

// Loop verification (include/vslam.h, "loop verification"): a candidate is a coincidence of words until geometry confirms it.
// matchPairs is the matcher over a table of (query frame, train frame) pairs, on the GPU (vslam_match_pairs_host): slot p gets the
// nearest two of every descriptor of frame pairs[p].query_set of `query` among those of frame pairs[p].train_set of `train` (the two
// may be one object).  A slot that names no frame on either side is empty: its lists are.
struct PairMatches {
    std::vector<std::vector<vslam_nn2>> nn;         // [slot][query descriptor]
    std::vector<std::vector<vslam_match>> matches;  // [slot]: the accepted queries, ascending query order
};
PairMatches matchPairs(const DescriptorSets& query, const DescriptorSets& train, const std::vector<vslam_set_pair>& pairs, float ratio = 0.8f,
                       const DefinedSets* queryDefined = nullptr, const DefinedSets* trainDefined = nullptr);
// The whole chain from candidates to loops over one sequence of frames searched in itself: the table of LoopCandidates::candidates
// (c = maxCandidates slots per frame, frame ids from dbFirst), matchPairs, the points of every matched record gathered, the
// fundamental matrix of every slot by RANSAC (vslam_epipolar_host with seed + slot: the sampling of slot p of one batched
// vslam_epipolar_dev call) and the verdict, on the GPU (vslam_loop_verdict_host).  points[f]: one keypoint per descriptor of frame f.
struct VerifiedLoops {
    std::vector<vslam_set_pair> pairs;              // [frames * c]
    std::vector<std::vector<vslam_match>> matches;  // [slot]
    std::vector<vslam_epipolar> models;             // [slot]
    std::vector<vslam_loop> loops;                  // [frame]: slot = -1 and train_set = -1 without a loop
    std::vector<int32_t> loopList;                  // the frames that have a loop, ascending
};
VerifiedLoops verifyLoops(const DescriptorSets& frames, const std::vector<std::vector<SLAM::point>>& points,
                          const std::vector<std::vector<vslam_place_cand>>& candidates, uint32_t maxCandidates, uint32_t dbFirst = 0,
                          const vslam_loop_params& params = {12, 2, 5, 0}, const vslam_epipolar_params& ransac = {512, 1, 4.0}, float ratio = 0.8f,
                          const DefinedSets* defined = nullptr);
// Frame structure (include/vslam.h, "frame structure"): what chainPoses read and wrote, seen per frame, on the GPU
// (vslam_frame_world_host): one camera per frame of the pairs + 1 frames and, per feature index, the lowest live record of the
// frame's source pair, or -1.  The world point of feature k of frame f is map[cams[f].pair][index[f][k]] of Trajectory::map.
struct FrameWorld {
    std::vector<vslam_frame_cam> cams;  // [pairs + 1]; empty without a pair
    std::vector<int32_t> index;         // [pairs + 1][pointCap]
};
FrameWorld frameWorld(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                      uint32_t matchCap, const std::vector<uint64_t>& frontBits, uint32_t pointCap, const std::vector<vslam_chain>& chain);

// Loop alignment (include/vslam.h, "loop alignment"): per slot of a set-pair table the similarity (s, R, t) with
// y_train_world = s R x_query_world + t between the world points of the slot's two frames, by RANSAC on the GPU (vslam_sim3_host;
// the sample, Horn's closed form, the composition with the two cameras and the two reprojection tests are stated in the header).
// One end of the loops: the frames of a chained run.  For loops inside one run both ends are one object.
struct WorldSide {
    FrameWorld frames;               // of frameWorld
    uint32_t pointCap = 0;           // as given to frameWorld
    std::vector<double> map;         // Trajectory::map, [pairs][mapCap][3]
    uint32_t mapCap = 0;             // the matchCap of the chained pairs
    std::vector<SLAM::point> points; // [pairs + 1][pointsCap]: the frames' point lists
    uint32_t pointsCap = 0;
};
struct LoopAlignment {
    std::vector<vslam_sim3> models;               // [slot]
    std::vector<uint64_t> inlierBits;             // [slot][(matchCap + 63) / 64]: the winner's inliers among the match records
    std::vector<vslam_sim3_corr> correspondences; // [slot][matchCap]: the first n_corr rows of a slot
    std::vector<int32_t> links;                   // [slot][matchCap][2]: the two map records of a match record, or -1
};
// matches [slots][matchCap] and matchCounts [slots] with real feature indices (PairMatches laid side by side); selectBits, when
// given, [slots][(matchCap + 63) / 64]: only the records whose bit is set take part.
LoopAlignment alignLoops(const WorldSide& query, const WorldSide& train, const std::vector<vslam_set_pair>& pairs,
                         const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts, uint32_t matchCap,
                         const vslam_sim3_params& params, const std::vector<uint64_t>* selectBits = nullptr);
}  // namespace vslam
