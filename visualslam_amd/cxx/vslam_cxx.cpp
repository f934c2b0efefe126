#include "vslam_cxx.hpp"

#include <algorithm>
#include <cmath>
#include <mutex>

using cv::Mat;

namespace vslam {

vslam_ctx* default_context(int device) {
    static std::mutex mu;
    static std::map<int, vslam_ctx*> ctxs;
    std::lock_guard<std::mutex> lock(mu);
    auto it = ctxs.find(device);
    if (it != ctxs.end()) return it->second;
    vslam_ctx* c = nullptr;
    const int rc = vslam_ctx_create(device, nullptr, &c);
    if (rc != VSLAM_OK) throw Error(rc, std::string("vslam_ctx_create: ") + vslam_status_string(rc) + " (no usable HIP device: there is no CPU fallback)");
    ctxs[device] = c;
    return c;
}

void check(int status, vslam_ctx* ctx, const char* what) {
    if (status != VSLAM_OK)
        throw Error(status, std::string(what) + ": " + vslam_status_string(status) + ": " + vslam_last_error(ctx));
}

}  // namespace vslam

using vslam::check;
using vslam::default_context;

static void require(bool ok, const char* msg) {
    if (!ok) throw vslam::Error(VSLAM_ERR_INVALID, msg);
}

namespace vslamcv {

void GaussianBlur(const Mat& src, Mat& dst, cv::Size ksize, double sigmaX, double, int) {
    require(src.type() == cv::CV_8U && ksize.width == ksize.height, "GaussianBlur: CV_8U, square kernels only");
    Mat out(src.rows, src.cols, cv::CV_8U);
    vslam_ctx* c = default_context();
    check(vslam_gaussian_blur_u8(c, src.data, src.rows, src.cols, src.step, ksize.width, sigmaX, out.data, out.step), c, "GaussianBlur");
    dst = out;
}

void Sobel(const Mat& src, Mat& dst, int ddepth, int dx, int dy, int ksize, double scale, double delta, int) {
    require(src.type() == cv::CV_8U && ddepth == cv::CV_32F && ksize == 1 && scale == 1 && delta == 0, "Sobel: CV_8U -> CV_32F, ksize 1 only");
    Mat out(src.rows, src.cols, cv::CV_32F);
    vslam_ctx* c = default_context();
    check(vslam_sobel_k1_u8_f32(c, src.data, src.rows, src.cols, src.step, dx, dy, out.ptr<float>(), out.step), c, "Sobel");
    dst = out;
}

void convertScaleAbs(const Mat& src, Mat& dst) {
    require(src.type() == cv::CV_32F, "convertScaleAbs: CV_32F input only");
    Mat out(src.rows, src.cols, cv::CV_8U);
    vslam_ctx* c = default_context();
    check(vslam_convert_scale_abs_f32(c, src.ptr<float>(), src.rows, src.cols, src.step, out.data, out.step), c, "convertScaleAbs");
    dst = out;
}

void resize(const Mat& src, Mat& dst, cv::Size, double fx, double fy, int interpolation) {
    require(src.type() == cv::CV_8U, "resize: CV_8U only");
    vslam_ctx* c = default_context();
    if (fx == 2 && fy == 2 && interpolation == INTER_LINEAR) {
        Mat out(src.rows * 2, src.cols * 2, cv::CV_8U);
        check(vslam_resize_linear2x_u8(c, src.data, src.rows, src.cols, src.step, out.data, out.step), c, "resize x2");
        dst = out;
    } else if (fx == 0.5 && fy == 0.5 && interpolation == INTER_NEAREST) {
        int r, cc;
        vslam_half_size(src.rows, src.cols, &r, &cc);
        Mat out(r, cc, cv::CV_8U);
        check(vslam_resize_nearest_half_u8(c, src.data, src.rows, src.cols, src.step, out.data, out.step), c, "resize x0.5");
        dst = out;
    } else {
        throw vslam::Error(VSLAM_ERR_UNSUPPORTED, "resize: only (2,2,INTER_LINEAR) and (0.5,0.5,INTER_NEAREST) are on the hot path");
    }
}

}  // namespace vslamcv

Mat HarrisCorner(Mat& Ix, Mat& Iy) {
    require(Ix.type() == cv::CV_32F && Iy.type() == cv::CV_32F && Ix.rows == Iy.rows && Ix.cols == Iy.cols && Ix.step == Iy.step,
            "HarrisCorner: two CV_32F gradients of equal geometry");
    // intended geometry rows x cols (the reference allocates it transposed: SURVEY Appendix B-1)
    Mat image(Ix.rows, Ix.cols, cv::CV_32F);
    vslam_ctx* c = default_context();
    check(vslam_harris_from_grad_f32(c, Ix.ptr<float>(), Iy.ptr<float>(), Ix.rows, Ix.cols, Ix.step, 0.04f, 3, image.ptr<float>(), image.step), c,
          "HarrisCorner");
    return image;
}

Mat NonMaximumSuppression(Mat& response, int windowSize) {
    Mat localMax(response.rows, response.cols, cv::CV_8U);
    vslam_ctx* c = default_context();
    if (response.type() == cv::CV_8U)
        check(vslam_nms_strict_u8(c, response.data, response.rows, response.cols, response.step, windowSize, localMax.data, localMax.step), c,
              "NonMaximumSuppression");
    else
        check(vslam_nms_strict_f32(c, response.ptr<float>(), response.rows, response.cols, response.step, windowSize, localMax.data, localMax.step),
              c, "NonMaximumSuppression");
    return localMax;
}

Mat NMS2(Mat& response, int windowSize) {
    require(response.type() == cv::CV_32F, "NMS2: CV_32F response");
    Mat nms(response.rows, response.cols, cv::CV_32F);  // intended f32 map (Appendix B-3)
    vslam_ctx* c = default_context();
    float true_max = 0;
    check(vslam_nms2_f32(c, response.ptr<float>(), response.rows, response.cols, response.step, windowSize, nms.ptr<float>(), nms.step, &true_max), c,
          "NMS2");
    return nms;
}

std::vector<vslam_kp> HarrisKeypoints(const Mat& gray, float k) {
    require(gray.type() == cv::CV_8U, "HarrisKeypoints: CV_8U frame");
    vslam_ctx* c = default_context();
    std::vector<vslam_kp> out(1 << 16);
    size_t n = 0;
    check(vslam_harris_keypoints_u8(c, gray.data, gray.rows, gray.cols, gray.step, k, out.data(), out.size(), &n), c, "HarrisKeypoints");
    if (n > out.size()) {
        out.resize(n);
        check(vslam_harris_keypoints_u8(c, gray.data, gray.rows, gray.cols, gray.step, k, out.data(), out.size(), &n), c, "HarrisKeypoints");
    }
    out.resize(n);
    return out;
}

// ------------------------------------------------------------------------------- GaussPyramid

GaussPyramid::GaussPyramid(Mat& img, int numOctaves, double sigma) { build(img, numOctaves, sigma); }
GaussPyramid::GaussPyramid(Mat& img, double sigma) { build(img, 0, sigma); }  // automatic octave count

GaussPyramid::~GaussPyramid() {
    if (pyr_) vslam_pyramid_destroy(pyr_);
}

void GaussPyramid::build(Mat& img, int numOctaves, double sigma) {
    require(img.type() == cv::CV_8U && !img.empty(), "GaussPyramid: CV_8U image");
    vslam_ctx* c = default_context();
    check(vslam_pyramid_build_u8(c, img.data, img.rows, img.cols, img.step, numOctaves, sigma, &pyr_), c, "GaussPyramid");
    check(vslam_pyramid_get_info(pyr_, &info_), c, "GaussPyramid info");
    for (int o = 0; o < info_.n_octaves; ++o)
        sigmas_[o] = std::vector<double>(info_.sigma[o], info_.sigma[o] + info_.n_levels);
    if (eagerGradients())  // processGradients for every octave now, as GaussPyramid.cpp:118 does
        for (int kind = 0; kind < 4; ++kind) (void)allGrads(kind);
}

namespace {
int g_eager_gradients = -1;  // -1: not set, follow the environment
}
void GaussPyramid::setEagerGradients(bool on) { g_eager_gradients = on ? 1 : 0; }
bool GaussPyramid::eagerGradients() {
    if (g_eager_gradients >= 0) return g_eager_gradients != 0;
    const char* e = std::getenv("VSLAM_EAGER_GRADIENTS");
    return e && e[0] == '1';
}

void GaussPyramid::checkOctave(int octave) const {
    if (octave < 0 || octave >= info_.n_octaves) throw std::out_of_range("GaussPyramid: octave");  // std::map::at in the reference
}

double GaussPyramid::getSigmaAt(int octave, int level) const {
    checkOctave(octave);
    if (level < 0 || level >= info_.n_levels) throw std::out_of_range("GaussPyramid: level");
    return info_.sigma[octave][level];
}

double GaussPyramid::calculateSigma(int octave, int level) const { return vslam_sigma_at(info_.sigma0, octave, level); }

const std::vector<double>& GaussPyramid::octaveSigma(int octave) {
    checkOctave(octave);
    return sigmas_.at(octave);
}

const std::vector<Mat>& GaussPyramid::octaveBlur(int octave) {
    checkOctave(octave);
    auto it = gauss_.find(octave);
    if (it == gauss_.end()) {
        std::vector<Mat> v;
        for (int l = 0; l < info_.n_levels; ++l) {
            Mat m(info_.rows[octave], info_.cols[octave], cv::CV_8U);
            check(vslam_pyramid_get_gauss(pyr_, octave, l, m.data, m.step), default_context(), "octaveBlur");
            v.push_back(m);
        }
        it = gauss_.emplace(octave, std::move(v)).first;
    }
    return it->second;
}

const std::vector<Mat>& GaussPyramid::octaveDiff(int octave) {
    checkOctave(octave);
    auto it = diff_.find(octave);
    if (it == diff_.end()) {
        std::vector<Mat> v;
        for (int l = 0; l < info_.n_dogs; ++l) {
            Mat m(info_.rows[octave], info_.cols[octave], cv::CV_8U);
            check(vslam_pyramid_get_dog(pyr_, octave, l, m.data, m.step), default_context(), "octaveDiff");
            v.push_back(m);
        }
        it = diff_.emplace(octave, std::move(v)).first;
    }
    return it->second;
}

const std::vector<Mat>& GaussPyramid::grads(int octave, int kind) {
    checkOctave(octave);
    auto it = grad_[kind].find(octave);
    if (it == grad_[kind].end()) {  // one kernel per level fills all four kinds of the octave
        std::vector<Mat> v[4];
        for (int l = 0; l < info_.n_levels; ++l) {
            Mat m[4];
            for (auto& q : m) q.create(info_.rows[octave], info_.cols[octave], cv::CV_32F);
            check(vslam_pyramid_get_gradients(pyr_, octave, l, m[0].ptr<float>(), m[1].ptr<float>(), m[2].ptr<float>(), m[3].ptr<float>(), m[0].step),
                  default_context(), "processGradients");
            for (int q = 0; q < 4; ++q) v[q].push_back(m[q]);
        }
        for (int q = 0; q < 4; ++q) grad_[q].emplace(octave, std::move(v[q]));
        it = grad_[kind].find(octave);
    }
    return it->second;
}

const std::vector<Mat>& GaussPyramid::imagePyramid() {
    if (img_pyramid_.empty())
        for (int o = 0; o < info_.n_octaves; ++o) {
            Mat m(info_.rows[o], info_.cols[o], cv::CV_8U);
            check(vslam_pyramid_get_base(pyr_, o, m.data, m.step), default_context(), "imagePyramid");
            img_pyramid_.push_back(m);
        }
    return img_pyramid_;
}

const Mat& GaussPyramid::octaveImage(int octave) {
    checkOctave(octave);
    return imagePyramid().at((size_t)octave);
}

const std::map<int, std::vector<Mat>>& GaussPyramid::pyramidGauss() {
    for (int o = 0; o < info_.n_octaves; ++o) octaveBlur(o);
    return gauss_;
}

const std::map<int, std::vector<Mat>>& GaussPyramid::allGrads(int kind) {
    for (int o = 0; o < info_.n_octaves; ++o) grads(o, kind);
    return grad_[kind];
}

const std::map<int, std::vector<Mat>>& GaussPyramid::pyramidDiff() {
    for (int o = 0; o < info_.n_octaves; ++o) octaveDiff(o);
    return diff_;
}

// copyMakeBorder(..., BORDER_REPLICATE) + clone (GaussPyramid.cpp:133-141).  Pure data movement
// for callers that want the padded copies; the extrema kernel itself clamps addresses instead.
std::vector<Mat> GaussPyramid::padOctave(int padding, const std::vector<Mat>& images) {
    std::vector<Mat> padded;
    for (const Mat& im : images) {
        Mat p(im.rows + 2 * padding, im.cols + 2 * padding, im.type());
        const size_t es = im.elemSize();
        for (int r = 0; r < p.rows; ++r) {
            const int sr = std::min(std::max(r - padding, 0), im.rows - 1);
            for (int c = 0; c < p.cols; ++c) {
                const int sc = std::min(std::max(c - padding, 0), im.cols - 1);
                std::memcpy(p.data + p.step * r + es * c, im.data + im.step * sr + es * sc, es);
            }
        }
        padded.push_back(p);
    }
    return padded;
}

template <class F>
static void append_points(std::vector<SLAM::point>& dst, F&& call) {
    vslam_ctx* c = default_context();
    size_t n = 0;
    std::vector<vslam_point> buf(1 << 16);
    check(call(c, buf.data(), buf.size(), &n), c, "initialKeypointDetection");
    if (n > buf.size()) {
        buf.resize(n);
        check(call(c, buf.data(), buf.size(), &n), c, "initialKeypointDetection");
    }
    for (size_t i = 0; i < n; ++i)
        dst.emplace_back(buf[i].row, buf[i].col, buf[i].value, buf[i].padding, buf[i].octave, buf[i].level);
}

void initialKeypointDetection(std::vector<SLAM::point>& keypoints, GaussPyramid& pyramid, int octave, int windowSize) {
    append_points(keypoints, [&](vslam_ctx* c, vslam_point* out, size_t cap, size_t* n) {
        return vslam_dog_keypoints(c, pyramid.handle(), octave, windowSize, out, cap, n);
    });
}

void scaleSpaceCandidates(std::vector<SLAM::point>& candidates, GaussPyramid& pyramid, int octave, int windowSize, int minContrast) {
    append_points(candidates, [&](vslam_ctx* c, vslam_point* out, size_t cap, size_t* n) {
        return vslam_dog_extrema(c, pyramid.handle(), octave, windowSize, minContrast, nullptr, out, cap, n);
    });
}

void scaleSpaceExtremaDense(std::vector<SLAM::point>& candidates, GaussPyramid& pyramid, int octave, int minContrast) {
    append_points(candidates, [&](vslam_ctx* c, vslam_point* out, size_t cap, size_t* n) {
        return vslam_dog_extrema_dense(c, pyramid.handle(), octave, minContrast, nullptr, out, cap, n);
    });
}

bool FeaturePointLocalization(std::vector<cv::Mat>& dogs_padded, std::vector<SLAM::point>& keypoints, int level, SLAM::point& point) {
    vslam_ctx* c = default_context();
    if (level < 1 || level + 1 >= (int)dogs_padded.size()) throw vslam::Error(VSLAM_ERR_RANGE, "FeaturePointLocalization: level out of range");
    const cv::Mat& d = dogs_padded[level];
    const int i = point.row, j = point.col;
    if (i < 1 || j < 1 || i + 1 >= d.rows || j + 1 >= d.cols) throw vslam::Error(VSLAM_ERR_RANGE, "FeaturePointLocalization: point outside the padded image");
    const int q[4] = {(int)d.at<cv::uchar>(i, j - 1) - (int)d.at<cv::uchar>(i, j + 1),                                    // :226
                      (int)d.at<cv::uchar>(i - 1, j) - (int)d.at<cv::uchar>(i + 1, j),                                    // :227
                      (int)dogs_padded[level - 1].at<cv::uchar>(i, j) - (int)dogs_padded[level + 1].at<cv::uchar>(i, j),  // :228
                      point.value};
    int keep = 0, value = point.value;
    check(vslam_localize_points(c, q, 1, &keep, &value), c, "FeaturePointLocalization");
    if (!keep) return false;
    point.value = value;  // :246
    keypoints.emplace_back(point);
    return true;
}

float computeEdgeResponse(const SLAM::point& keypoint, const cv::Mat& grad_x, const cv::Mat& grad_y) {
    vslam_ctx* c = default_context();
    const int x = keypoint.col, y = keypoint.row, p = keypoint.padding;
    if (p < 0 || y - p < 0 || x - p < 0 || y + p > grad_x.rows || x + p > grad_x.cols || grad_y.rows != grad_x.rows || grad_y.cols != grad_x.cols)
        throw vslam::Error(VSLAM_ERR_RANGE, "computeEdgeResponse: window outside the gradient images");
    std::vector<float> wx, wy;
    for (int u = y - p; u < y + p; ++u)      // :93
        for (int v = x - p; v < x + p; ++v) {  // :94
            wx.push_back(grad_x.at<float>(u, v));
            wy.push_back(grad_y.at<float>(u, v));
        }
    float response = 0.f;
    check(vslam_edge_response_windows(c, wx.data(), wy.data(), (int)wx.size(), 1, &response), c, "computeEdgeResponse");
    return response;
}

void filterKeypoints(GaussPyramid& pyramid, int octave, std::vector<SLAM::point>& keypoints, std::vector<SLAM::point>& reducedKeypoints) {
    vslam_ctx* c = default_context();
    static_assert(sizeof(SLAM::point) == sizeof(vslam_point), "SLAM::point must stay binary compatible with vslam_point");
    const vslam_point* in = reinterpret_cast<const vslam_point*>(keypoints.data());
    size_t n = 0;
    std::vector<vslam_point> buf(std::max<size_t>(64, 2 * keypoints.size()));
    check(vslam_filter_keypoints(c, pyramid.handle(), octave, in, keypoints.size(), buf.data(), buf.size(), &n), c, "filterKeypoints");
    if (n > buf.size()) {
        buf.resize(n);
        check(vslam_filter_keypoints(c, pyramid.handle(), octave, in, keypoints.size(), buf.data(), buf.size(), &n), c, "filterKeypoints");
    }
    for (size_t i = 0; i < n; ++i)
        reducedKeypoints.emplace_back(buf[i].row, buf[i].col, buf[i].value, buf[i].padding, buf[i].octave, buf[i].level);
}

void StructureMatrix(cv::Mat& M, cv::Mat& Ix, cv::Mat& Iy, int padding, int i, int j) {
    vslam_ctx* c = default_context();
    if (padding < 0 || i - padding < 0 || j - padding < 0 || i + padding >= Ix.rows || j + padding >= Ix.cols || Iy.rows != Ix.rows ||
        Iy.cols != Ix.cols || M.rows < 2 || M.cols < 2)
        throw vslam::Error(VSLAM_ERR_RANGE, "StructureMatrix: window outside the gradient images");
    std::vector<float> wx, wy;
    for (int u = i - padding; u <= i + padding; ++u)      // :16
        for (int v = j - padding; v <= j + padding; ++v) {  // :17
            wx.push_back(Ix.at<float>(u, v));
            wy.push_back(Iy.at<float>(u, v));
        }
    float m[3] = {0.f, 0.f, 0.f};
    check(vslam_structure_matrix_windows(c, wx.data(), wy.data(), (int)wx.size(), 1, m), c, "StructureMatrix");
    M.at<float>(0, 0) = m[0];  // :25-28
    M.at<float>(0, 1) = m[1];
    M.at<float>(1, 0) = m[1];
    M.at<float>(1, 1) = m[2];
}

// ---- Rotation (include/src/Rotation/rotation.cpp) ------------------------------------------------

namespace SLAM {
float Rotation::convertToRadians(float theta) {  // rotation.cpp:5-7
    return (float)((double)theta * (3.1415926535897932384626433832795 / (double)180.0f));
}
const cv::Point2f Rotation::cos_sin_of_angle(float theta, bool degrees) {  // :9-17
    if (degrees) {
        float c, s;
        vslam_cos_sin_deg(theta, &c, &s);
        return cv::Point2f(c, s);
    }
    return cv::Point2f((float)std::cos((double)theta), (float)std::sin((double)theta));
}
cv::Point2i Rotation::rotate_pt_CW(const cv::Point2i& pt, const cv::Point2i& center, const cv::Point2f& angles) {  // :19-27
    cv::Point2i rot(pt.x, pt.y);
    rot -= center;
    const float a = (float)rot.x * angles.x, b = (float)rot.y * angles.y, d = (float)rot.x * angles.y, e = (float)rot.y * angles.x;
    const int x_r = (int)(a - b), y_r = (int)(d + e);
    return cv::Point2i(x_r + center.x, y_r + center.y);
}
cv::Point2i Rotation::rotate_pt_CW(const cv::Point2i& pt, const cv::Point2i& center, float theta, bool degrees) {  // :53-63
    return rotate_pt_CW(pt, center, cos_sin_of_angle(theta, degrees));
}
std::vector<cv::Point2i> Rotation::getRotatedWindowPoints(cv::Mat&, const cv::Point2i& center, int windowSize, float theta, bool degrees) {  // :112-130
    std::vector<cv::Point2i> out;
    if (windowSize <= 0) return out;
    if (!degrees) {
        const int padding = windowSize / 2;
        const cv::Point2f angles = cos_sin_of_angle(theta, false);
        for (int i = center.y - padding; i <= center.y + padding; ++i)
            for (int j = center.x - padding; j <= center.x + padding; ++j) out.push_back(rotate_pt_CW(cv::Point2i(j, i), center, angles));
        return out;
    }
    std::vector<int32_t> xy(2 * (size_t)(windowSize + 1) * (windowSize + 1));
    if (vslam_rotated_window_points(center.x, center.y, windowSize, theta, xy.data()) != VSLAM_OK)
        throw vslam::Error(VSLAM_ERR_INVALID, "getRotatedWindowPoints: bad arguments");
    for (size_t q = 0; q < xy.size() / 2; ++q) out.emplace_back(xy[2 * q], xy[2 * q + 1]);
    return out;
}
}  // namespace SLAM

// ---- SIFT (Diff_of_Gauss.cpp:561-693) ---------------------------------------------------------------

void SIFT(std::vector<SLAM::point>& reducedKeypoints, std::vector<std::vector<float>>& featureDescriptors_vec, GaussPyramid& pyramid,
          int octave, std::vector<unsigned char>* defined) {
    vslam_ctx* c = vslam::default_context();
    const size_t n = reducedKeypoints.size();
    if (defined) defined->assign(n, 1);
    if (n == 0) return;
    std::vector<float> desc(128 * n);
    std::vector<unsigned char> def(n, 1);
    vslam::check(vslam_sift_descriptors(c, pyramid.handle(), octave, reinterpret_cast<const vslam_point*>(reducedKeypoints.data()), n,
                                        desc.data(), defined ? def.data() : nullptr),
                 c, "SIFT");
    for (size_t i = 0; i < n; ++i) featureDescriptors_vec.emplace_back(desc.begin() + 128 * i, desc.begin() + 128 * (i + 1));  // :678
    if (defined) *defined = def;
}

void writeFeatureDescriptors(const std::string& file_name, const std::vector<std::vector<float>>& v) {
    std::vector<float> flat;
    flat.reserve(128 * v.size());
    for (const auto& d : v) {
        if (d.size() != 128) throw vslam::Error(VSLAM_ERR_INVALID, "writeFeatureDescriptors: a descriptor is not 128 floats");
        flat.insert(flat.end(), d.begin(), d.end());
    }
    if (vslam_descriptor_file_write(file_name.c_str(), flat.data(), v.size()) != VSLAM_OK)
        throw vslam::Error(VSLAM_ERR_INVALID, "writeFeatureDescriptors: cannot write " + file_name);
}

// ---- matching (the step after SIFT; no reference counterpart beyond the comment at Diff_of_Gauss.cpp:687) ---------

vslam::Matches vslam::matchDescriptors(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train, float ratio,
                                       const std::vector<unsigned char>* query_defined, const std::vector<unsigned char>* train_defined) {
    auto flatten = [](const std::vector<std::vector<float>>& v, const std::vector<unsigned char>* defined) {
        require(!defined || defined->size() == v.size(), "matchDescriptors: one defined flag per descriptor");
        std::vector<float> flat;
        flat.reserve(128 * v.size());
        for (const auto& d : v) {
            require(d.size() == 128, "matchDescriptors: a descriptor is not 128 floats");
            flat.insert(flat.end(), d.begin(), d.end());
        }
        return flat;
    };
    const std::vector<float> q = flatten(query, query_defined), t = flatten(train, train_defined);
    vslam::Matches out;
    out.nn.resize(query.size());
    out.matches.resize(query.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_match_host(c, q.data(), query_defined ? query_defined->data() : nullptr, nullptr, query.size(), t.data(),
                                  train_defined ? train_defined->data() : nullptr, nullptr, train.size(), ratio * ratio, 0,
                                  out.nn.empty() ? nullptr : out.nn.data(), out.matches.empty() ? nullptr : out.matches.data(), out.matches.size(), &total),
                 c, "matchDescriptors");
    out.matches.resize(total);
    return out;
}

vslam::Matches vslam::matchMutual(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train, float ratio,
                                  const std::vector<unsigned char>* query_defined, const std::vector<unsigned char>* train_defined) {
    auto flatten = [](const std::vector<std::vector<float>>& v, const std::vector<unsigned char>* defined) {
        require(!defined || defined->size() == v.size(), "matchMutual: one defined flag per descriptor");
        std::vector<float> flat;
        flat.reserve(128 * v.size());
        for (const auto& d : v) {
            require(d.size() == 128, "matchMutual: a descriptor is not 128 floats");
            flat.insert(flat.end(), d.begin(), d.end());
        }
        return flat;
    };
    const std::vector<float> q = flatten(query, query_defined), t = flatten(train, train_defined);
    vslam::Matches out;
    out.nn.resize(query.size());
    out.rnn.resize(train.size());
    out.matches.resize(query.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_match_mutual_host(c, q.data(), query_defined ? query_defined->data() : nullptr, nullptr, query.size(), t.data(),
                                         train_defined ? train_defined->data() : nullptr, nullptr, train.size(), ratio * ratio, 0,
                                         out.nn.empty() ? nullptr : out.nn.data(), out.rnn.empty() ? nullptr : out.rnn.data(),
                                         out.matches.empty() ? nullptr : out.matches.data(), out.matches.size(), &total),
                 c, "matchMutual");
    out.matches.resize(total);
    return out;
}

vslam::Matches vslam::matchGuided(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train,
                                  const std::vector<SLAM::point>& queryPoints, const std::vector<SLAM::point>& trainPoints, const vslam_epipolar& model,
                                  const vslam_guided_params& params, const std::vector<unsigned char>* query_defined,
                                  const std::vector<unsigned char>* train_defined) {
    static_assert(sizeof(SLAM::point) == sizeof(vslam_point), "SLAM::point is the ABI's point record");
    require(queryPoints.size() == query.size() && trainPoints.size() == train.size(), "matchGuided: one keypoint per descriptor");
    auto flatten = [](const std::vector<std::vector<float>>& v, const std::vector<unsigned char>* defined) {
        require(!defined || defined->size() == v.size(), "matchGuided: one defined flag per descriptor");
        std::vector<float> flat;
        flat.reserve(128 * v.size());
        for (const auto& d : v) {
            require(d.size() == 128, "matchGuided: a descriptor is not 128 floats");
            flat.insert(flat.end(), d.begin(), d.end());
        }
        return flat;
    };
    const std::vector<float> q = flatten(query, query_defined), t = flatten(train, train_defined);
    vslam::Matches out;
    out.nn.resize(query.size());
    out.matches.resize(query.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_match_guided_host(c, q.data(), query_defined ? query_defined->data() : nullptr,
                                         reinterpret_cast<const vslam_point*>(queryPoints.data()), query.size(), t.data(),
                                         train_defined ? train_defined->data() : nullptr, reinterpret_cast<const vslam_point*>(trainPoints.data()),
                                         train.size(), &model, &params, out.nn.empty() ? nullptr : out.nn.data(),
                                         out.matches.empty() ? nullptr : out.matches.data(), out.matches.size(), &total),
                 c, "matchGuided");
    out.matches.resize(total);
    return out;
}

vslam::Matches vslam::matchGuidedHF(const std::vector<std::vector<float>>& query, const std::vector<std::vector<float>>& train,
                                    const std::vector<SLAM::point>& queryPoints, const std::vector<SLAM::point>& trainPoints,
                                    const vslam_epipolar* epipolarModel, const vslam_homography* homographyModel, const vslam_guided_hf_params& params,
                                    const std::vector<unsigned char>* query_defined, const std::vector<unsigned char>* train_defined) {
    static_assert(sizeof(SLAM::point) == sizeof(vslam_point), "SLAM::point is the ABI's point record");
    require(epipolarModel || homographyModel, "matchGuidedHF: no model");
    require(queryPoints.size() == query.size() && trainPoints.size() == train.size(), "matchGuidedHF: one keypoint per descriptor");
    auto flatten = [](const std::vector<std::vector<float>>& v, const std::vector<unsigned char>* defined) {
        require(!defined || defined->size() == v.size(), "matchGuidedHF: one defined flag per descriptor");
        std::vector<float> flat;
        flat.reserve(128 * v.size());
        for (const auto& d : v) {
            require(d.size() == 128, "matchGuidedHF: a descriptor is not 128 floats");
            flat.insert(flat.end(), d.begin(), d.end());
        }
        return flat;
    };
    const std::vector<float> q = flatten(query, query_defined), t = flatten(train, train_defined);
    vslam::Matches out;
    out.nn.resize(query.size());
    out.matches.resize(query.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_match_guided_hf_host(c, q.data(), query_defined ? query_defined->data() : nullptr,
                                            reinterpret_cast<const vslam_point*>(queryPoints.data()), query.size(), t.data(),
                                            train_defined ? train_defined->data() : nullptr, reinterpret_cast<const vslam_point*>(trainPoints.data()),
                                            train.size(), epipolarModel, homographyModel, &params, out.nn.empty() ? nullptr : out.nn.data(),
                                            out.matches.empty() ? nullptr : out.matches.data(), out.matches.size(), &total),
                 c, "matchGuidedHF");
    out.matches.resize(total);
    return out;
}

// ---- two-view geometry (the reference's README step 3; no reference code) ------------------------------------------

vslam::Epipolar vslam::fundamentalRansac(const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                                         const std::vector<SLAM::point>& trainPoints, const vslam_epipolar_params& params) {
    static_assert(sizeof(SLAM::point) == sizeof(vslam_point), "SLAM::point is the ABI's point record");
    vslam::Epipolar out{};
    out.inliers.resize(matches.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_epipolar_host(c, matches.empty() ? nullptr : matches.data(), matches.size(),
                                     reinterpret_cast<const vslam_point*>(queryPoints.data()), queryPoints.size(),
                                     reinterpret_cast<const vslam_point*>(trainPoints.data()), trainPoints.size(), &params, &out.model, nullptr,
                                     out.inliers.empty() ? nullptr : out.inliers.data(), out.inliers.size(), &total, nullptr),
                 c, "fundamentalRansac");
    out.inliers.resize(total);
    return out;
}

vslam::Refit vslam::refitFundamental(const vslam_epipolar& model, const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                                     const std::vector<SLAM::point>& trainPoints, const vslam_refit_params& params) {
    vslam::Refit out{};
    out.inliers.resize(matches.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_refit_host(c, &model, matches.empty() ? nullptr : matches.data(), matches.size(),
                                  reinterpret_cast<const vslam_point*>(queryPoints.data()), queryPoints.size(),
                                  reinterpret_cast<const vslam_point*>(trainPoints.data()), trainPoints.size(), &params, &out.model, &out.info, nullptr,
                                  out.inliers.empty() ? nullptr : out.inliers.data(), out.inliers.size(), &total),
                 c, "refitFundamental");
    out.inliers.resize(total);
    return out;
}

vslam::Homography vslam::findHomography(const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                                        const std::vector<SLAM::point>& trainPoints, const vslam_epipolar* epipolarModel,
                                        const vslam_homography_params& params) {
    vslam::Homography out{};
    out.inliers.resize(matches.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_homography_host(c, matches.empty() ? nullptr : matches.data(), matches.size(),
                                       reinterpret_cast<const vslam_point*>(queryPoints.data()), queryPoints.size(),
                                       reinterpret_cast<const vslam_point*>(trainPoints.data()), trainPoints.size(), epipolarModel, &params, &out.model,
                                       nullptr, out.inliers.empty() ? nullptr : out.inliers.data(), out.inliers.size(), &total, nullptr,
                                       epipolarModel ? &out.gated : nullptr),
                 c, "findHomography");
    out.inliers.resize(total);
    return out;
}

vslam::HomographyRefit vslam::refitHomography(const vslam_homography& model, const std::vector<vslam_match>& matches,
                                              const std::vector<SLAM::point>& queryPoints, const std::vector<SLAM::point>& trainPoints,
                                              const vslam_hrefit_params& params, const vslam_epipolar* epipolarModel) {
    vslam::HomographyRefit out{};
    out.inliers.resize(matches.size());
    size_t total = 0;
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_hrefit_host(c, &model, matches.empty() ? nullptr : matches.data(), matches.size(),
                                   reinterpret_cast<const vslam_point*>(queryPoints.data()), queryPoints.size(),
                                   reinterpret_cast<const vslam_point*>(trainPoints.data()), trainPoints.size(), epipolarModel, &params, &out.model,
                                   &out.info, nullptr, out.inliers.empty() ? nullptr : out.inliers.data(), out.inliers.size(), &total,
                                   epipolarModel ? &out.gated : nullptr),
                 c, "refitHomography");
    out.inliers.resize(total);
    return out;
}

vslam::Pose vslam::relativePose(const vslam_epipolar& model, const std::vector<vslam_match>& matches, const std::vector<SLAM::point>& queryPoints,
                                const std::vector<SLAM::point>& trainPoints, const vslam_pose_params& camera) {
    vslam::Pose out{};
    out.points.resize(matches.size() * 3);
    out.frontBits.resize((matches.size() + 63) / 64);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_pose_host(c, &model, matches.empty() ? nullptr : matches.data(), matches.size(),
                                 reinterpret_cast<const vslam_point*>(queryPoints.data()), queryPoints.size(),
                                 reinterpret_cast<const vslam_point*>(trainPoints.data()), trainPoints.size(), &camera, &out.pose, out.candidates,
                                 out.points.empty() ? nullptr : out.points.data(), out.frontBits.empty() ? nullptr : out.frontBits.data()),
                 c, "relativePose");
    if (out.pose.best < 0) out.points.clear();
    return out;
}

vslam::HomographyPose vslam::poseFromHomography(const vslam_homography& model, const std::vector<vslam_match>& matches,
                                                const std::vector<SLAM::point>& queryPoints, const std::vector<SLAM::point>& trainPoints,
                                                const vslam_pose_params& camera, vslam::Pose& pose, const vslam_pose* prior, double maxDist2,
                                                double minSpread, uint32_t ambiguousNum, uint32_t ambiguousDen, bool onlyDegenerate) {
    const size_t m = matches.size(), words = (m + 63) / 64;
    require(m < (1u << 31) && queryPoints.size() < (1u << 31) && trainPoints.size() < (1u << 31), "poseFromHomography: too many records");
    require(m == 0 || (!queryPoints.empty() && !trainPoints.empty()), "poseFromHomography: matches without points");
    require(pose.pose.n_matches == m && (pose.points.empty() || pose.points.size() == m * 3) && (pose.frontBits.empty() || pose.frontBits.size() == words),
            "poseFromHomography: pose is not relativePose's over these matches");
    // the batched entry point takes capacities of at least one: an empty list goes up as one unused record
    std::vector<vslam_match> mt(matches);
    std::vector<SLAM::point> qp(queryPoints), tp(trainPoints);
    mt.resize(std::max<size_t>(m, 1)), qp.resize(std::max<size_t>(qp.size(), 1)), tp.resize(std::max<size_t>(tp.size(), 1));
    const uint32_t count = (uint32_t)m;
    std::vector<double> points(mt.size() * 3, 0.0);
    std::vector<uint64_t> bits((mt.size() + 63) / 64, 0);
    vslam_pose rec = pose.pose;
    vslam::HomographyPose out{};
    vslam_hpose_out o{};
    o.struct_size = sizeof(o);
    o.poses = &rec, o.poses_bytes = sizeof(rec);
    o.info = &out.info, o.info_bytes = sizeof(out.info);
    o.candidates = out.candidates, o.candidates_bytes = sizeof(out.candidates);
    o.points = points.data(), o.points_bytes = points.size() * sizeof(double);
    o.front_bits = bits.data(), o.front_bits_bytes = bits.size() * sizeof(uint64_t);
    const vslam_hpose_params params{camera, maxDist2, minSpread, ambiguousNum, ambiguousDen, onlyDegenerate ? 1 : 0, 0};
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_hpose_host(c, &model, mt.data(), &count, (uint32_t)mt.size(), reinterpret_cast<const vslam_point*>(qp.data()), (uint32_t)qp.size(),
                                  reinterpret_cast<const vslam_point*>(tp.data()), (uint32_t)tp.size(), 1, prior, &params, &o),
                 c, "poseFromHomography");
    if (model.best >= 0 && (!onlyDegenerate || model.degenerate != 0)) {  // selected: the pair's record, points and bits are the call's
        pose.pose = rec;
        points.resize(rec.best >= 0 ? m * 3 : 0);
        bits.resize(words);
        pose.points.swap(points), pose.frontBits.swap(bits);
    }
    return out;
}

vslam::Trajectory vslam::chainPoses(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                                    uint32_t matchCap, const std::vector<double>& points, const std::vector<uint64_t>& frontBits, uint32_t pointCap,
                                    const vslam_chain_params& params) {
    const size_t n = poses.size(), recs = n * matchCap;
    require(n <= 65535 && matchCounts.size() == n && matches.size() == recs && points.size() == recs * 3 &&
                frontBits.size() == n * (((size_t)matchCap + 63) / 64),
            "chainPoses: one count, matchCap records, matchCap points and (matchCap + 63) / 64 words per pair");
    vslam::Trajectory out;
    out.chain.resize(n);
    out.map.assign(recs * 3, 0.0);
    out.links.assign(recs, -1);
    out.ratios.assign(recs, 0.0);
    if (n == 0) return out;
    vslam_chain_out o{};
    o.struct_size = sizeof(o);
    o.chain = out.chain.data(), o.chain_bytes = n * sizeof(vslam_chain);
    o.map = out.map.data(), o.map_bytes = out.map.size() * sizeof(double);
    o.links = out.links.data(), o.links_bytes = out.links.size() * sizeof(int32_t);
    o.ratios = out.ratios.data(), o.ratios_bytes = out.ratios.size() * sizeof(double);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_chain_host(c, poses.data(), matches.data(), matchCounts.data(), matchCap, points.data(), frontBits.data(), pointCap, (int)n, &params,
                                  &o),
                 c, "chainPoses");
    return out;
}

vslam::Tracks vslam::buildTracks(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                                 uint32_t matchCap, const std::vector<uint64_t>& frontBits, uint32_t pointCap, const std::vector<vslam_chain>& chain,
                                 const std::vector<SLAM::point>& framePoints, const vslam_tracks_params& params) {
    const size_t n = poses.size(), recs = n * matchCap, words = n * (((size_t)matchCap + 63) / 64);
    require(n <= 65535 && matchCounts.size() == n && matches.size() == recs && frontBits.size() == words && chain.size() == n &&
                (n == 0 || framePoints.size() == (n + 1) * pointCap),
            "buildTracks: one count and one chain record, matchCap records and (matchCap + 63) / 64 words per pair, pointCap points per frame");
    vslam::Tracks out;
    out.tracks.assign(recs, vslam_track{});
    out.refs.assign(recs, vslam_track_ref{0xffffffffu, 0xffffffffu});
    out.goodBits.assign(words, 0);
    out.summary.assign(n, vslam_track_summary{});
    if (n == 0) return out;
    vslam_tracks_out o{};
    o.struct_size = sizeof(o);
    o.tracks = out.tracks.data(), o.tracks_bytes = recs * sizeof(vslam_track);
    o.refs = out.refs.data(), o.refs_bytes = recs * sizeof(vslam_track_ref);
    o.good_bits = out.goodBits.data(), o.good_bits_bytes = words * sizeof(uint64_t);
    o.summary = out.summary.data(), o.summary_bytes = n * sizeof(vslam_track_summary);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_tracks_host(c, poses.data(), matches.data(), matchCounts.data(), matchCap, frontBits.data(), pointCap, (int)n, chain.data(),
                                   reinterpret_cast<const vslam_point*>(framePoints.data()), &params, &o),
                 c, "buildTracks");
    return out;
}

vslam::Bundle vslam::bundleAdjust(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                                  uint32_t matchCap, const std::vector<uint64_t>& frontBits, uint32_t pointCap, const std::vector<vslam_chain>& chain,
                                  const std::vector<SLAM::point>& framePoints, const std::vector<vslam_track>& tracksIn,
                                  const std::vector<vslam_track_ref>& refs, const std::vector<vslam_bundle_cam>& camsIn,
                                  const vslam_bundle_params& params) {
    const size_t n = poses.size(), recs = n * matchCap, words = n * (((size_t)matchCap + 63) / 64);
    require(n <= 65535 && matchCounts.size() == n && matches.size() == recs && frontBits.size() == words && chain.size() == n &&
                (n == 0 || framePoints.size() == (n + 1) * pointCap),
            "bundleAdjust: one count and one chain record, matchCap records and (matchCap + 63) / 64 words per pair, pointCap points per frame");
    require(tracksIn.size() == recs && refs.size() == recs && (camsIn.empty() || camsIn.size() == n),
            "bundleAdjust: matchCap tracks and refs per pair, and no cameras or one per pair");
    vslam::Bundle out;
    out.tracks = tracksIn;
    out.cams.assign(n, vslam_bundle_cam{});
    out.pointInfo.assign(recs, vslam_bundle_point{});
    out.memberBits.assign(2 * words, 0);
    if (n == 0) return out;
    vslam_bundle_out o{};
    o.struct_size = sizeof(o);
    o.tracks = out.tracks.data(), o.tracks_bytes = recs * sizeof(vslam_track);
    o.cams = out.cams.data(), o.cams_bytes = n * sizeof(vslam_bundle_cam);
    o.point_info = out.pointInfo.data(), o.point_info_bytes = recs * sizeof(vslam_bundle_point);
    o.member_bits = out.memberBits.data(), o.member_bits_bytes = 2 * words * sizeof(uint64_t);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_bundle_host(c, poses.data(), matches.data(), matchCounts.data(), matchCap, frontBits.data(), pointCap, (int)n, chain.data(),
                                   reinterpret_cast<const vslam_point*>(framePoints.data()), tracksIn.data(), refs.data(),
                                   camsIn.empty() ? nullptr : camsIn.data(), &params, &o),
                 c, "bundleAdjust");
    return out;
}

vslam::Resection vslam::resectPoses(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                                    uint32_t matchCap, const std::vector<double>& points, const std::vector<uint64_t>& frontBits, uint32_t pointCap,
                                    const std::vector<vslam_match>& obsMatches, const std::vector<uint32_t>& obsCounts, uint32_t obsCap,
                                    const std::vector<SLAM::point>& trainPoints, uint32_t trainCap, const vslam_resect_params& params) {
    const size_t n = poses.size(), recs = n * matchCap, orecs = n * obsCap, owords = n * (((size_t)obsCap + 63) / 64);
    require(n <= 65535 && matchCounts.size() == n && matches.size() == recs && points.size() == recs * 3 &&
                frontBits.size() == n * (((size_t)matchCap + 63) / 64),
            "resectPoses: one count, matchCap records, matchCap points and (matchCap + 63) / 64 words per pair");
    require(obsCounts.size() == n && obsMatches.size() == orecs && trainPoints.size() == n * trainCap,
            "resectPoses: one count, obsCap observation records and trainCap points per pair");
    vslam::Resection out;
    out.models.resize(n);
    out.inlierBits.assign(owords, 0);
    out.correspondences.assign(orecs, vslam_resect_corr{});
    out.links.assign(orecs, -1);
    if (n == 0) return out;
    vslam_resect_out o{};
    o.struct_size = sizeof(o);
    o.models = out.models.data(), o.models_bytes = n * sizeof(vslam_resect);
    o.inlier_bits = out.inlierBits.data(), o.inlier_bits_bytes = owords * sizeof(uint64_t);
    o.correspondences = out.correspondences.data(), o.correspondences_bytes = orecs * sizeof(vslam_resect_corr);
    o.links = out.links.data(), o.links_bytes = orecs * sizeof(int32_t);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_resect_host(c, poses.data(), matches.data(), matchCounts.data(), matchCap, points.data(), frontBits.data(), pointCap,
                                   obsMatches.data(), obsCounts.data(), obsCap, reinterpret_cast<const vslam_point*>(trainPoints.data()), trainCap, (int)n,
                                   &params, &o),
                 c, "resectPoses");
    return out;
}

vslam::RefinedResection vslam::refineResection(const std::vector<vslam_resect>& models, const std::vector<vslam_resect_corr>& correspondences,
                                               uint32_t obsCap, const vslam_resect_refine_params& params) {
    const size_t n = models.size(), orecs = n * obsCap, owords = n * (((size_t)obsCap + 63) / 64);
    require(n <= 65535 && correspondences.size() == orecs, "refineResection: obsCap correspondence rows per pair");
    vslam::RefinedResection out;
    out.models.resize(n);
    out.info.assign(n, vslam_resect_refine{});
    out.inlierBits.assign(owords, 0);
    if (n == 0) return out;
    vslam_resect_refine_out o{};
    o.struct_size = sizeof(o);
    o.models = out.models.data(), o.models_bytes = n * sizeof(vslam_resect);
    o.info = out.info.data(), o.info_bytes = n * sizeof(vslam_resect_refine);
    o.inlier_bits = out.inlierBits.data(), o.inlier_bits_bytes = owords * sizeof(uint64_t);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_resect_refine_host(c, models.data(), correspondences.data(), obsCap, (int)n, &params, &o), c, "refineResection");
    return out;
}

// ---- place recognition (include/vslam.h, "place recognition") -----------------------------------------------------

static void requireFrames(const vslam::DescriptorSets& frames, const vslam::DefinedSets* defined, const char* sizes, const char* row) {
    require(!defined || defined->size() == frames.size(), sizes);
    for (size_t f = 0; f < frames.size(); ++f) {
        require(!defined || (*defined)[f].size() == frames[f].size(), sizes);
        for (const auto& d : frames[f]) require(d.size() == 128, row);
    }
}

// The frames as the host arrays of the *_host entry points: desc [n][cap][128], defined [n][cap], counts [n]; cap >= 1.
struct PackedFrames {
    size_t cap = 1;
    std::vector<float> desc;
    std::vector<unsigned char> def;
    std::vector<uint32_t> counts;
    PackedFrames(const vslam::DescriptorSets& frames, const vslam::DefinedSets* defined, const char* tooMany) : counts(frames.size()) {
        const size_t n = frames.size();
        for (const auto& f : frames) cap = std::max(cap, f.size());
        require(cap <= 0xffffffffu, tooMany);
        desc.assign(n * cap * 128, 0.0f);
        def.assign(n * cap, 1);
        for (size_t f = 0; f < n; ++f) {
            counts[f] = (uint32_t)frames[f].size();
            for (size_t r = 0; r < frames[f].size(); ++r) {
                std::copy(frames[f][r].begin(), frames[f][r].end(), desc.begin() + (f * cap + r) * 128);
                if (defined) def[f * cap + r] = (*defined)[f][r];
            }
        }
    }
};

vslam::Vocabulary vslam::sampleVocabulary(const DescriptorSets& frames, uint32_t K, const DefinedSets* defined) {
    requireFrames(frames, defined, "sampleVocabulary: one defined flag per descriptor", "sampleVocabulary: a descriptor is not 128 floats");
    require(!frames.empty() && frames.size() <= 65535 && K >= 1 && K <= 65536, "sampleVocabulary: 1 .. 65535 frames, 1 .. 65536 words");
    vslam::Vocabulary v;
    v.words.assign((size_t)K * 128, 0.0f);
    v.defined.assign(K, 0);
    const uint32_t n = (uint32_t)frames.size();
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t s = k % n, rows = (uint32_t)std::min<size_t>(frames[s].size(), 0xffffffffu);
        if (rows == 0) continue;
        const uint32_t r = (uint32_t)((k / n) * 2654435761u) % rows;
        if (defined && !(*defined)[s][r]) continue;
        std::copy(frames[s][r].begin(), frames[s][r].end(), v.words.begin() + (size_t)k * 128);
        v.defined[k] = 1;
    }
    return v;
}

vslam::Words vslam::assignWords(const DescriptorSets& frames, const Vocabulary& vocabulary, const DefinedSets* defined) {
    requireFrames(frames, defined, "assignWords: one defined flag per descriptor", "assignWords: a descriptor is not 128 floats");
    const uint32_t K = vocabulary.size();
    require(vocabulary.words.size() == (size_t)K * 128, "assignWords: 128 floats per word");
    require(frames.size() <= 65535 && K >= 1 && K <= 65536, "assignWords: at most 65535 frames, 1 .. 65536 words");
    const size_t n = frames.size();
    const PackedFrames p(frames, defined, "assignWords: too many descriptors");
    const size_t cap = p.cap;
    const std::vector<float>& desc = p.desc;
    const std::vector<unsigned char>& def = p.def;
    const std::vector<uint32_t>& counts = p.counts;
    std::vector<float> d2(n * cap, 0.0f);
    std::vector<int32_t> w(n * cap, -1);
    vslam::Words out;
    out.K = K;
    out.hist.assign(n * K, 0);
    out.word.resize(n), out.dist2.resize(n);
    if (n == 0) return out;
    vslam_words_out o{};
    o.struct_size = sizeof(o);
    o.words = w.data(), o.words_bytes = w.size() * sizeof(int32_t);
    o.word_dist2 = d2.data(), o.word_dist2_bytes = d2.size() * sizeof(float);
    o.hist = out.hist.data(), o.hist_bytes = out.hist.size() * sizeof(uint32_t);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_words_host(c, desc.data(), def.data(), counts.data(), (uint32_t)cap, (int)n, vocabulary.words.data(), vocabulary.defined.data(), K, &o), c,
                 "assignWords");
    for (size_t f = 0; f < n; ++f) {
        out.word[f].assign(w.begin() + f * cap, w.begin() + f * cap + counts[f]);
        out.dist2[f].assign(d2.begin() + f * cap, d2.begin() + f * cap + counts[f]);
    }
    return out;
}

vslam::LoopCandidates vslam::findLoopCandidates(const std::vector<uint32_t>& histQ, uint32_t qFirst, const std::vector<uint32_t>& histDb, uint32_t dbFirst,
                                                uint32_t K, const vslam_place_params& params) {
    require(K >= 1 && K <= 65536, "findLoopCandidates: 1 .. 65536 words");
    require(histQ.size() % K == 0 && histDb.size() % K == 0, "findLoopCandidates: K entries per frame");
    const size_t nq = histQ.size() / K, nd = histDb.size() / K;
    require(nq <= 65535 && nd <= 65535, "findLoopCandidates: at most 65535 frames on either side");
    require(params.max_candidates >= 1 && params.max_candidates <= 8, "findLoopCandidates: max_candidates must be 1 .. 8");
    const uint32_t cmax = params.max_candidates;
    vslam::LoopCandidates out;
    out.candidates.resize(nq);
    out.weights.assign(K, 0), out.selfQuery.assign(nq, 0), out.selfDb.assign(nd, 0);
    if (nq == 0) return out;
    std::vector<vslam_place_cand> cands(nq * cmax);
    std::vector<uint32_t> counts(nq, 0);
    vslam_place_out o{};
    o.struct_size = sizeof(o);
    o.candidates = cands.data(), o.candidates_bytes = cands.size() * sizeof(vslam_place_cand);
    o.cand_counts = counts.data(), o.cand_counts_bytes = counts.size() * sizeof(uint32_t);
    o.weights = out.weights.data(), o.weights_bytes = out.weights.size() * sizeof(uint32_t);
    o.self_q = out.selfQuery.data(), o.self_q_bytes = nq * sizeof(uint32_t);
    if (nd) o.self_db = out.selfDb.data(), o.self_db_bytes = nd * sizeof(uint32_t);
    vslam_ctx* c = vslam::default_context();
    const bool same = &histQ == &histDb;
    vslam::check(vslam_place_host(c, histQ.data(), (uint32_t)nq, qFirst, same ? histQ.data() : (nd ? histDb.data() : nullptr), (uint32_t)nd, dbFirst, K, &params,
                                  &o), c, "findLoopCandidates");
    for (size_t i = 0; i < nq; ++i) out.candidates[i].assign(cands.begin() + i * cmax, cands.begin() + i * cmax + std::min(counts[i], cmax));
    return out;
}

// ---- vocabulary training (include/vslam.h, "vocabulary training") --------------------------------------------------

vslam::TrainedVocabulary vslam::trainVocabulary(const DescriptorSets& frames, const Vocabulary& vocabulary, uint32_t rounds, const DefinedSets* defined) {
    requireFrames(frames, defined, "trainVocabulary: one defined flag per descriptor", "trainVocabulary: a descriptor is not 128 floats");
    const uint32_t K = vocabulary.size();
    require(vocabulary.words.size() == (size_t)K * 128, "trainVocabulary: 128 floats per word");
    require(frames.size() <= 65535 && K >= 1 && K <= 65536, "trainVocabulary: at most 65535 frames, 1 .. 65536 words");
    require(rounds >= 1 && rounds <= 64, "trainVocabulary: rounds must be 1 .. 64");
    const PackedFrames p(frames, defined, "trainVocabulary: too many descriptors");
    require((uint64_t)frames.size() * p.cap <= 0xffffffffull, "trainVocabulary: too many descriptors");
    vslam::TrainedVocabulary out;
    out.vocabulary.words.assign((size_t)K * 128, 0.0f);
    out.vocabulary.defined = vocabulary.defined;
    out.sizes.assign(K, 0);
    out.report.assign(rounds, vslam_kmeans_round{0, 0, 0, 0});
    const vslam_kmeans_params params{rounds, 0};
    vslam_kmeans_out o{};
    o.struct_size = sizeof(o);
    o.vocab = out.vocabulary.words.data(), o.vocab_bytes = out.vocabulary.words.size() * sizeof(float);
    o.sizes = out.sizes.data(), o.sizes_bytes = out.sizes.size() * sizeof(uint32_t);
    o.report = out.report.data(), o.report_bytes = out.report.size() * sizeof(vslam_kmeans_round);
    const uint32_t none = 0;  // (no frames: the entry point still asks for the two pointers)
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_vocab_kmeans_host(c, frames.empty() ? vocabulary.words.data() : p.desc.data(), frames.empty() ? nullptr : p.def.data(),
                                         frames.empty() ? &none : p.counts.data(), (uint32_t)p.cap, (int)frames.size(), vocabulary.words.data(),
                                         vocabulary.defined.data(), K, &params, &o), c, "trainVocabulary");
    return out;
}

// ---- loop verification (include/vslam.h, "loop verification") -------------------------------------------------------

static bool emptyPair(const vslam_set_pair& pr, size_t nQuery, size_t nTrain) { return (uint32_t)pr.query_set >= nQuery || (uint32_t)pr.train_set >= nTrain; }

vslam::PairMatches vslam::matchPairs(const DescriptorSets& query, const DescriptorSets& train, const std::vector<vslam_set_pair>& pairs, float ratio,
                                     const DefinedSets* queryDefined, const DefinedSets* trainDefined) {
    requireFrames(query, queryDefined, "matchPairs: one defined flag per descriptor", "matchPairs: a descriptor is not 128 floats");
    const bool same = &query == &train && queryDefined == trainDefined;
    if (!same) requireFrames(train, trainDefined, "matchPairs: one defined flag per descriptor", "matchPairs: a descriptor is not 128 floats");
    require(query.size() <= 65535 && train.size() <= 65535 && pairs.size() <= 65535, "matchPairs: at most 65535 frames on either side and 65535 pairs");
    require(std::isfinite(ratio) && ratio > 0.0f, "matchPairs: ratio must be finite and positive");
    vslam::PairMatches out;
    out.nn.resize(pairs.size()), out.matches.resize(pairs.size());
    if (pairs.empty()) return out;
    const PackedFrames q(query, queryDefined, "matchPairs: too many descriptors");
    const vslam::DescriptorSets noFrames;
    const PackedFrames t(same ? noFrames : train, same ? nullptr : trainDefined, "matchPairs: too many descriptors");
    static const float noRow[128] = {};  // (a side without frames is never read: the entry point still asks for its pointers)
    static const uint32_t noCount = 0;
    auto sets = [&](const PackedFrames& f, size_t n) {
        return vslam_desc_sets{n ? f.desc.data() : noRow, n ? f.def.data() : nullptr, nullptr, n ? f.counts.data() : &noCount, (uint32_t)f.cap};
    };
    const vslam_desc_sets Q = sets(q, query.size()), T = same ? Q : sets(t, train.size());
    const size_t n = pairs.size(), cap = q.cap;
    std::vector<vslam_nn2> nn(n * cap);
    std::vector<vslam_match> matches(n * cap);
    std::vector<uint32_t> counts(n, 0);
    vslam_match_out o{};
    o.struct_size = sizeof(o);
    o.nn = nn.data(), o.nn_bytes = nn.size() * sizeof(vslam_nn2);
    o.matches = matches.data(), o.matches_bytes = matches.size() * sizeof(vslam_match), o.match_cap = (uint32_t)cap;
    o.match_counts = counts.data(), o.match_counts_bytes = counts.size() * sizeof(uint32_t);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_match_pairs_host(c, &Q, (int)query.size(), &T, (int)train.size(), pairs.data(), (int)n, ratio * ratio, 0, &o), c, "matchPairs");
    for (size_t p = 0; p < n; ++p) {
        if (emptyPair(pairs[p], query.size(), train.size())) continue;
        out.nn[p].assign(nn.begin() + p * cap, nn.begin() + p * cap + q.counts[pairs[p].query_set]);
        out.matches[p].assign(matches.begin() + p * cap, matches.begin() + p * cap + std::min<size_t>(counts[p], cap));
    }
    return out;
}

vslam::VerifiedLoops vslam::verifyLoops(const DescriptorSets& frames, const std::vector<std::vector<SLAM::point>>& points,
                                        const std::vector<std::vector<vslam_place_cand>>& candidates, uint32_t maxCandidates, uint32_t dbFirst,
                                        const vslam_loop_params& params, const vslam_epipolar_params& ransac, float ratio, const DefinedSets* defined) {
    const size_t n = frames.size(), cmax = maxCandidates;
    require(points.size() == n && candidates.size() == n, "verifyLoops: one point list and one candidate list per frame");
    for (size_t f = 0; f < n; ++f) require(points[f].size() == frames[f].size(), "verifyLoops: one keypoint per descriptor");
    require(cmax >= 1 && cmax <= 8, "verifyLoops: maxCandidates must be 1 .. 8");
    require(n * cmax <= 65535, "verifyLoops: at most 65535 slots");
    require(params.min_inliers >= 1 && params.den > 0 && params.reserved == 0, "verifyLoops: min_inliers and den must be positive, reserved 0");
    vslam::VerifiedLoops out;
    out.pairs.assign(n * cmax, vslam_set_pair{-1, -1});
    for (size_t i = 0; i < n; ++i)
        for (size_t r = 0; r < std::min(candidates[i].size(), cmax); ++r) {
            const long long d = (long long)candidates[i][r].frame - (long long)dbFirst;
            if (d >= 0 && d < (long long)n) out.pairs[i * cmax + r] = vslam_set_pair{(int32_t)i, (int32_t)d};
        }
    out.matches = vslam::matchPairs(frames, frames, out.pairs, ratio, defined, defined).matches;
    out.models.assign(n * cmax, vslam_epipolar{});
    out.loops.resize(n);
    if (n == 0) return out;
    for (size_t p = 0; p < out.pairs.size(); ++p) {
        out.models[p].best = -1;
        if (emptyPair(out.pairs[p], n, n)) continue;
        // the gather: record i of the local list is record i of the slot's matches
        const std::vector<vslam_match>& m = out.matches[p];
        std::vector<vslam_match> local(m.size());
        std::vector<SLAM::point> qp(m.size()), tp(m.size());
        for (size_t i = 0; i < m.size(); ++i) {
            local[i] = vslam_match{(int32_t)i, (int32_t)i, m[i].dist2};
            qp[i] = points[out.pairs[p].query_set][m[i].query];
            tp[i] = points[out.pairs[p].train_set][m[i].train];
        }
        vslam_epipolar_params prm = ransac;
        prm.seed = ransac.seed + (uint32_t)p;  // hypothesis h of pair 0 under seed + p draws what pair p draws under seed
        out.models[p] = vslam::fundamentalRansac(local, qp, tp, prm).model;
    }
    std::vector<int32_t> list(n, -1);
    uint32_t count = 0;
    vslam_loop_out o{};
    o.struct_size = sizeof(o);
    o.loops = out.loops.data(), o.loops_bytes = out.loops.size() * sizeof(vslam_loop);
    o.loop_list = list.data(), o.loop_list_bytes = list.size() * sizeof(int32_t);
    o.n_loops = &count, o.n_loops_bytes = sizeof(count);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_loop_verdict_host(c, out.models.data(), out.pairs.data(), (uint32_t)n, (uint32_t)cmax, (uint32_t)n, &params, &o), c, "verifyLoops");
    out.loopList.assign(list.begin(), list.begin() + std::min<size_t>(count, n));
    return out;
}

vslam::FrameWorld vslam::frameWorld(const std::vector<vslam_pose>& poses, const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts,
                                    uint32_t matchCap, const std::vector<uint64_t>& frontBits, uint32_t pointCap, const std::vector<vslam_chain>& chain) {
    const size_t n = poses.size();
    require(n <= 65535 && matchCounts.size() == n && chain.size() == n && matches.size() == n * matchCap &&
                frontBits.size() == n * (((size_t)matchCap + 63) / 64),
            "frameWorld: one count, one chain record, matchCap records and (matchCap + 63) / 64 words per pair");
    vslam::FrameWorld out;
    if (n == 0) return out;
    out.cams.resize(n + 1);
    out.index.assign((n + 1) * pointCap, -1);
    vslam_frame_world_out o{};
    o.struct_size = sizeof(o);
    o.cams = out.cams.data(), o.cams_bytes = out.cams.size() * sizeof(vslam_frame_cam);
    o.index = out.index.data(), o.index_bytes = out.index.size() * sizeof(int32_t);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_frame_world_host(c, poses.data(), matches.data(), matchCounts.data(), matchCap, frontBits.data(), pointCap, chain.data(), (int)n, &o),
                 c, "frameWorld");
    return out;
}

static vslam_sim3_side sim3Side(const vslam::WorldSide& s, const char* sizes) {
    const size_t nf = s.frames.cams.size();
    require(nf <= 65536 && s.pointCap && s.mapCap && s.pointsCap && s.frames.index.size() == nf * s.pointCap && s.points.size() == nf * s.pointsCap &&
                !s.map.empty() && s.map.size() % ((size_t)s.mapCap * 3) == 0 && s.map.size() / ((size_t)s.mapCap * 3) <= 65535,
            sizes);
    return vslam_sim3_side{s.frames.cams.data(), s.frames.index.data(), s.map.data(), reinterpret_cast<const vslam_point*>(s.points.data()), s.mapCap,
                           s.pointCap, s.pointsCap, (uint32_t)(s.map.size() / ((size_t)s.mapCap * 3)), (int32_t)nf, 0};
}

vslam::LoopAlignment vslam::alignLoops(const vslam::WorldSide& query, const vslam::WorldSide& train, const std::vector<vslam_set_pair>& pairs,
                                       const std::vector<vslam_match>& matches, const std::vector<uint32_t>& matchCounts, uint32_t matchCap,
                                       const vslam_sim3_params& params, const std::vector<uint64_t>* selectBits) {
    const size_t n = pairs.size(), recs = n * matchCap, words = n * (((size_t)matchCap + 63) / 64);
    require(n <= 65535 && matchCap > 0 && matchCounts.size() == n && matches.size() == recs && (!selectBits || selectBits->size() == words),
            "alignLoops: one count, matchCap records and (matchCap + 63) / 64 select words per slot");
    const vslam_pose_params& K = params.K;
    require(params.n_hypotheses >= 1 && params.n_hypotheses <= 65535 && std::isfinite(params.max_dist2) && params.max_dist2 > 0.0 && std::isfinite(K.fx) &&
                std::isfinite(K.fy) && std::isfinite(K.cx) && std::isfinite(K.cy) && K.fx > 0.0 && K.fy > 0.0,
            "alignLoops: 1 .. 65535 hypotheses, a finite positive max_dist2, finite intrinsics with positive fx and fy");
    const char* sizes = "alignLoops: a side is frames [frames] with index [frames][pointCap], map [pairs][mapCap][3] and points [frames][pointsCap]";
    const vslam_sim3_side q = sim3Side(query, sizes), t = &train == &query ? q : sim3Side(train, sizes);
    vslam::LoopAlignment out;
    out.models.resize(n);
    out.inlierBits.assign(words, 0);
    out.correspondences.resize(recs);
    out.links.assign(recs * 2, -1);
    if (n == 0) return out;
    vslam_sim3_out o{};
    o.struct_size = sizeof(o);
    o.models = out.models.data(), o.models_bytes = n * sizeof(vslam_sim3);
    o.inlier_bits = out.inlierBits.data(), o.inlier_bits_bytes = words * sizeof(uint64_t);
    o.correspondences = out.correspondences.data(), o.correspondences_bytes = recs * sizeof(vslam_sim3_corr);
    o.links = out.links.data(), o.links_bytes = out.links.size() * sizeof(int32_t);
    vslam_ctx* c = vslam::default_context();
    vslam::check(vslam_sim3_host(c, &q, &t, pairs.data(), matches.data(), matchCounts.data(), matchCap, selectBits ? selectBits->data() : nullptr, (int)n,
                                 &params, &o),
                 c, "alignLoops");
    return out;
}
