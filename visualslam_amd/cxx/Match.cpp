// The step the reference's `DoG` executable stops short of (Diff_of_Gauss.cpp:687, "final step is graphing and comparing
// two images with each other"): the DoG pipeline of DoG.cpp on two images - pyramid, initialKeypointDetection,
// filterKeypoints and SIFT per octave - and then every descriptor of the first matched against every descriptor of the
// second (vslam::matchDescriptors: exact nearest two, ratio test 0.8).  Prints one JSON line with the counts.  --mutual (first)
// takes the cross-checked list instead (vslam::matchMutual: the accepted queries whose train descriptor chose them back): the
// line gains "mutual": true, "accepted" counts that list and every step after it reads it.  --epipolar adds
// the step after that: the RANSAC fundamental matrix of the accepted matches (vslam::fundamentalRansac: 512 hypotheses, seed 1,
// Sampson distance below 2 pixels) as an "epipolar" object with the inlier count and F.  --guided [max_dist2[,ratio[,max_desc_dist2]]]
// (after --epipolar; defaults 4.0, 0.8, no bound) matches again inside each query's epipolar band under that F
// (vslam::matchGuided) and runs the same RANSAC on the guided list: "guided_matches" and "guided_inliers"; the steps after it
// still read the first list.  --homography (after these) adds
// the RANSAC homography of the same matches and the degeneracy verdict (vslam::findHomography: 512 hypotheses, seed 1, transfer
// error below 2 pixels, degenerate from n_H / n_F >= 1 / 2 with at least 16 inliers) as a "homography" object; the steps after
// it then read the gated model, so a degenerate pair gets no refit and no pose.  --guided-h [max_transfer2[,ratio[,max_desc_dist2]]]
// (after --homography; defaults 4.0, 0.8, no bound) matches again under the model that applies to the pair - the band under the
// gated F, or a window around H x when the pair is degenerate (vslam::matchGuidedHF) - and runs the RANSAC homography on that
// list: "guided_hf_kind", "guided_hf_matches" and "guided_hf_h_inliers".  --hrefit ROUNDS (straight after --homography) refits H
// over all its inliers first (vslam::refitHomography) and prints an "hrefit" object with n_before, n_after, accepted, stop, the
// verdict run again and the new H; --guided-h and --hpose then read the refitted model and its gate.  --refit ROUNDS (after these)
// refits that model over all its inliers (vslam::refitFundamental) and prints a "refit" object with n_before, n_after,
// accepted, stop and the new F.  --pose fx,fy,cx,cy (after --epipolar and --refit) adds the step after that: the camera motion
// from the inlier matches - the refit's when --refit is given - (vslam::relativePose) as a "pose" object with R, t, the winning
// candidate and the number of inliers in front of both cameras.
// --hpose (after --homography and --pose) adds the pose of a pair the gate removed, from H itself (vslam::poseFromHomography
// into a copy of that pose): an "hpose" object with kind, best, ambiguous, n_support, front, front_runner and the pose it left.
//   usage: Match [--mutual] [--epipolar [--guided [D2[,RATIO[,BOUND]]]] [--homography [--hrefit ROUNDS] [--guided-h [T2[,RATIO[,BOUND]]]]] [--refit ROUNDS] [--pose fx,fy,cx,cy [--hpose]]] [first.pgm second.pgm | WxH] [octaves, default 4]
//          (WxH: frames 0 and 1 of the synthetic stream)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "imgio.hpp"
#include "vslam_cxx.hpp"

using namespace cv;

namespace {
struct Described {
    std::vector<std::vector<float>> descriptors;
    std::vector<unsigned char> defined;
    std::vector<SLAM::point> points;  // the oriented keypoint of every descriptor
    size_t n_defined = 0;
};

Described describe(Mat img, int numOctaves) {  // (the reference's constructor takes a non-const Mat&)
    Described out;
    GaussPyramid pyramid{img, numOctaves, 1.6};
    for (int octave = 0; octave < pyramid.getNumOctaves(); ++octave) {
        std::vector<SLAM::point> keypoints, reducedKeypoints;
        initialKeypointDetection(keypoints, pyramid, octave, 3);
        filterKeypoints(pyramid, octave, keypoints, reducedKeypoints);
        std::vector<unsigned char> defined;
        SIFT(reducedKeypoints, out.descriptors, pyramid, octave, &defined);
        out.defined.insert(out.defined.end(), defined.begin(), defined.end());
        out.points.insert(out.points.end(), reducedKeypoints.begin(), reducedKeypoints.end());
    }
    for (unsigned char d : out.defined) out.n_defined += d != 0;
    return out;
}
}  // namespace

int main(int argc, char** argv) {
    try {
        const bool mutual = argc > 1 && std::strcmp(argv[1], "--mutual") == 0;
        if (mutual) --argc, ++argv;
        const bool epipolar = argc > 1 && std::strcmp(argv[1], "--epipolar") == 0;
        if (epipolar) --argc, ++argv;
        // the optional value of --guided / --guided-h is all numbers and commas ("4.0", "4.0,0.8,1.0"): "512x384" and "a.pgm" are not
        auto threeNumbers = [&](double& first, float& ratio2, float& bound) {
            double a = 0.0, ratio = 0.0, b = 0.0;
            int used = 0;
            const int got = argc > 1 ? std::sscanf(argv[1], "%lf%n,%lf%n,%lf%n", &a, &used, &ratio, &used, &b, &used) : 0;
            if (got >= 1 && argv[1][used] == '\0') {
                first = a;
                if (got >= 2) ratio2 = (float)ratio * (float)ratio;
                if (got >= 3) bound = (float)b;
                --argc, ++argv;
            }
        };
        vslam_guided_params guidedParams{0.64f, HUGE_VALF, 4.0, 0, 0};
        const bool guided = epipolar && argc > 1 && std::strcmp(argv[1], "--guided") == 0;
        if (guided) {
            --argc, ++argv;
            threeNumbers(guidedParams.max_dist2, guidedParams.ratio2, guidedParams.max_desc_dist2);
        }
        const bool homography = epipolar && argc > 1 && std::strcmp(argv[1], "--homography") == 0;
        if (homography) --argc, ++argv;
        vslam_hrefit_params hrefitParams{0, 4.0, 1, 2, 16};
        const bool hrefit = homography && argc > 2 && std::strcmp(argv[1], "--hrefit") == 0;
        if (hrefit) {
            if (std::sscanf(argv[2], "%u", &hrefitParams.rounds) != 1 || hrefitParams.rounds < 1 || hrefitParams.rounds > 8)
                throw std::runtime_error("--hrefit takes the number of rounds, 1 .. 8");
            argc -= 2, argv += 2;
        }
        vslam_guided_hf_params guidedHfParams{0.64f, HUGE_VALF, 4.0, 4.0, 0, 0};
        const bool guidedH = homography && argc > 1 && std::strcmp(argv[1], "--guided-h") == 0;
        if (guidedH) {
            --argc, ++argv;
            threeNumbers(guidedHfParams.max_transfer2, guidedHfParams.ratio2, guidedHfParams.max_desc_dist2);
        }
        vslam_refit_params refitParams{0, 4.0};
        const bool refit = epipolar && argc > 2 && std::strcmp(argv[1], "--refit") == 0;
        if (refit) {
            if (std::sscanf(argv[2], "%u", &refitParams.rounds) != 1 || refitParams.rounds < 1 || refitParams.rounds > 8)
                throw std::runtime_error("--refit takes the number of rounds, 1 .. 8");
            argc -= 2, argv += 2;
        }
        vslam_pose_params camera{};
        const bool pose = epipolar && argc > 2 && std::strcmp(argv[1], "--pose") == 0;
        if (pose) {
            if (std::sscanf(argv[2], "%lf,%lf,%lf,%lf", &camera.fx, &camera.fy, &camera.cx, &camera.cy) != 4)
                throw std::runtime_error("--pose takes fx,fy,cx,cy");
            argc -= 2, argv += 2;
        }
        const bool hpose = pose && homography && argc > 1 && std::strcmp(argv[1], "--hpose") == 0;
        if (hpose) --argc, ++argv;
        Mat first, second;
        int w = 0, h = 0, next = 2;
        if (argc < 2) {
            first = imgio::synthetic(384, 512, 0), second = imgio::synthetic(384, 512, 1);
        } else if (std::sscanf(argv[1], "%dx%d", &w, &h) == 2 && w > 0 && h > 0) {
            first = imgio::synthetic(h, w, 0), second = imgio::synthetic(h, w, 1);
        } else {
            if (argc < 3) throw std::runtime_error("usage: Match [--mutual] [--epipolar [--guided [D2[,RATIO[,BOUND]]]] [--homography [--hrefit ROUNDS] [--guided-h [T2[,RATIO[,BOUND]]]]] [--refit ROUNDS] [--pose fx,fy,cx,cy [--hpose]]] [first.pgm second.pgm | WxH] [octaves]");
            first = imgio::read_pgm(argv[1]), second = imgio::read_pgm(argv[2]);
            next = 3;
        }
        const int numOctaves = argc > next ? std::atoi(argv[next]) : 4;
        const auto t0 = std::chrono::steady_clock::now();
        const Described q = describe(first, numOctaves), t = describe(second, numOctaves);
        const vslam::Matches m = mutual ? vslam::matchMutual(q.descriptors, t.descriptors, 0.8f, &q.defined, &t.defined)
                                        : vslam::matchDescriptors(q.descriptors, t.descriptors, 0.8f, &q.defined, &t.defined);
        std::string extra = mutual ? ", \"mutual\": true" : "";
        if (epipolar) {
            const vslam::Epipolar e = vslam::fundamentalRansac(m.matches, q.points, t.points);
            char buf[512];
            std::snprintf(buf, sizeof buf, ", \"epipolar\": {\"n_inliers\": %u, \"best\": %d, \"n_valid\": %u, \"hypotheses\": 512, \"max_dist2\": 4.0, \"F\": [", e.model.n_inliers,
                          e.model.best, e.model.n_valid);
            extra += buf;
            for (int i = 0; i < 9; ++i) {
                std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", e.model.F[i]);
                extra += buf;
            }
            extra += "]}";
            if (guided) {
                const vslam::Matches g = vslam::matchGuided(q.descriptors, t.descriptors, q.points, t.points, e.model, guidedParams, &q.defined, &t.defined);
                const vslam::Epipolar ge = vslam::fundamentalRansac(g.matches, q.points, t.points);
                std::snprintf(buf, sizeof buf, ", \"guided_matches\": %zu, \"guided_inliers\": %u", g.matches.size(), ge.model.n_inliers);
                extra += buf;
            }
            vslam_epipolar model = e.model;
            std::vector<vslam_match> inliers = e.inliers;
            vslam_homography hmodel{};
            hmodel.best = -1;
            if (homography) {
                const vslam::Homography hg = vslam::findHomography(m.matches, q.points, t.points, &e.model);
                std::snprintf(buf, sizeof buf, ", \"homography\": {\"n_inliers\": %u, \"best\": %d, \"n_valid\": %u, \"n_epipolar\": %u, \"degenerate\": %d, \"H\": [",
                              hg.model.n_inliers, hg.model.best, hg.model.n_valid, hg.model.n_epipolar, hg.model.degenerate);
                extra += buf;
                for (int i = 0; i < 9; ++i) {
                    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", hg.model.H[i]);
                    extra += buf;
                }
                extra += "]}";
                model = hg.gated, hmodel = hg.model;
                if (hrefit) {
                    const vslam::HomographyRefit hr = vslam::refitHomography(hg.model, m.matches, q.points, t.points, hrefitParams, &e.model);
                    std::snprintf(buf, sizeof buf, ", \"hrefit\": {\"rounds\": %u, \"n_before\": %u, \"n_after\": %u, \"accepted\": %u, \"stop\": %d, "
                                  "\"n_epipolar\": %u, \"degenerate\": %d, \"H\": [",
                                  hrefitParams.rounds, hr.info.n_before, hr.info.n_after, hr.info.accepted, hr.info.stop, hr.model.n_epipolar, hr.model.degenerate);
                    extra += buf;
                    for (int i = 0; i < 9; ++i) {
                        std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", hr.model.H[i]);
                        extra += buf;
                    }
                    extra += "]}";
                    model = hr.gated, hmodel = hr.model;
                }
                if (guidedH) {
                    const vslam::Matches g = vslam::matchGuidedHF(q.descriptors, t.descriptors, q.points, t.points, &model, &hmodel, guidedHfParams,
                                                                  &q.defined, &t.defined);
                    const vslam::Homography gh = vslam::findHomography(g.matches, q.points, t.points);
                    std::snprintf(buf, sizeof buf, ", \"guided_hf_kind\": \"%s\", \"guided_hf_matches\": %zu, \"guided_hf_h_inliers\": %u",
                                  model.best >= 0 ? "F" : hmodel.best >= 0 ? "H" : "none", g.matches.size(), gh.model.n_inliers);
                    extra += buf;
                }
            }
            if (refit) {
                const vslam::Refit r = vslam::refitFundamental(model, m.matches, q.points, t.points, refitParams);
                std::snprintf(buf, sizeof buf, ", \"refit\": {\"rounds\": %u, \"n_before\": %u, \"n_after\": %u, \"accepted\": %u, \"stop\": %d, \"F\": [",
                              refitParams.rounds, r.info.n_before, r.info.n_after, r.info.accepted, r.info.stop);
                extra += buf;
                for (int i = 0; i < 9; ++i) {
                    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", r.model.F[i]);
                    extra += buf;
                }
                extra += "]}";
                model = r.model, inliers = r.inliers;
            }
            if (pose) {
                const vslam::Pose p = vslam::relativePose(model, inliers, q.points, t.points, camera);
                std::snprintf(buf, sizeof buf, ", \"pose\": {\"n_matches\": %u, \"n_front\": %u, \"best\": %d, \"valid\": %d, \"R\": [", p.pose.n_matches,
                              p.pose.n_front, p.pose.best, p.pose.valid);
                extra += buf;
                for (int i = 0; i < 9; ++i) {
                    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", p.pose.R[i]);
                    extra += buf;
                }
                extra += "], \"t\": [";
                for (int i = 0; i < 3; ++i) {
                    std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", p.pose.t[i]);
                    extra += buf;
                }
                extra += "]}";
                if (hpose) {
                    vslam::Pose filled = p;
                    const vslam::HomographyPose hp = vslam::poseFromHomography(hmodel, inliers, q.points, t.points, camera, filled);
                    std::snprintf(buf, sizeof buf, ", \"hpose\": {\"kind\": %d, \"best\": %d, \"ambiguous\": %d, \"n_support\": %u, \"front\": %u, "
                                  "\"front_runner\": %u, \"pose_best\": %d, \"pose_n_front\": %u}",
                                  hp.info.kind, hp.info.best, hp.info.ambiguous, hp.info.n_support, hp.info.front, hp.info.front_runner, filled.pose.best,
                                  filled.pose.n_front);
                    extra += buf;
                }
            }
        }
        const auto t1 = std::chrono::steady_clock::now();
        size_t exact = 0, nearest = 0;
        for (const vslam_nn2& r : m.nn) nearest += r.index >= 0;
        for (const vslam_match& a : m.matches) exact += a.dist2 == 0.0f;
        std::printf("{\"exe\": \"Match\", \"octaves\": %d, \"query\": {\"rows\": %d, \"cols\": %d, \"descriptors\": %zu, \"defined\": %zu}, "
                    "\"train\": {\"rows\": %d, \"cols\": %d, \"descriptors\": %zu, \"defined\": %zu}, \"with_nearest\": %zu, \"accepted\": %zu, "
                    "\"zero_distance\": %zu, \"ratio\": 0.8, \"ms\": %.3f%s}\n",
                    numOctaves, first.rows, first.cols, q.descriptors.size(), q.n_defined, second.rows, second.cols, t.descriptors.size(), t.n_defined,
                    nearest, m.matches.size(), exact, std::chrono::duration<double, std::milli>(t1 - t0).count(), extra.c_str());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Match: %s\n", e.what());
        return EXIT_FAILURE;
    }
}
