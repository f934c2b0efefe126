// Place recognition over a sequence of images, headless: the DoG pipeline of DoG.cpp on every frame - pyramid,
// initialKeypointDetection, filterKeypoints and SIFT per octave -, then a vocabulary sampled from the frames' own descriptors
// (vslam::sampleVocabulary), the visual word of every descriptor with a histogram per frame (vslam::assignWords), and the loop
// candidates of every frame among the frames at least min_gap before it (vslam::findLoopCandidates; include/vslam.h, "place
// recognition").  Prints one JSON line: the descriptor count of every frame and its candidates as [frame, score, norm].
//   usage: Place [--words K] [--gap G] [--candidates C] [--threshold NUM/DEN] [--octaves N] [--vocab-frames V] [--kmeans R] [--verify MIN_INLIERS]
//                (a.pgm b.pgm ... | WxH N)
//          (WxH N: frames 0 .. N-1 of the synthetic stream; defaults: K 256, gap 4, 3 candidates, threshold 1/5, 3 octaves;
//           --vocab-frames V: the vocabulary is sampled from the first V frames only, default all;
//           --kmeans R: the sampled vocabulary is trained for R rounds on those frames before the words are taken
//           (vslam::trainVocabulary; "vocabulary training"), and the line carries the report of every round as
//           [assigned, changed, empty, ran];
//           --verify MIN_INLIERS: every candidate is matched and tested against a RANSAC fundamental matrix (vslam::verifyLoops;
//           "loop verification", inlier share 2/5), and the line carries each frame's verified loop beside its candidates as
//           "loops": [train frame, slot, matches, inliers] ([-1, -1, 0, 0]: none) and every slot's "verified": [matches, inliers, best])
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "imgio.hpp"
#include "vslam_cxx.hpp"

using namespace cv;

int main(int argc, char** argv) {
    try {
        uint32_t K = 256;
        vslam_place_params params{4, 3, 1, 5, 0, 0};
        int numOctaves = 3;
        size_t vocabFrames = 0;
        uint32_t kmeansRounds = 0, verifyMinInliers = 0;
        while (argc > 2 && argv[1][0] == '-' && argv[1][1] == '-') {
            const std::string opt = argv[1];
            if (opt == "--words") K = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            else if (opt == "--gap") params.min_gap = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            else if (opt == "--candidates") params.max_candidates = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            else if (opt == "--octaves") numOctaves = std::atoi(argv[2]);
            else if (opt == "--vocab-frames") vocabFrames = (size_t)std::strtoul(argv[2], nullptr, 10);
            else if (opt == "--kmeans") kmeansRounds = (uint32_t)std::strtoul(argv[2], nullptr, 10);
            else if (opt == "--verify") {
                verifyMinInliers = (uint32_t)std::strtoul(argv[2], nullptr, 10);
                if (verifyMinInliers == 0) throw std::runtime_error("--verify takes MIN_INLIERS >= 1");
            }
            else if (opt == "--threshold") {
                if (std::sscanf(argv[2], "%u/%u", &params.num, &params.den) != 2) throw std::runtime_error("--threshold takes NUM/DEN");
            } else throw std::runtime_error("unknown option " + opt);
            argc -= 2, argv += 2;
        }
        std::vector<Mat> images;
        int w = 0, h = 0;
        if (argc == 3 && std::sscanf(argv[1], "%dx%d", &w, &h) == 2 && w > 0 && h > 0) {
            for (int f = 0; f < std::atoi(argv[2]); ++f) images.push_back(imgio::synthetic(h, w, f));
        } else {
            for (int a = 1; a < argc; ++a) images.push_back(imgio::read_pgm(argv[a]));
        }
        if (images.empty())
            throw std::runtime_error("usage: Place [--words K] [--gap G] [--candidates C] [--threshold NUM/DEN] [--octaves N] [--vocab-frames V] [--kmeans R] [--verify MIN_INLIERS] (a.pgm b.pgm ... | WxH N)");

        vslam::DescriptorSets frames(images.size());
        vslam::DefinedSets defined(images.size());
        std::vector<std::vector<SLAM::point>> points(images.size());
        for (size_t f = 0; f < images.size(); ++f) {
            GaussPyramid pyramid{images[f], numOctaves, 1.6};
            for (int octave = 0; octave < pyramid.getNumOctaves(); ++octave) {
                std::vector<SLAM::point> keypoints, reducedKeypoints;
                initialKeypointDetection(keypoints, pyramid, octave, 3);
                filterKeypoints(pyramid, octave, keypoints, reducedKeypoints);
                std::vector<unsigned char> def;
                SIFT(reducedKeypoints, frames[f], pyramid, octave, &def);
                points[f].insert(points[f].end(), reducedKeypoints.begin(), reducedKeypoints.end());
                defined[f].insert(defined[f].end(), def.begin(), def.end());
            }
        }
        if (vocabFrames == 0 || vocabFrames > frames.size()) vocabFrames = frames.size();
        const vslam::DescriptorSets vocabSets(frames.begin(), frames.begin() + vocabFrames);
        const vslam::DefinedSets vocabDefined(defined.begin(), defined.begin() + vocabFrames);
        vslam::Vocabulary vocabulary = vslam::sampleVocabulary(vocabSets, K, &vocabDefined);
        std::vector<vslam_kmeans_round> report;
        if (kmeansRounds) {
            vslam::TrainedVocabulary trained = vslam::trainVocabulary(vocabSets, vocabulary, kmeansRounds, &vocabDefined);
            vocabulary = std::move(trained.vocabulary);
            report = std::move(trained.report);
        }
        const vslam::Words words = vslam::assignWords(frames, vocabulary, &defined);
        const vslam::LoopCandidates loops = vslam::findLoopCandidates(words.hist, 0, words.hist, 0, K, params);

        size_t definedWords = 0;
        for (unsigned char d : vocabulary.defined) definedWords += d != 0;
        std::string s = "{\"frames\": " + std::to_string(frames.size()) + ", \"words\": " + std::to_string(K) + ", \"defined_words\": " + std::to_string(definedWords) +
                        ", \"min_gap\": " + std::to_string(params.min_gap) + ", \"threshold\": [" + std::to_string(params.num) + ", " + std::to_string(params.den) +
                        "], \"descriptors\": [";
        for (size_t f = 0; f < frames.size(); ++f) s += (f ? ", " : "") + std::to_string(frames[f].size());
        if (kmeansRounds) {
            s += "], \"kmeans\": [";
            for (size_t t = 0; t < report.size(); ++t)
                s += (t ? ", [" : "[") + std::to_string(report[t].assigned) + ", " + std::to_string(report[t].changed) + ", " + std::to_string(report[t].empty) + ", " +
                     std::to_string(report[t].ran) + "]";
        }
        s += "], \"assigned\": [";
        for (size_t f = 0; f < frames.size(); ++f) {
            size_t n = 0;
            for (int32_t wd : words.word[f]) n += wd >= 0;
            s += (f ? ", " : "") + std::to_string(n);
        }
        s += "], \"candidates\": [";
        for (size_t f = 0; f < frames.size(); ++f) {
            s += f ? ", [" : "[";
            for (size_t r = 0; r < loops.candidates[f].size(); ++r) {
                const vslam_place_cand& c = loops.candidates[f][r];
                s += (r ? ", [" : "[") + std::to_string(c.frame) + ", " + std::to_string(c.score) + ", " + std::to_string(c.norm) + "]";
            }
            s += "]";
        }
        if (verifyMinInliers) {
            const vslam::VerifiedLoops v = vslam::verifyLoops(frames, points, loops.candidates, params.max_candidates, 0, vslam_loop_params{verifyMinInliers, 2, 5, 0},
                                                              vslam_epipolar_params{512, 1, 4.0}, 0.8f, &defined);
            s += "], \"loops\": [";
            for (size_t f = 0; f < frames.size(); ++f) {
                const vslam_loop& l = v.loops[f];
                s += (f ? ", [" : "[") + std::to_string(l.train_set) + ", " + std::to_string(l.slot) + ", " + std::to_string(l.n_matches) + ", " +
                     std::to_string(l.n_inliers) + "]";
            }
            s += "], \"verified\": [";
            for (size_t f = 0; f < frames.size(); ++f) {
                s += f ? ", [" : "[";
                for (size_t r = 0; r < loops.candidates[f].size(); ++r) {
                    const vslam_epipolar& m = v.models[f * params.max_candidates + r];
                    s += (r ? ", [" : "[") + std::to_string(m.n_matches) + ", " + std::to_string(m.n_inliers) + ", " + std::to_string(m.best) + "]";
                }
                s += "]";
            }
        }
        std::printf("%s]}\n", s.c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Place: %s\n", e.what());
        return 1;
    }
    return 0;
}
