// Host driver of the C++ wrappers vslam::sampleVocabulary, vslam::assignWords and vslam::findLoopCandidates
// (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_place_cpu.py and tests/test_gpu_place.py.  Without an argument it makes the
// calls that the wrappers refuse before they need a GPU and checks sampleVocabulary (host code) on a tiny case, and prints "ok".
// With --valid it makes one small valid findLoopCandidates call and prints "status N": 0 with a GPU, the ABI's VSLAM_ERR_HIP
// without one.
//   driver words in.bin out.bin   in: uint64 n_sets, cap, K; counts u32 [n_sets]; desc f32 [n_sets][cap][128]; defined u8 [n_sets][cap]
//                                 out: the K words f32 [K][128], defined u8 [K]; per set its words i32 and dist2 f32 (count each); hist u32 [n_sets][K]
//   driver place in.bin out.bin   in: uint64 nq, nd, K, q_first, db_first, same; vslam_place_params; hist_q u32 [nq][K]; hist_db u32 [nd][K] unless same
//                                 out: per query frame uint32 count and its candidates; weights [K]; self_q [nq]; self_db [nd]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vslam_cxx.hpp"

template <typename T>
static bool get(std::FILE* f, T* p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}
template <typename T>
static void put(std::FILE* f, const T* p, size_t n) {
    if (n) std::fwrite(p, sizeof(T), n, f);
}

template <typename F>
static bool refused(F call) {
    try {
        call();
    } catch (const vslam::Error& e) {
        return e.status == VSLAM_ERR_INVALID;
    }
    return false;
}

int main(int argc, char** argv) {
    const vslam::DescriptorSets two(2, std::vector<std::vector<float>>(3, std::vector<float>(128, 0.5f)));
    const std::vector<uint32_t> hist(4 * 10, 1);
    if (argc < 2) {
        vslam::DescriptorSets shortRow = two;
        shortRow[1][2].resize(127);
        const vslam::DefinedSets d1(1, std::vector<unsigned char>(3, 1)), d2(2, std::vector<unsigned char>(2, 1));
        vslam::Vocabulary v = vslam::sampleVocabulary(two, 5), bad = v;
        bad.words.pop_back();
        const std::vector<uint32_t> odd(41, 1);
        bool ok = refused([&] { vslam::sampleVocabulary(shortRow, 5); }) && refused([&] { vslam::sampleVocabulary(two, 0); }) &&
                  refused([&] { vslam::sampleVocabulary(two, 65537); }) && refused([&] { vslam::sampleVocabulary(two, 5, &d1); }) &&
                  refused([&] { vslam::sampleVocabulary(vslam::DescriptorSets(), 5); }) && refused([&] { vslam::assignWords(shortRow, v); }) &&
                  refused([&] { vslam::assignWords(two, bad); }) && refused([&] { vslam::assignWords(two, v, &d2); }) &&
                  refused([&] { vslam::assignWords(two, vslam::Vocabulary()); }) && refused([&] { vslam::findLoopCandidates(odd, 0, hist, 0, 10); }) &&
                  refused([&] { vslam::findLoopCandidates(hist, 0, hist, 0, 0); }) &&
                  refused([&] { vslam::findLoopCandidates(hist, 0, hist, 0, 10, vslam_place_params{4, 9, 1, 5, 0, 0}); });
        // the sampling rule on the host: 2 sets of 3 rows, 5 words -> sets 0 1 0 1 0, rows (k / 2) * 2654435761 mod 2^32 mod 3 = 0 0 1 1 1
        vslam::DescriptorSets marked = two;
        for (int s = 0; s < 2; ++s)
            for (int r = 0; r < 3; ++r) marked[s][r][0] = (float)(10 * s + r);
        vslam::DefinedSets holes(2, std::vector<unsigned char>(3, 1));
        holes[1][1] = 0;
        v = vslam::sampleVocabulary(marked, 5, &holes);
        const float want[5] = {0.0f, 10.0f, 1.0f, 0.0f, 1.0f};
        const unsigned char wdef[5] = {1, 1, 1, 0, 1};
        for (int k = 0; k < 5; ++k) ok = ok && v.words[128 * k] == want[k] && v.defined[k] == wdef[k] && v.words[128 * k + 1] == (wdef[k] ? 0.5f : 0.0f);
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    if (argc == 2 && std::strcmp(argv[1], "--valid") == 0) {
        int status = VSLAM_OK;
        try {
            const vslam::LoopCandidates r = vslam::findLoopCandidates(hist, 0, hist, 0, 10, vslam_place_params{1, 2, 0, 1, 0, 0});
            if (r.candidates.size() != 4 || r.weights.size() != 10 || r.candidates[3].size() != 2 || r.candidates[3][0].frame != 0) status = 1;
        } catch (const vslam::Error& e) {
            status = e.status;
        }
        std::printf("status %d\n", status);
        return 0;
    }
    if (argc != 4) return 2;
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    try {
        if (std::strcmp(argv[1], "words") == 0) {
            uint64_t n[3];
            if (!get(f, n, 3)) return 2;
            const size_t sets = n[0], cap = n[1];
            const uint32_t K = (uint32_t)n[2];
            std::vector<uint32_t> counts(sets);
            std::vector<float> desc(sets * cap * 128);
            std::vector<unsigned char> def(sets * cap);
            if (!get(f, counts.data(), sets) || !get(f, desc.data(), desc.size()) || !get(f, def.data(), def.size())) return 2;
            std::fclose(f);
            vslam::DescriptorSets frames(sets);
            vslam::DefinedSets defined(sets);
            for (size_t s = 0; s < sets; ++s)
                for (size_t r = 0; r < counts[s]; ++r) {
                    frames[s].emplace_back(desc.begin() + (s * cap + r) * 128, desc.begin() + (s * cap + r + 1) * 128);
                    defined[s].push_back(def[s * cap + r]);
                }
            const vslam::Vocabulary v = vslam::sampleVocabulary(frames, K, &defined);
            const vslam::Words w = vslam::assignWords(frames, v, &defined);
            std::FILE* o = std::fopen(argv[3], "wb");
            if (!o) return 2;
            put(o, v.words.data(), v.words.size());
            put(o, v.defined.data(), v.defined.size());
            for (size_t s = 0; s < sets; ++s) put(o, w.word[s].data(), w.word[s].size()), put(o, w.dist2[s].data(), w.dist2[s].size());
            put(o, w.hist.data(), w.hist.size());
            std::fclose(o);
        } else {
            uint64_t n[6];
            vslam_place_params P{};
            if (!get(f, n, 6) || !get(f, &P, 1)) return 2;
            std::vector<uint32_t> hq(n[0] * n[2]), hd(n[5] ? 0 : n[1] * n[2]);
            if (!get(f, hq.data(), hq.size()) || !get(f, hd.data(), hd.size())) return 2;
            std::fclose(f);
            const vslam::LoopCandidates r = vslam::findLoopCandidates(hq, (uint32_t)n[3], n[5] ? hq : hd, (uint32_t)n[4], (uint32_t)n[2], P);
            std::FILE* o = std::fopen(argv[3], "wb");
            if (!o) return 2;
            for (const auto& c : r.candidates) {
                const uint32_t k = (uint32_t)c.size();
                put(o, &k, 1);
                put(o, c.data(), c.size());
            }
            put(o, r.weights.data(), r.weights.size());
            put(o, r.selfQuery.data(), r.selfQuery.size());
            put(o, r.selfDb.data(), r.selfDb.size());
            std::fclose(o);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "place_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
