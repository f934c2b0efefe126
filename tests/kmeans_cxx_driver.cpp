// Host driver of the C++ wrapper vslam::trainVocabulary (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_kmeans_cpu.py and
// tests/test_gpu_kmeans.py.  Without an argument it makes the calls that the wrapper refuses before it needs a GPU and prints
// "ok".  With --valid it makes one small valid call and prints "status N": 0 with a GPU, the ABI's VSLAM_ERR_HIP without one.
//   driver train in.bin out.bin   in: uint64 n_sets, cap, K, rounds; counts u32 [n_sets]; desc f32 [n_sets][cap][128]; defined u8 [n_sets][cap];
//                                     vocab f32 [K][128]; vocab_defined u8 [K]
//                                 out: the trained words f32 [K][128]; sizes u32 [K]; report [rounds]
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
    vslam::DescriptorSets two(2, std::vector<std::vector<float>>(3, std::vector<float>(128, 0.5f)));
    two[1][2][7] = 0.25f;
    if (argc < 2) {
        vslam::DescriptorSets shortRow = two;
        shortRow[1][2].resize(127);
        const vslam::DefinedSets d1(1, std::vector<unsigned char>(3, 1));
        const vslam::Vocabulary v = vslam::sampleVocabulary(two, 5);
        vslam::Vocabulary bad = v;
        bad.words.pop_back();
        const bool ok = refused([&] { vslam::trainVocabulary(shortRow, v, 2); }) && refused([&] { vslam::trainVocabulary(two, bad, 2); }) &&
                        refused([&] { vslam::trainVocabulary(two, vslam::Vocabulary(), 2); }) && refused([&] { vslam::trainVocabulary(two, v, 0); }) &&
                        refused([&] { vslam::trainVocabulary(two, v, 65); }) && refused([&] { vslam::trainVocabulary(two, v, 2, &d1); });
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    if (argc == 2 && std::strcmp(argv[1], "--valid") == 0) {
        int status = VSLAM_OK;
        try {
            const vslam::TrainedVocabulary r = vslam::trainVocabulary(two, vslam::sampleVocabulary(two, 2), 3);
            if (r.vocabulary.size() != 2 || r.sizes.size() != 2 || r.report.size() != 3 || r.report[0].ran != 1 || r.report[0].changed != 6) status = 1;
        } catch (const vslam::Error& e) {
            status = e.status;
        }
        std::printf("status %d\n", status);
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "train") != 0) return 2;
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    try {
        uint64_t n[4];
        if (!get(f, n, 4)) return 2;
        const size_t sets = n[0], cap = n[1], K = n[2];
        std::vector<uint32_t> counts(sets);
        std::vector<float> desc(sets * cap * 128);
        std::vector<unsigned char> def(sets * cap);
        vslam::Vocabulary v;
        v.words.resize(K * 128), v.defined.resize(K);
        if (!get(f, counts.data(), sets) || !get(f, desc.data(), desc.size()) || !get(f, def.data(), def.size()) || !get(f, v.words.data(), v.words.size()) ||
            !get(f, v.defined.data(), K))
            return 2;
        std::fclose(f);
        vslam::DescriptorSets frames(sets);
        vslam::DefinedSets defined(sets);
        for (size_t s = 0; s < sets; ++s)
            for (size_t r = 0; r < counts[s]; ++r) {
                frames[s].emplace_back(desc.begin() + (s * cap + r) * 128, desc.begin() + (s * cap + r + 1) * 128);
                defined[s].push_back(def[s * cap + r]);
            }
        const vslam::TrainedVocabulary t = vslam::trainVocabulary(frames, v, (uint32_t)n[3], &defined);
        std::FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 2;
        put(o, t.vocabulary.words.data(), t.vocabulary.words.size());
        put(o, t.sizes.data(), t.sizes.size());
        put(o, t.report.data(), t.report.size());
        std::fclose(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "kmeans_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
