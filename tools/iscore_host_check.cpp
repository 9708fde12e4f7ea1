// iscore_host_check.cpp - the job and partial planning of a ccd_iscore run (cool_chic_amd/csrc/ccd_iscore_plan.hpp, DESIGN.md section
// 4.19) as a stand-alone CPU program: meant to be built with -fsanitize=address,undefined, host code only (the header has no HIP
// in it, no device code is compiled, no device is needed, and the sanitizers are never asked of an offload target):
//
//   hipcc --offload-host-only -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/iscore_host_check.cpp -o iscore_host_check
//   ./iscore_host_check
//
// Seeded frames of every size class (one unit, one-pixel sides, ragged tiles, 1080p, the format's 16 383 limit) with random items:
// every job's workgroups are those of its tiles, the partial ranges tile [0, total) without gap or overlap in result order, the
// launches' workgroup counts add up, the classes follow (item, sinc-8), and the refusals (an item of no frame, 2^31 workgroups).
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../cool_chic_amd/csrc/ccd_iscore_plan.hpp"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using namespace ccd;

int main() {
    std::mt19937 rng(419);
    const int sides[] = {1, 2, 3, 4, 5, 63, 64, 65, 67, 70, 127, 128, 130, 131, 1080, 1920, 16383};
    const int n_sides = static_cast<int>(sizeof(sides) / sizeof(sides[0]));
    long long jobs = 0;
    for (int round = 0; round < 400; ++round) {
        std::vector<IScoreGeo> frames(rng() % 6);
        for (auto& g : frames) {
            g.chroma_shift = static_cast<int32_t>(rng() % 2);
            g.h = sides[rng() % n_sides]; g.w = sides[rng() % n_sides];
            if (g.chroma_shift) { g.h += g.h & 1; g.w += g.w & 1; }
            g.sinc8 = static_cast<int32_t>(rng() % 2);
        }
        std::vector<int> item_frame(frames.empty() ? 0 : rng() % 80);
        for (auto& f : item_frame) f = static_cast<int>(rng() % frames.size());
        std::vector<IScoreSlot> plan;
        uint32_t cls[kIScoreClasses], total = 7;
        CHECK(iscore_plan(frames, item_frame, plan, cls, &total) == CCD_OK);
        CHECK(plan.size() == frames.size() + item_frame.size());
        uint64_t at = 0, per[kIScoreClasses] = {0, 0, 0, 0};
        for (size_t r = 0; r < plan.size(); ++r) {
            const bool item = r >= frames.size();
            const IScoreGeo& g = frames[item ? static_cast<size_t>(item_frame[r - frames.size()]) : r];
            const int uw = g.w >> g.chroma_shift, uh = g.h >> g.chroma_shift;
            CHECK(plan[r].n_blocks == static_cast<uint32_t>((uw + 63) / 64) * static_cast<uint32_t>((uh + 3) / 4) && plan[r].n_blocks >= 1);
            CHECK(plan[r].part_first == at);
            CHECK(plan[r].cls == (item ? 2 : 0) + (g.sinc8 ? 1 : 0));
            at += plan[r].n_blocks;
            per[plan[r].cls] += plan[r].n_blocks;
            ++jobs;
        }
        CHECK(total == at);
        for (int c = 0; c < kIScoreClasses; ++c) CHECK(cls[c] == per[c]);
        if (!frames.empty()) {  // an item of no frame
            std::vector<int> bad = item_frame;
            bad.push_back(static_cast<int>(frames.size()));
            CHECK(iscore_plan(frames, bad, plan, cls, &total) == CCD_ERR_ARG);
            bad.back() = -1;
            CHECK(iscore_plan(frames, bad, plan, cls, &total) == CCD_ERR_ARG);
        }
    }
    // 2^31 workgroups: a 16 383 x 16 383 frame has 256 x 4 096 = 2^20 of them, so 2 047 items still fit beside the base pair
    std::vector<IScoreGeo> big(1, IScoreGeo{16383, 16383, 0, 1});
    std::vector<IScoreSlot> plan;
    uint32_t cls[kIScoreClasses], total = 0;
    CHECK(iscore_blocks(big[0]) == (1u << 20));
    CHECK(iscore_plan(big, std::vector<int>(2046, 0), plan, cls, &total) == CCD_OK && total == 2047u << 20);
    CHECK(iscore_plan(big, std::vector<int>(2047, 0), plan, cls, &total) == CCD_ERR_UNSUPPORTED);
    std::printf("iscore_host_check: %lld jobs planned, all checks passed\n", jobs);
    return 0;
}
