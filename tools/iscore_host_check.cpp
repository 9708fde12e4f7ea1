// iscore_host_check.cpp - the job and partial planning of a ccd_iscore run (cool_chic_amd/csrc/ccd_iscore_plan.hpp, DESIGN.md section
// 4.19) and the host side of the unit kernels of P / B frames (ccd_inter_job.hpp: job geometry, workgroup counts, launch tables,
// block layout) as a stand-alone CPU program: meant to be built with -fsanitize=address,undefined, host code only (the headers
// make no HIP call, no device code is compiled, no device is needed, and the sanitizers are never asked of an offload target):
//
//   hipcc --offload-host-only -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/iscore_host_check.cpp -o iscore_host_check
//   ./iscore_host_check
//
// Seeded frames of every size class (one unit, one-pixel sides, ragged tiles, 1080p, the format's 16 383 limit) with random items:
// every job's workgroups are those of its tiles, the partial ranges tile [0, total) without gap or overlap in result order, the
// launches' workgroup counts add up, the classes follow (item, sinc-8), and the refusals (an item of no frame, 2^31 workgroups).
// ccd_inter_job.hpp over the sides 1, 2, 63, 64, 65, 16 383, the three formats (4:2:0 with even sides), 8 / 10 / 16 bits, P and B:
// fill_inter_geometry against the expressions it replaced, written out here; inter_blocks against a count of the tiles that hold a
// unit; put_job_launch's prefix sums and its 2^31 refusal; BlockCursor's sub-blocks aligned to 256 bytes, disjoint, inside the block.
// Reference items: every item of a round also is, at random, a role item or a reference item with reference
// 0, 1 or both replaced; iscore_plan_conv gives one conversion job per replaced reference, in item order, reference 0 first, whose
// workgroups are the PIXEL tiles of the frame (whatever its format) and tile [0, total) without gap or overlap; iscore_ref_mode is
// checked against the table of the unit walk's modes; the refusals: an item of no frame, a refs outside 0..3, 2^31 workgroups.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>

#include "../cool_chic_amd/csrc/ccd_inter_job.hpp"
#include "../cool_chic_amd/csrc/ccd_iscore_plan.hpp"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using namespace ccd;

// workgroups of a frame by enumeration: the 64 x 4 tiles of the unit raster that hold at least one unit
static uint32_t blocks_by_count(int h, int w, int cs) {
    const int uh = h >> cs, uw = w >> cs;
    uint32_t n = 0;
    for (int ty = 0; ty * 4 < uh; ++ty)
        for (int tx = 0; tx * 64 < uw; ++tx) ++n;
    return n;
}

static long long check_inter_job() {
    const int sides[] = {1, 2, 63, 64, 65, 16383}, depths[] = {8, 10, 16};
    const int32_t flow[4] = {3, -5, -7, 11};
    long long n = 0;
    std::vector<InterUnitJob> jobs;
    for (int h : sides) for (int w : sides) for (int fdt = 0; fdt < 3; ++fdt) for (int bd : depths) for (int ft = 1; ft <= 2; ++ft) {
        if (fdt == 1 && ((h | w) & 1)) continue;  // 4:2:0: even sides only
        const int taps = (n % 2) ? 8 : 4;
        InterUnitJob J;
        std::memset(&J, 0x5a, sizeof(J));
        const InterUnitJob before = J;
        fill_inter_geometry(J, InterFrameDesc{h, w, bd, fdt, ft, taps, flow});
        // the expressions of make_inter_job / make_dep_recon / make_job before the filler
        const bool two = ft == 2;
        const int cs = fdt == 1 ? 1 : 0;
        CHECK(J.frame_type == ft && J.H == h && J.W == w && J.n_taps == taps);
        for (int i = 0; i < 4; ++i) CHECK(J.gflow[i] == ((i < 2 || two) ? flow[i] : 0));
        CHECK(J.chroma_shift == cs && J.wide == (bd > 8) && J.tiles_x == ((w >> cs) + 63) / 64);
        CHECK(J.maxv == static_cast<float>((1 << bd) - 1));
        // pointers and mode are the caller's
        CHECK(J.residue == before.residue && J.motion == before.motion && J.ref0 == before.ref0 && J.ref1 == before.ref1 && J.w0 == before.w0 &&
              J.w1 == before.w1 && J.plane[0] == before.plane[0] && J.plane[1] == before.plane[1] && J.plane[2] == before.plane[2] && J.mode == before.mode);
        CHECK(inter_tiles_x(w, cs) == J.tiles_x && inter_blocks(h, w, cs) == blocks_by_count(h, w, cs) && inter_blocks(h, w, cs) >= 1);
        jobs.push_back(J);
        // the layout: sizes that hold the planes, and the sub-blocks a candidate of K probe slots carves (ccd_dsens_add_inter)
        const PlaneLayout lay = plane_layout(h, w, bd, fdt);
        const size_t hw = static_cast<size_t>(h) * w, chw = cs ? static_cast<size_t>(h / 2) * (w / 2) : hw, sample = bd > 8 ? 2 : 1;
        CHECK(lay.f32_3 % 256 == 0 && lay.luma % 256 == 0 && lay.chroma % 256 == 0);
        CHECK(lay.f32_3 >= 12 * hw && lay.f32_3 < 12 * hw + 256 && lay.luma >= hw * sample && lay.luma < hw * sample + 256);
        CHECK(lay.chroma >= chw * sample && lay.chroma < chw * sample + 256 && lay.planes() == lay.luma + 2 * lay.chroma);
        if (hw <= 65 * 65) {  // (the cursor only adds: nothing of the block is touched, small blocks say it all)
            const int K = 3, n_refs = two ? 2 : 1;
            const size_t total = 2 * n_refs * lay.f32_3 + (K + 1) * lay.planes();
            Block blk;  // (host memory behind a Block: no pool, no device)
            blk.p = std::aligned_alloc(256, total);
            CHECK(blk.p != nullptr);
            BlockCursor cur(blk);
            std::vector<std::pair<char*, size_t>> subs;
            for (int r = 0; r < 2 * n_refs; ++r) subs.emplace_back(reinterpret_cast<char*>(cur.f32(lay)), 12 * hw);
            for (int k = 0; k <= K; ++k) {
                void* pl[3];
                cur.planes(lay, pl);
                for (int p = 0; p < 3; ++p) subs.emplace_back(static_cast<char*>(pl[p]), (p ? chw : hw) * sample);
            }
            char* end = static_cast<char*>(blk.p);
            for (const auto& sb : subs) {  // in order, aligned, each behind the one before, all inside the block
                CHECK(reinterpret_cast<uintptr_t>(sb.first) % 256 == 0 && sb.first >= end);
                std::memset(sb.first, 0, sb.second);  // (under the address sanitizer: inside the allocation)
                end = sb.first + sb.second;
            }
            CHECK(cur.at == static_cast<char*>(blk.p) + total && end <= cur.at);
            std::free(blk.p);
        }
        ++n;
    }
    // launch tables: the prefix is the running sum of the jobs' workgroups, a job inside a larger struct counts by its frame
    TableImage img;
    JobLaunch L;
    img.put("x", 1);  // (so that the tables do not start at 0)
    CHECK(put_job_launch(img, jobs, L) == CCD_OK && L.n_jobs == static_cast<int>(jobs.size()));
    CHECK(L.jobs % 256 == 0 && L.prefix % 256 == 0 && L.jobs >= 256 && L.prefix >= L.jobs + jobs.size() * sizeof(InterUnitJob));
    CHECK(img.bytes.size() == L.prefix + (jobs.size() + 1) * sizeof(uint32_t));
    uint64_t sum = 0;
    for (size_t i = 0; i <= jobs.size(); ++i) {
        uint32_t got;
        std::memcpy(&got, img.bytes.data() + L.prefix + i * sizeof(uint32_t), sizeof(got));
        CHECK(got == sum);
        if (i < jobs.size()) {
            CHECK(std::memcmp(img.bytes.data() + L.jobs + i * sizeof(InterUnitJob), &jobs[i], sizeof(InterUnitJob)) == 0);
            sum += blocks_by_count(jobs[i].H, jobs[i].W, jobs[i].chroma_shift);
        }
    }
    CHECK(L.n_blocks == sum);
    std::vector<InterScoreJob> none;
    CHECK(put_job_launch(img, none, L) == CCD_OK && L.n_jobs == 0 && L.n_blocks == 0);
    // 2^31 workgroups: 2^20 per 16 383 x 16 383 frame, so 2 047 jobs fit and 2 048 do not
    InterScoreJob big;
    std::memset(&big, 0, sizeof(big));
    fill_inter_geometry(big.recon, InterFrameDesc{16383, 16383, 8, 0, 1, 8, flow});
    CHECK(put_job_launch(img, std::vector<InterScoreJob>(2047, big), L) == CCD_OK && L.n_blocks == 2047u << 20);
    CHECK(put_job_launch(img, std::vector<InterScoreJob>(2048, big), L) == CCD_ERR_UNSUPPORTED);
    DsensDepJob dep;
    std::memset(&dep, 0, sizeof(dep));
    dep.recon = big.recon;
    CHECK(put_job_launch(img, std::vector<DsensDepJob>(2, dep), L) == CCD_OK && L.n_blocks == 2u << 20);
    return n;
}

int main() {
    const long long filled = check_inter_job();
    std::mt19937 rng(419);
    const int sides[] = {1, 2, 3, 4, 5, 63, 64, 65, 67, 70, 127, 128, 130, 131, 1080, 1920, 16383};
    const int n_sides = static_cast<int>(sizeof(sides) / sizeof(sides[0]));
    long long jobs = 0, conv_jobs = 0;
    // the unit walk's mode of a reference item: P frames and "both" warp everything (2); a B frame's single replaced reference: 3 / 4
    CHECK(iscore_ref_mode(1, 1) == 2 && iscore_ref_mode(2, 3) == 2 && iscore_ref_mode(2, 1) == 3 && iscore_ref_mode(2, 2) == 4);
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
        // the same items as reference items
        std::vector<IScoreItemGeo> items(item_frame.size());
        for (size_t i = 0; i < items.size(); ++i) items[i] = IScoreItemGeo{item_frame[i], static_cast<int32_t>(rng() % 4)};
        std::vector<IScoreConv> conv;
        uint32_t conv_total = 7;
        CHECK(iscore_plan_conv(frames, items, conv, &conv_total) == CCD_OK);
        size_t k = 0;
        uint64_t conv_at = 0;
        for (size_t i = 0; i < items.size(); ++i) {
            const IScoreGeo& g = frames[static_cast<size_t>(items[i].frame)];
            for (int which = 0; which < 2; ++which) {
                if (!(items[i].refs >> which & 1)) continue;
                CHECK(k < conv.size() && conv[k].item == static_cast<int32_t>(i) && conv[k].which == which);
                CHECK(conv[k].n_blocks == blocks_by_count(g.h, g.w, 0) && conv[k].n_blocks >= 1 && conv[k].block_first == conv_at);
                conv_at += conv[k].n_blocks;
                ++k;
                ++conv_jobs;
            }
        }
        CHECK(k == conv.size() && conv_total == conv_at);
        if (!items.empty()) {
            std::vector<IScoreItemGeo> bad = items;
            bad.back().refs = 4;
            CHECK(iscore_plan_conv(frames, bad, conv, &conv_total) == CCD_ERR_ARG);
            bad.back() = IScoreItemGeo{static_cast<int32_t>(frames.size()), 1};
            CHECK(iscore_plan_conv(frames, bad, conv, &conv_total) == CCD_ERR_ARG);
            bad.back().frame = -1;
            CHECK(iscore_plan_conv(frames, bad, conv, &conv_total) == CCD_ERR_ARG);
        }
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
    CHECK(inter_blocks(big[0].h, big[0].w, big[0].chroma_shift) == (1u << 20));
    CHECK(iscore_plan(big, std::vector<int>(2046, 0), plan, cls, &total) == CCD_OK && total == 2047u << 20);
    CHECK(iscore_plan(big, std::vector<int>(2047, 0), plan, cls, &total) == CCD_ERR_UNSUPPORTED);
    // conversion workgroups: 2^20 per 16 383 x 16 383 reference, two per item with both replaced
    std::vector<IScoreConv> conv;
    CHECK(iscore_plan_conv(big, std::vector<IScoreItemGeo>(1023, IScoreItemGeo{0, 3}), conv, &total) == CCD_OK && total == 2046u << 20 && conv.size() == 2046);
    CHECK(iscore_plan_conv(big, std::vector<IScoreItemGeo>(1024, IScoreItemGeo{0, 3}), conv, &total) == CCD_ERR_UNSUPPORTED);
    CHECK(iscore_plan_conv(big, std::vector<IScoreItemGeo>(5, IScoreItemGeo{0, 0}), conv, &total) == CCD_OK && total == 0 && conv.empty());
    static_assert(sizeof(PlanesConvJob) == 56 && sizeof(InterUnitJob) == 128, "table entries");
    std::printf("iscore_host_check: %lld jobs planned, %lld conversion jobs planned, %lld job geometries filled, all checks passed\n", jobs, conv_jobs, filled);
    return 0;
}
