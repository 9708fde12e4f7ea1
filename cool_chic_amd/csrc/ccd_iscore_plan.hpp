// ccd_iscore_plan.hpp - which launch every job of a ccd_iscore run belongs to and where its workgroup partials sit (host only, no
// HIP calls: tools/iscore_host_check.cpp runs it under the sanitizers).  Results are numbered frames first (the base pairs), then items.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/ccd.h"
#include "ccd_inter_job.hpp"

namespace ccd {

constexpr int kIScoreMaxSide = 16383;       // the format's 14-bit img_size
constexpr int kIScoreMaxItems = 1 << 20;
// launches of a run, in order: base pairs with a run-time tap count, base pairs sinc-8, items run-time, items sinc-8
constexpr int kIScoreClasses = 4;

struct IScoreGeo { int32_t h, w, chroma_shift, sinc8; };
struct IScoreSlot { int32_t cls; uint32_t n_blocks, part_first; };

// out[r] for every result, the workgroups of every launch and of the whole run.  CCD_ERR_ARG for an item of no frame,
// CCD_ERR_UNSUPPORTED when a run would need 2^31 workgroups or more.
inline int iscore_plan(const std::vector<IScoreGeo>& frames, const std::vector<int>& item_frame, std::vector<IScoreSlot>& out,
                       uint32_t class_blocks[kIScoreClasses], uint32_t* total_blocks) {
    const size_t n_frames = frames.size();
    out.assign(n_frames + item_frame.size(), IScoreSlot{});
    uint64_t total = 0, per_class[kIScoreClasses] = {0, 0, 0, 0};
    for (size_t r = 0; r < out.size(); ++r) {
        const bool item = r >= n_frames;
        if (item && (item_frame[r - n_frames] < 0 || static_cast<size_t>(item_frame[r - n_frames]) >= n_frames)) return CCD_ERR_ARG;
        const IScoreGeo& g = frames[item ? static_cast<size_t>(item_frame[r - n_frames]) : r];
        IScoreSlot& s = out[r];
        s.cls = (item ? 2 : 0) + (g.sinc8 ? 1 : 0);
        s.n_blocks = inter_blocks(g.h, g.w, g.chroma_shift);
        s.part_first = static_cast<uint32_t>(total);
        total += s.n_blocks;
        per_class[s.cls] += s.n_blocks;
        if (total > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
    }
    for (int c = 0; c < kIScoreClasses; ++c) class_blocks[c] = static_cast<uint32_t>(per_class[c]);
    *total_blocks = static_cast<uint32_t>(total);
    return CCD_OK;
}

}  // namespace ccd
