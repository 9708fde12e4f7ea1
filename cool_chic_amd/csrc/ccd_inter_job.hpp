// ccd_inter_job.hpp - the host side of the unit kernels of P / B frames (InterUnitJob, ccd_device.hpp; DESIGN.md sections 4.15, 4.16,
// 4.19), shared by ccd_dsens_api.cpp and ccd_iscore_api.cpp: the geometry of a job, the workgroups that cover a frame, the device
// blocks that hold its references and planes, and the launch tables.  Host only, no HIP calls: tools/iscore_host_check.cpp runs it
// under the sanitizers.
#pragma once
#include <cstdint>
#include <vector>

#include "ccd_host.hpp"

namespace ccd {

// What the geometry of a job depends on: the frame's size and sample format, and its frame header.
struct InterFrameDesc {
    int32_t h, w, bitdepth, frame_data_type;
    int32_t frame_type, warp_filter_size;
    const int32_t* global_flow;  // [4]: (x, y) per reference; a P frame's second pair is not read
};

// workgroups of 64 x 4 units (a unit: one luma sample or, 4:2:0, one quad) that cover a frame
inline int32_t inter_tiles_x(int w, int chroma_shift) { return ((w >> chroma_shift) + 63) / 64; }
inline uint32_t inter_blocks(int h, int w, int chroma_shift) {
    return static_cast<uint32_t>(inter_tiles_x(w, chroma_shift)) * static_cast<uint32_t>(((h >> chroma_shift) + 3) / 4);
}

// Everything of a job but its pointers and its mode.
inline void fill_inter_geometry(InterUnitJob& J, const InterFrameDesc& f) {
    J.frame_type = f.frame_type;
    J.H = f.h; J.W = f.w;
    J.n_taps = f.warp_filter_size;
    for (int i = 0; i < 4; ++i) J.gflow[i] = (i < 2 || f.frame_type == 2) ? f.global_flow[i] : 0;
    J.chroma_shift = f.frame_data_type == 1 ? 1 : 0;
    J.wide = f.bitdepth > 8;
    J.tiles_x = inter_tiles_x(f.w, J.chroma_shift);
    J.maxv = static_cast<float>((1 << f.bitdepth) - 1);
}

// Sizes of what a frame takes in a device block, each a multiple of 256 bytes: the frame as f32 4:4:4 (a reference as the warp
// reads it, or warped), a luma plane, a chroma plane.
struct PlaneLayout { size_t f32_3, luma, chroma; size_t planes() const { return luma + 2 * chroma; } };
inline PlaneLayout plane_layout(int h, int w, int bitdepth, int frame_data_type) {
    const size_t hw = static_cast<size_t>(h) * w, sample = bitdepth > 8 ? 2 : 1;
    const size_t chw = frame_data_type == 1 ? static_cast<size_t>(h / 2) * (w / 2) : hw;
    return PlaneLayout{align256(3 * hw * sizeof(float)), align256(hw * sample), align256(chw * sample)};
}
// Consecutive sub-blocks of a block.
struct BlockCursor {
    char* at;
    explicit BlockCursor(const Block& b) : at(b.as<char>()) {}
    float* f32(const PlaneLayout& L) { return static_cast<float*>(take(L.f32_3)); }
    void planes(const PlaneLayout& L, void** pl) { pl[0] = take(L.luma); pl[1] = take(L.chroma); pl[2] = take(L.chroma); }
    void* take(size_t bytes) { char* p = at; at += bytes; return p; }
};

// One launch of a unit kernel: offsets into the tables block.
struct JobLaunch { size_t jobs = 0, prefix = 0; int n_jobs = 0; uint32_t n_blocks = 0; };
// Appends the jobs and the prefix table of their workgroups.  CCD_ERR_UNSUPPORTED when the launch would need 2^31 workgroups or more.
template <typename Job>
int put_job_launch(TableImage& img, const std::vector<Job>& jobs, JobLaunch& L) {
    std::vector<uint32_t> prefix(jobs.size() + 1, 0);
    uint64_t blocks = 0;
    for (size_t i = 0; i < jobs.size(); ++i) {
        const InterUnitJob& J = unit_job(jobs[i]);
        blocks += inter_blocks(J.H, J.W, J.chroma_shift);
        if (blocks > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
        prefix[i + 1] = static_cast<uint32_t>(blocks);
    }
    L.n_jobs = static_cast<int>(jobs.size()); L.n_blocks = static_cast<uint32_t>(blocks);
    L.jobs = img.put(jobs); L.prefix = img.put(prefix);
    return CCD_OK;
}

}  // namespace ccd
