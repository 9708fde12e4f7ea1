// ccd_quality.hpp - tables shared between ccd_quality_* (ccd_quality_api.cpp) and the kernels of ccd_quality.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace ccd {

constexpr int kQScales = 5;          // MS-SSIM scales
constexpr int kQWin = 11;            // taps of the Gaussian window
constexpr int kQTile = 32;           // an MS-SSIM tile gives kQTile x kQTile window positions ...
constexpr int kQStage = kQTile + kQWin - 1;  // ... from kQStage x kQStage staged samples
constexpr int kQMinSide = 16 * kQWin;        // shorter side a plane needs for five scales (176)
constexpr int kQSseBytes = 16384;    // bytes of each of the two pictures one squared-error tile reads
constexpr int kQMaxDim = 16383;

// One plane of one item.  Scale j of the plane is (h >> j) x (w >> j); scale 0 is read from dec / src, scales 1..4 from
// pool[.][j - 1], which hold the SUM of the 4^j samples under each pixel as float32: at most 65535 * 256 < 2^24, so the
// pooled pictures are exact and the division by 4^j is folded into the normalisation of the moments.
struct QualityPlane {
    const void* dec;
    const void* src;
    float* pool[2][kQScales - 1];
    int32_t h, w;
    int32_t wide;        // samples are uint16 (bit depth above 8)
    int32_t n_scales;    // 5, or 0: no MS-SSIM tiles for this plane
    double inv_maxv;     // 1 / (2^bitdepth - 1)
};

struct QualityOut {      // per plane, written by the final kernel
    uint64_t sse;
    double cs_sum[kQScales], ssim_sum[kQScales];
};

struct QualityBatch {    // kernel argument
    const QualityPlane* planes;
    int32_t n_planes;
    const uint32_t* sse_prefix;  // [n_planes + 1]: first squared-error tile of each plane
    const uint32_t* ms_prefix;   // [kQScales][n_planes + 1]: first tile of each plane in the launch of a scale
    uint32_t scale_first[kQScales + 1];  // first slot of a scale's launch in ms_part
    uint64_t* sse_part;          // [squared-error tiles]
    double* ms_part;             // [MS-SSIM tiles of all scales][2]: sums of cs and ssim over the tile
    QualityOut* out;             // [n_planes]
    double g[kQWin];             // the window, normalised to sum 1
};

hipError_t launch_quality(const QualityBatch& B, uint32_t n_sse_tiles, hipStream_t stream);  // ccd_quality.hip

}  // namespace ccd
