// ccd_ingest.hip - latent grids that were GIVEN as device pointers (ccd_batch_add_latents, on_device = 1) go where the entropy
// kernel would have left them, and are checked against the coder's alphabet on the way (gfx950).
//
// One launch per run covers every grid of every such slot.  A grid is a segment {src, dst, n, slot}; a 64-lane workgroup
// copies kIngestChunk bytes of one segment and finds it in a prefix table of workgroups (as the PNG packer's blocks and the
// quality meter's tiles do).  16-byte loads and stores where source and destination are aligned alike, bytes at the ragged
// ends and for a source that is not: grids like 18 x 65 or 3 x 9 at odd offsets are ordinary input.
//
// Status.  A byte outside [-64, 63] makes its lane store CCD_ERR_VALUE into the slot's status word: every writer stores the
// same value, so plain stores do.  The word has to read CCD_OK before the launch, on every run, and a store of CCD_OK from
// INSIDE the launch would race with the violations other workgroups of the same slot report.  So a slot alternates between
// two words: run k reports into word `word` (0 or kIngestWordB) and the first lane of the slot's first segment
// unconditionally stores CCD_OK into the OTHER word, the one run k + 1 reports into.  Each word is written by one kind of
// store per launch; launches of a batch are ordered by their stream.  ccd_batch_wait reads the word of the last run.
#include <hip/hip_runtime.h>

#include "ccd_kernels.hpp"

namespace ccd {
namespace {
// A byte is inside [-64, 63] exactly when its two top bits are equal; per byte of a dword: bit 7 of x ^ (x << 1).
__device__ __forceinline__ uint32_t outside4(uint32_t x) { return (x ^ (x << 1)) & 0x80808080u; }

__global__ __launch_bounds__(64) void latent_ingest_kernel(const IngestSeg* __restrict__ segs, const uint32_t* __restrict__ prefix, int n_segs,
                                                           int32_t* __restrict__ status_all, int word) {
    const uint32_t blk = blockIdx.x;
    const int s = entry_of(prefix, n_segs, blk);
    const IngestSeg S = segs[s];
    const uint32_t chunk = blk - prefix[s];
    const uint32_t lane = threadIdx.x;
    int32_t* status = status_all + static_cast<size_t>(S.slot) * 64;
    if (chunk == 0 && lane == 0 && (s == 0 || segs[s - 1].slot != S.slot)) status[word ^ kIngestWordB] = CCD_OK;  // for the NEXT run
    const uint32_t o0 = chunk * kIngestChunk;  // (< n: the prefix gives a segment ceil(n / kIngestChunk) workgroups)
    const uint32_t n = S.n - o0 < kIngestChunk ? S.n - o0 : kIngestChunk;
    const int8_t* src = S.src + o0;
    int8_t* dst = S.dst + o0;
    // [0, head) bytes, [head, head + body) 16-byte units, [head + body, n) bytes
    uint32_t head = n, body = 0;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src), da = reinterpret_cast<uintptr_t>(dst);
    if (((sa ^ da) & 15) == 0) {
        const uint32_t to_16 = static_cast<uint32_t>((16 - (sa & 15)) & 15);
        head = to_16 < n ? to_16 : n;
        body = (n - head) & ~15u;
    }
    uint32_t bad = 0;
    for (uint32_t i = lane; i < head; i += 64) {
        const uint32_t v = static_cast<uint8_t>(src[i]);
        dst[i] = static_cast<int8_t>(v);
        bad |= (v ^ (v << 1)) & 0x80u;
    }
    for (uint32_t i = head + lane * 16; i < head + body; i += 64 * 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + i);
        *reinterpret_cast<uint4*>(dst + i) = v;
        bad |= outside4(v.x) | outside4(v.y) | outside4(v.z) | outside4(v.w);
    }
    for (uint32_t i = head + body + lane; i < n; i += 64) {
        const uint32_t v = static_cast<uint8_t>(src[i]);
        dst[i] = static_cast<int8_t>(v);
        bad |= (v ^ (v << 1)) & 0x80u;
    }
    if (bad) status[word] = CCD_ERR_VALUE;
}
}  // namespace

hipError_t launch_latent_ingest(const IngestSeg* d_segs, const uint32_t* d_prefix, int n_segs, uint32_t n_blocks, int32_t* d_status_all,
                                int word, hipStream_t stream) {
    if (n_segs <= 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(latent_ingest_kernel, dim3(n_blocks), dim3(64), 0, stream, d_segs, d_prefix, n_segs, d_status_all, word);
    return hipGetLastError();
}
}  // namespace ccd
