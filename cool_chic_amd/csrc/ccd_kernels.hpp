// ccd_kernels.hpp - the one declaration of every host-callable function a .hip file defines (launch_quality: ccd_quality.hpp).
// Included by the host files that call them AND by the .hip files that define them, so that a definition which drifts from its
// declaration no longer matches it: the call site is left with an undefined symbol and the link (-Wl,--no-undefined) fails.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "ccd_device.hpp"

namespace ccd {
// ccd_entropy.hip
size_t entropy_lds_bytes(int dim, int arm_len);
hipError_t launch_entropy(const EntropyParams* d_slots, int n_slots, size_t lds_bytes, hipStream_t stream);
hipError_t launch_laplace_bounds(const int32_t* mu_idx, const int32_t* scale_idx, const int32_t* sym,
                                 const float* scale_table, int64_t n, uint32_t* left, uint32_t* right, hipStream_t stream);
hipError_t launch_laplace_sweep_generic(const float* scale_table, int scale_first, int n_scales, uint32_t* out, hipStream_t stream);
// ccd_entropy_pipe.hip
size_t entropy_pipe_lds_bytes(int dim, int n_layers, int ring_rows, int mfma);
int entropy_pipe_ring_rows(int max_grid_w);
bool entropy_pipe_supports_mfma(int dim, int n_layers, int n_ifce_out, int narrow, int max_grid_w, long long max_abs_weight,
                                long long max_feature_bound);
bool entropy_pipe_supports(int dim, int n_layers, int narrow, int max_grid_w);
hipError_t launch_entropy_pipe(const EntropyParams* d_slots, int n_slots, int nv, int mfma, int dyn, int shape, size_t lds_bytes, hipStream_t stream);
int entropy_pipe_fixed_shape(int dim, int n_layers, int n_spatial);
hipError_t launch_laplace_sweep_pipe(const float* scale_table, const double* rcp_table, int scale_first, int n_scales, uint32_t* out, hipStream_t stream);
// ccd_float.hip
hipError_t launch_upsample_step(const UpsampleLevel* d_levels, const uint32_t* d_zmap, int n_z, int max_w, int max_h, hipStream_t stream);
hipError_t launch_i8_to_f32(const int8_t* in, float* out, size_t n, hipStream_t stream);
hipError_t launch_syn_layer(const float* in, const float* in2, const float* wt, const float* bias, float* out, int c_in,
                            int c_out, int k, int residual, int relu, int h, int w, hipStream_t stream);
hipError_t launch_resize_nearest(const float* in, float* out, int c, int h_in, int w_in, int h_out, int w_out,
                                 hipStream_t stream);
hipError_t launch_resize_interp(const float* in, float* out, int c, int h_in, int w_in, int h_out, int w_out, int cubic,
                                float scale_y, float scale_x, hipStream_t stream);
hipError_t launch_final_resize(const float* in, float* out, int c, int h_in, int w_in, int h_out, int w_out, int mode,
                               hipStream_t stream);
hipError_t launch_cr_noise(float* out, size_t n, hipStream_t stream);
hipError_t launch_planes(const float* src, void* p0, void* p1, void* p2, int h, int w, int bitdepth, int frame_data_type,
                         hipStream_t stream);
hipError_t launch_widen_u8(const uint8_t* in, uint16_t* out, size_t n, hipStream_t stream);
// ccd_synth_fused.hip
bool syn_fused_supports(int c_in, int c, int halo);
void syn_fused_tiles(int h, int w, int halo, int* tiles_x, int* tiles_y);
hipError_t launch_syn_fused(const SynthFused* d_frames, int n_frames, int c_in, int c, int max_tiles_x, int max_tiles_y,
                            hipStream_t stream);
// ccd_fused.hip, ccd_fused_pre.hip, ccd_fused_cr.hip
bool fused_dec_supports(int c_in, int c);
size_t fused_dec_lds_bytes(int n_lv, int c, int n_conv, int n_params, int pre);
void fused_dec_param_shape(int c_in, int c, int* nwv, int* nws, int* nwc, int* nwo);
hipError_t launch_fused_dec(const FusedDec* d_frames, const void* d_work, int n_work, int c_in, int c, int pre, size_t lds_bytes, hipStream_t stream);
hipError_t launch_fused_dec_pre(const FusedDec* d_frames, const void* d_work, int n_work, int c_in, int c, size_t lds_bytes, hipStream_t stream);
hipError_t launch_fused_pyramid(const FusedDec* d_frames, const void* d_work, int n_work, int levels, size_t lds_bytes, hipStream_t stream);
size_t fused_pyr_lds_bytes(int n_lv);
bool fused_dec_cr_supports(int c_in, int c);
hipError_t launch_fused_dec_cr(const FusedDec* d_frames, const void* d_work, int n_work, int c_in, int c, size_t lds_bytes, hipStream_t stream);
int fused_dec_profile(unsigned long long* out16, int reset);
int fused_dec_profile_pre(unsigned long long* out16, int reset);
// ccd_inter.hip
hipError_t launch_planes_to_444(const void* p0, const void* p1, const void* p2, float* out, int h, int w, int bitdepth,
                                int frame_data_type, hipStream_t stream);
hipError_t launch_planes_to_444_jobs(const PlanesConvJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, hipStream_t stream);
hipError_t launch_inter_recon(int frame_type, int h, int w, int n_taps, const int* gflow, const float* residue, const float* motion,
                              const float* ref0, const float* ref1, float* out, hipStream_t stream);
size_t inter_coef_bytes(int frame_type, int h, int w);
hipError_t launch_inter_coef8(int frame_type, int h, int w, const float* motion, void* coef, hipStream_t stream);
hipError_t launch_inter_apply8(int frame_type, int h, int w, const int* gflow, const float* residue, const float* motion, const float* ref0,
                               const float* ref1, const void* coef, float* out, hipStream_t stream);
hipError_t launch_dsens_inter(const InterUnitJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, hipStream_t stream);
hipError_t launch_dsens_dep(const DsensDepJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, hipStream_t stream);
hipError_t launch_inter_score(const InterScoreJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, uint64_t* d_part,
                              hipStream_t stream);
hipError_t launch_inter_score_final(const InterScoreRange* d_ranges, int n_ranges, const uint64_t* d_part, uint64_t* d_sse, hipStream_t stream);
hipError_t launch_spin(unsigned long long ticks, hipStream_t stream);
// ccd_encode.hip
size_t encode_contexts_lds_bytes(int dim);
int encode_block_threads();
hipError_t launch_encode(const EncodeParams* d_slots, int n_slots, unsigned max_blocks, size_t lds_bytes, hipStream_t stream);
hipError_t launch_encode_rate(const EncodeParams* d_slots, const RateParams* d_rate, int n_slots, unsigned max_blocks, int max_grids,
                              size_t lds_bytes, hipStream_t stream);
hipError_t launch_encode_deltas(const EncodeParams* d_slots, const DeltaParams* d_delta, int n_slots, unsigned max_blocks,
                                unsigned max_tiles, size_t lds_bytes, hipStream_t stream);
hipError_t launch_encode_rate_deltas(int kind, const EncodeParams* d_slots, const RateDeltaParams* d_param, int n_slots, unsigned max_chunks,
                                     unsigned max_cand, size_t lds_generic, size_t lds_incremental, hipStream_t stream);
// ccd_ingest.hip
hipError_t launch_latent_ingest(const IngestSeg* d_segs, const uint32_t* d_prefix, int n_segs, uint32_t n_blocks, int32_t* d_status_all,
                                int word, hipStream_t stream);
// ccd_dsens.hip
hipError_t launch_dsens_apply(const DsensSeg* d_segs, const uint32_t* d_prefix, int n_segs, uint32_t n_blocks, hipStream_t stream);
hipError_t launch_dsens_sse(const DsensPass* d_passes, const uint32_t* d_unit_prefix, const uint32_t* d_probe_prefix, int n_passes,
                            uint32_t n_units, uint32_t n_probes, int64_t* d_slab, hipStream_t stream);
hipError_t launch_dsens_dep_final(const DsensDepGrid* d_grids, const uint32_t* d_prefix, int n_grids, uint32_t n_blocks, hipStream_t stream);
// ccd_inter.hip: the reach tables of the follows of one tap-count class
hipError_t launch_rdoq_reach(const RdoqReachJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, hipStream_t stream);
// The tables of one step (all device pointers), as the host hands them to launch_rdoq_step.  The kernels take the pointers they
// read as __restrict__ arguments of their own (ccd_rdoq.hip says why), not this struct.
struct RdoqStepTables {
    const RdoqGrid* grids;         // [n_grids], slot by slot
    const RdoqSlot* slots;         // [n_slots]
    const uint32_t* lane_prefix;   // [n_grids + 1] workgroups of 64 latents, a lane each
    const uint32_t* big_prefix;    // [n_grids + 1] entries of the `big` lists, a workgroup each
    const uint32_t* chunk_prefix;  // [n_grids + 1] chunks of kRdoqChunk latents (reduce, phase 0)
    const uint32_t* cell_prefix;   // [n_slots + 1] workgroups of 64 cells of the rasters' owners (settle)
    int32_t n_grids, n_slots;
    uint32_t n_lane_blocks;        // lane_prefix[n_grids]: the workgroups behind them are the waves of the `big` lists
    // with follows or dependent maps; null, and read by no kernel, without
    const RdoqGridX* gx;           // beside the grid table
    const RdoqSlotX* sx;           // beside the slot table
    const uint32_t* comp_uid;      // first uids of the slots, component by component, ascending inside one
    const int32_t* comp_slot;      // ... and their slots
};
// One step as ccd_rdoq.hip launches it: `rounds` times claim, select (and settle between two rounds), then the two phases of the
// reduce launch.  t.gx != nullptr (a handle with follows or dependent maps): the reach tables and the flow boxes first, then the
// following variants of the same launches; the members from reach_jobs on are read only then.
struct RdoqStepLaunch {
    RdoqStepTables t;
    RdoqSums sums;
    uint32_t n_big, n_chunks, n_cell_blocks;  // the ends of t.big_prefix, t.chunk_prefix, t.cell_prefix
    int rounds;
    const RdoqReachJob* reach_jobs[2];  // [0] run-time taps, [1] sinc-8
    const uint32_t* reach_prefix[2];
    int n_reach[2];
    uint32_t reach_blocks[2];
    void* reach_mem;                // every reach table of the handle, one block
    size_t reach_bytes;
    int stages;                     // ccd_rdoq_debug_stages: 1 memset + reach, 2 flow boxes, 4 rounds + sums (tools/rd_bench.py)
};
hipError_t launch_rdoq_step(const RdoqStepLaunch& L, hipStream_t stream);
}  // namespace ccd
