// ccd_host.hpp - what the host files behind the C ABI share (host only): the block pool and what every handle builds on it (Block,
// Mirror, TableImage, StreamSet), per-device state, a batch and its slots.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "ccd_device.hpp"
#include "ccd_format.hpp"

// A failed call is reported by the return code alone: the thread's last HIP error is read once more, which resets it, so that
// the caller's own runtime (PyTorch checks hipGetLastError after its launches) does not meet an error that was this library's.
#define HIP_TRY(expr)                           \
    do {                                        \
        hipError_t e__ = (expr);                \
        if (e__ != hipSuccess) {                \
            (void)hipGetLastError();            \
            return CCD_ERR_HIP;                 \
        }                                       \
    } while (0)

namespace ccd {

// Caches of device blocks and pinned host blocks, one per device (free lists, byte counts and caps are all per device): a batch is created, filled, run and destroyed
// per image set, and hipMalloc / hipFree / hipHostMalloc of its arenas were a fifth of the time from bytes to planes
// (24 hipFree = 4.4 ms per Kodak set; 64 arenas of 50-100 MB per 1080p GOP).  Blocks are handed out in size classes
// (power of two up to 1 MB, then eighths of a power of two: <= 12.5 % slack) and come back on destroy; the cache is capped
// (CCD_POOL_MAX_MB, default 16384; CCD_PINNED_POOL_MAX_MB, default 2048: the cache is invisible to PyTorch's allocator, so it
// stays a few percent of the device) - beyond the cap a block is really freed.
// ccd_pool_trim() empties the caches.  The current device must be the block's device (callers hipSetDevice first).
class BlockPool {
public:
    enum Kind { kDevice = 0, kPinned = 1 };
    static size_t size_class(size_t bytes);
    void* acquire(int device, Kind kind, size_t bytes, size_t* got);
    void release(int device, Kind kind, void* p, size_t cls);
    void trim(int device);
private:
    static int key(int device, Kind kind) { return device * 2 + kind; }
    static size_t cap(Kind kind);
    static size_t env_mb(const char* name, size_t dflt);
    std::mutex mu_;
    std::map<int, std::multimap<size_t, void*>> free_;
    std::map<int, size_t> cached_;  // bytes in free_[key], same key
};
BlockPool& pool();  // the process's one pool (ccd_runtime.cpp)

// A block from the pool with its class size (what release() needs).
struct Block {
    void* p = nullptr;
    size_t cls = 0;
    int device = 0;
    BlockPool::Kind kind = BlockPool::kDevice;
    bool get(int dev, BlockPool::Kind k, size_t bytes) { drop(); device = dev; kind = k; p = pool().acquire(dev, k, bytes, &cls); return p != nullptr; }
    // grows only: a block that is large enough stays (nothing of it may be in flight when it is exchanged)
    bool ensure(int dev, BlockPool::Kind k, size_t bytes) { return cls >= bytes || get(dev, k, bytes); }
    void drop() { if (p) pool().release(device, kind, p, cls); p = nullptr; cls = 0; }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// A device block and the pinned block it is staged through: tables go up, results come down, `bytes` of them.
struct Mirror {
    Block dev, host;
    bool ensure(int device, size_t bytes) { return dev.ensure(device, BlockPool::kDevice, bytes) && host.ensure(device, BlockPool::kPinned, bytes); }
    hipError_t upload(size_t bytes, hipStream_t st) const { return hipMemcpyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, st); }
    hipError_t download(size_t bytes, hipStream_t st) const { return hipMemcpyAsync(host.p, dev.p, bytes, hipMemcpyDeviceToHost, st); }
    // the table a TableImage placed at `off`, where the kernels read it
    template <typename T> const T* dev_at(size_t off) const { return reinterpret_cast<const T*>(dev.as<char>() + off); }
    void drop() { dev.drop(); host.drop(); }
};

// Everything placed in a device block starts on a 256-byte boundary.
inline size_t align256(size_t v) { return (v + 255) & ~size_t{255}; }

// The rules of P / B frames that every entry point checks (ccd_inter_reconstruct, ccd_decode_video, ccd_dsens_add_inter).
// 2 / 4 taps = grid_sample bilinear / bicubic, 6.. = sinc (warp.py:49-56); odd or < 2 fails the reference's asserts (warp.py:41-47)
inline bool warp_filter_ok(int taps) { return taps >= 2 && taps <= 16 && !(taps & 1); }
// output channels of the cool-chics of a P (1) / B (2) frame (decode.py:156-189): role 0, the residue, has three colours, alpha and
// for B beta; role 1, the motion, one flow per reference
inline int inter_channels(int frame_type, int role) { return role == 0 ? (frame_type == 2 ? 5 : 4) : (frame_type == 2 ? 4 : 2); }
// 4:2:0 needs even sides: F.avg_pool2d(2) drops the odd row / column and write_yuv's chroma planes are h/2 x w/2, the reference's
// 4:4:4 round trip (yuv.py:303-316) no longer matches the luma size, and planes_to_444_kernel would read past such a chroma plane
inline bool yuv420_sides_ok(int frame_data_type, int h, int w) { return frame_data_type != 1 || !((h | w) & 1); }

// Host image of tables that go to the device in one copy; put() returns the aligned offset of what it appended.
struct TableImage {
    std::vector<char> bytes;
    size_t put(const void* p, size_t n) {
        const size_t at = align256(bytes.size());
        bytes.resize(at + n);
        if (n) std::memcpy(bytes.data() + at, p, n);
        return at;
    }
    template <typename T> size_t put(const std::vector<T>& v) { return put(v.data(), v.size() * sizeof(T)); }
};

// Every stream work of a handle was enqueued on: all of them are drained before a block of the handle goes back to the pool,
// not only the last one.
struct StreamSet {
    std::vector<hipStream_t> used;
    void note(hipStream_t st) { if (std::find(used.begin(), used.end(), st) == used.end()) used.push_back(st); }
    int drain() const {
        int rc = CCD_OK;
        for (hipStream_t st : used) if (hipStreamSynchronize(st) != hipSuccess) rc = CCD_ERR_HIP;
        return rc;
    }
};

// Per device, for the life of the process: the two Laplace-scale tables and the stream uploads run on (so that parsing
// slot k + 1 on the host overlaps the copy of slot k, and nothing waits for the caller's stream).
struct DeviceShared {
    float* d_scale_table = nullptr;
    double* d_rcp_table = nullptr;
    hipStream_t up_stream = nullptr;
    // side streams for the entropy launches of one batch (one per kernel instantiation in use: MLP width x variant): a
    // stream is a serial chain on one CU, so launches that queue behind each other on ONE stream add their durations
    static constexpr int kSide = 8;
    hipStream_t side[kSide] = {};
    // r06: which of them REALLY run at once.  HIP multiplexes its streams onto a few hardware queues (four by default,
    // GPU_MAX_HW_QUEUES), and two launches on streams that share one run one after the other: tools/ubench/queues.hip on MI355X /
    // ROCm 7.2 - the null stream + side[1] 9.7 ms where the null stream + side[0] take 4.9, three "concurrent" launches 2 x one
    // (profiles/r06/queues.txt); r05's fork over (caller's stream, side[0], side[1], ...) was serial or not by luck - with a
    // batch of 256 streams in two launches 72 ms instead of 37.  So the side streams are MEASURED once per device (calibrate):
    // conc[0 .. n_conc) are mutually concurrent ones (one per hardware queue: at most four are looked for), and the launches of a
    // batch that need to overlap go to those only - never to the caller's stream, which idles at the join and may alias any of them.
    int n_conc = 0;
    int conc[kSide] = {};
    int n_cu = 256;   // multiProcessorCount, read once (hipGetDeviceProperties is not a call for the path of every batch)
};
int device_shared(int device, DeviceShared** out);  // ccd_runtime.cpp

// Bump allocator over one pooled device block: every slot's buffers live in a single arena.
class Arena {
public:
    size_t reserve(size_t bytes) { size_t off = total_; total_ += align256(bytes); return off; }
    int commit(int device) {
        if (total_ == 0) total_ = 256;
        return blk_.get(device, BlockPool::kDevice, total_) ? CCD_OK : CCD_ERR_NOMEM;
    }
    template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(blk_.as<char>() + off); }
    void release() { blk_.drop(); }
    size_t total() const { return total_; }
private:
    Block blk_;
    size_t total_ = 0;
};

struct Slot {
    ccd_cc_header hdr;
    Network net;
    int bitdepth = 0, frame_data_type = 0;
    Arena arena;
    EntropyParams ep;
    std::vector<UpsampleLevel> levels;
    int dense_c = 0, dense_h = 0, dense_w = 0;
    float* d_dense = nullptr;
    // common randomness (coolchic.py:179-183): noise pyramid + two ping-pong stacks for fixed_upsampling
    bool cr = false;
    float* d_noise = nullptr;
    float* d_nstack[2] = {nullptr, nullptr};
    std::vector<size_t> noise_off;        // per latent level, finest first
    std::vector<int> lvl_h, lvl_w;        // latent level sizes, finest first
    // synthesis
    float* d_syn_params = nullptr;
    bool use_fused_syn = false;      // whole synthesis in one kernel (ccd_synth_fused.hip)
    SynthFused fused;
    bool use_fused_dec = false;      // upsampling + synthesis + integer samples in one kernel (ccd_fused.hip)
    bool float_finite = true;        // float_path_stays_finite(): the network cannot leave the finite float32 range
    bool fdec_pre = false;           // ... whose level-1 stack comes from the batch's pyramid launch (CCD_OPT_FUSED_DEC = 2)
    FusedDec fpyr;                   // ... descriptor of that launch: the same walk one level up (level 0 = this frame's level 1)
    FusedDec fdec;
    size_t fdec_lds = 0;
    std::vector<size_t> w_off, b_off;  // per main layer
    size_t stab_w = 0, stab_b = 0, out_w = 0, out_b = 0;
    float* d_tmp[2] = {nullptr, nullptr};
    float* d_stab = nullptr;
    float* d_syn_out = nullptr;  // [C][dense_h][dense_w]
    float* d_out = nullptr;      // [C][H][W] (== d_syn_out when no resize)
    void* d_plane[3] = {nullptr, nullptr, nullptr};
    int plane_h[3] = {0, 0, 0}, plane_w[3] = {0, 0, 0};
    size_t plane_off[3] = {0, 0, 0}, planes_bytes = 0;  // the three planes sit in ONE block of the arena (one copy moves them)
    Block staging;           // pinned host copy of the arena's head (status, payload, networks) for the asynchronous upload
    int32_t* d_status = nullptr;
    bool use_pipe = false;   // pipelined entropy kernel (32-bit operands) or the generic one
    bool use_mfma = false;   // ... with the ARM's layers on the matrix cores (limb-split int8)
    bool use_dyn = false;    // ... the instantiation that checks IFCE features on the device (worst case >= 2^15, or the test hook)
    int fixed_shape = 0;     // ... the instantiation with a compile-time ARM shape (1: intra/hop.cfg = 14 + 6 inputs, two hidden layers)
    int ring_rows = 64;      // rows of the pipelined kernel's decoded-symbol ring
    size_t lds_generic = 0, lds_pipe = 0;
    int lg = -1;             // entropy launch of the batch this slot is decoded by (index into ccd_batch::pipe_groups; -1: the generic launch)
    int fl = -1;             // launch group its float-path launches are keyed by (= lg while ccd_batch_run overlaps; -1: not keyed)
    // latents GIVEN instead of range-coded (ccd_batch_add_latents): no entropy launch holds the slot.  Host latents went up with
    // the head; device latents are copied from given_src[g] at the head of every run (ccd_ingest.hip)
    bool given = false, given_device = false;
    const int8_t* given_src[CCD_MAX_GRIDS] = {};
    int status = CCD_OK;
    int32_t host_status[64] = {0};
};

// The integer networks as the entropy kernels read them (the decoder's two and the device writer's): ARM = per layer w[in][out],
// b[out], then the stabiliser ws[dim][2], bs[2]; IFCE = per grid that has one w[in][out], b[out] at ifce_off[g].
struct IntNetBlobs {
    std::vector<int64_t> arm, ifce;
    std::vector<int32_t> ifce_off;
};
// (ccd_batch_plan.cpp)
void pack_int_networks(const ccd_cc_header& h, const Network& net, IntNetBlobs& out);
void fill_entropy_model(const ccd_cc_header& h, const Network& net, const IntNetBlobs& blobs, EntropyParams& E);
bool grids_nest(const ccd_cc_header& h);
// Plans every launch of the batch and uploads the tables they read, when slots were added since the last call (or `regroup`).
int build_launch_tables(ccd_batch* b, hipStream_t st);
// (ccd_dsens_api.cpp) Where a move of one latent of `grid` can reach: per axis a (0 rows, 1 columns) the samples
// [s + lo[a], s + hi[a]], s = floor(i * num[a] / den[a]) for the latent index i, before clipping to the picture.  footprint()
// returns 1 for a hyperlatent grid.
struct Footprint { int32_t lo[2], hi[2]; uint32_t num[2], den[2]; };
int footprint(const ccd_cc_header& h, int grid, Footprint& f);

}  // namespace ccd

struct ccd_batch {
    int device = 0;
    std::vector<std::unique_ptr<ccd::Slot>> slots;
    ccd::EntropyParams* d_params = nullptr;   // [pipe slots..., generic slots...]
    int n_params_uploaded = 0;
    bool regroup = false;                // an option that shapes the launch tables changed: rebuild them at the next run
    // every table the launches read (entropy descriptors, fused-kernel frames and work lists, pyramid steps) and the status
    // words of all slots live in ONE pooled device block, staged through ONE pinned block: one copy up, one copy down
    ccd::Block tables, tables_staging, status_host;
    int32_t* d_status_all = nullptr;     // [slots][64]
    hipEvent_t up_done = nullptr;        // recorded on the upload stream behind the last ccd_batch_add
    hipStream_t up_stream = nullptr;     // the device's shared upload stream
    // every stream the caller handed to ccd_batch_run_stage / ccd_batch_wait / ccd_batch_copy_*: drained before a block of this
    // batch goes back to the pool (or its tables are replaced)
    ccd::StreamSet streams;
    hipStream_t run_stream = nullptr;    // the stream of the last ccd_batch_run[_stage]: ccd_batch_wait waits for it too
    bool has_run = false;
    int drain();                         // ... with this batch's launches on the shared side streams (ccd_batch.cpp)
    // fork / join of the entropy launches over the device's side streams: the EVENTS belong to the batch (two host threads
    // running two batches on one GPU share the side streams, which only serialises their launches, but never an event)
    hipEvent_t fork = nullptr;
    hipEvent_t side_done[ccd::DeviceShared::kSide] = {};   // recorded behind EVERY launch of this batch on side stream k
    bool side_pending[ccd::DeviceShared::kSide] = {};      // ... and not yet known to have completed
    // the launch tables' copy (build_launch_tables): a run on ANOTHER stream than the one that carried it waits for this event
    hipEvent_t params_up = nullptr;
    hipStream_t params_stream = nullptr;
    bool uploads_unconfirmed = false;    // slots were added since the last ccd_batch_wait: launches order themselves behind up_done
    int n_pipe = 0, n_generic = 0;
    // cg: chain group - the slots of one kernel instantiation split by the expected length of their serial chains, so that the
    // float-path launches of the streams that finish early run while the longest chains are still decoding (ccd_batch_run)
    struct PipeGroup { int nv, mfma, dyn, shape, cg, first, n; size_t lds; double est; };
    // CCD_OPT_TIME_LAUNCHES: timing events around every entropy launch, on the stream it runs on (bench.py's roofline: the launches
    // of a step overlap on side streams, so events on the caller's stream only see the whole stage)
    int opt_time_launches = 0;
    std::vector<hipEvent_t> lt0, lt1;    // per entropy launch of the last run (launch order)
    // behind the float launches of pipe group gi in the last OVERLAPPED run (ccd_decode_video: a frame's flows are ready when the
    // launch of its motion cool-chic is, long before the whole batch); lg_valid: recorded in the last run
    std::vector<hipEvent_t> lg_done;
    bool lg_valid = false;
    int n_timed = 0;
    int opt_overlap = 1;                 // CCD_OVERLAP=0 (environment; A/B and tests): one entropy launch per instantiation, float stages behind the join
    std::vector<PipeGroup> pipe_groups;
    float* d_scale_table = nullptr;
    double* d_rcp_table = nullptr;
    size_t lds_generic = 0, lds_pipe = 0;
    int force_generic = 0;               // CCD_FORCE_GENERIC=1: tests exercise the fallback kernels
    // fused-synthesis launches: frames grouped by (padded input channels, output channels)
    struct FusedGroup { int cp, c, c_in, n, first, max_tx, max_ty; };
    std::vector<FusedGroup> fused_groups;
    ccd::SynthFused* d_fused = nullptr;
    // fused float path (ccd_fused.hip): frames grouped by (latent levels, output channels); one workgroup per run of tiles
    struct FdecGroup { int c_in, c, pre, cr, fl, first_frame, first_work, n_work; size_t lds; };
    std::vector<FdecGroup> fdec_groups;
    ccd::FusedDec* d_fdec = nullptr;
    void* d_fdec_work = nullptr;
    // pyramid launches in front of the kFdPre groups (stage 1): descriptors grouped by their number of levels
    struct PyrGroup { int levels, fl, first_frame, first_work, n_work; size_t lds; };
    std::vector<PyrGroup> pyr_groups;
    ccd::FusedDec* d_pyr = nullptr;
    void* d_pyr_work = nullptr;
    int opt_fused_dec = 2;               // CCD_OPT_FUSED_DEC: 2 = fused kernel behind the pyramid launch, 1 = the whole pyramid per tile, 0 = unfused
    int opt_keep_float = 1;              // CCD_OPT_KEEP_FLOAT
    int opt_range_bits = 0;              // CCD_OPT_RANGE_BITS (tests: lowered feature limit of the dynamic operand check)
    int opt_mfma_arm = 0;                // CCD_OPT_MFMA_ARM (off: bit-exact but slower than the vector-ALU producers)
    int opt_fixed_shape = 1;             // CCD_FIXED_SHAPE=0 (environment; A/B and tests): every network through the run-time-shape instantiations
    // upsampling: step k of every slot's pyramid in one launch
    struct UpsStep { int first_z, n_z, max_w, max_h; };
    std::vector<UpsStep> ups_steps;
    ccd::UpsampleLevel* d_levels = nullptr;
    uint32_t* d_zmap = nullptr;
    // the ingest launch of the slots whose latents are device pointers: one segment per grid, a prefix of 64-lane workgroups
    ccd::IngestSeg* d_ingest = nullptr;
    uint32_t* d_ingest_prefix = nullptr;
    int n_ingest = 0;
    uint32_t n_ingest_blocks = 0;
    unsigned ingest_runs = 0;            // ingest launches so far: launch k reports into status word (k & 1) * kIngestWordB
};
