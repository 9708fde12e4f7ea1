// ccd_runtime.cpp - what lives as long as the process (block pool, per-device tables and streams) and the entry points of
// include/ccd.h that need no batch: errors, header parsing, the classes of a network, debug hooks.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ccd_host.hpp"
#include "ccd_kernels.hpp"

namespace ccd {
static const uint32_t kScaleBits[kNumScale] = {
#include "../../include/ccd_scale_table.inc"
};

size_t BlockPool::size_class(size_t bytes) {
    if (bytes <= 4096) return 4096;
    size_t p2 = 4096;
    while (p2 < bytes) p2 <<= 1;
    if (p2 <= (size_t{1} << 20)) return p2;
    const size_t step = p2 >> 4;  // eighths of the power of two below
    return (bytes + step - 1) / step * step;
}
void* BlockPool::acquire(int device, Kind kind, size_t bytes, size_t* got) {
    const size_t cls = size_class(bytes);
    *got = cls;
    {
        std::lock_guard<std::mutex> lock(mu_);
        auto& fl = free_[key(device, kind)];
        auto it = fl.find(cls);
        if (it != fl.end()) {
            void* p = it->second;
            fl.erase(it);
            cached_[key(device, kind)] -= cls;
            return p;
        }
    }
    void* p = nullptr;
    const hipError_t e = kind == kDevice ? hipMalloc(&p, cls) : hipHostMalloc(&p, cls, hipHostMallocDefault);
    if (e != hipSuccess) {  // out of memory with blocks of other classes cached: give them back and retry once
        (void)hipGetLastError();
        trim(device);
        if ((kind == kDevice ? hipMalloc(&p, cls) : hipHostMalloc(&p, cls, hipHostMallocDefault)) != hipSuccess) return nullptr;
    }
    return p;
}
void BlockPool::release(int device, Kind kind, void* p, size_t cls) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lock(mu_);
        size_t& cached = cached_[key(device, kind)];  // the caps are per device (and kind), like the free lists and trim()
        if (cached + cls <= cap(kind)) {
            free_[key(device, kind)].emplace(cls, p);
            cached += cls;
            return;
        }
    }
    if (kind == kDevice) (void)hipFree(p); else (void)hipHostFree(p);
}
void BlockPool::trim(int device) {
    std::vector<std::pair<Kind, void*>> drop;
    {
        std::lock_guard<std::mutex> lock(mu_);
        for (int k = 0; k < 2; ++k) {
            auto& fl = free_[key(device, static_cast<Kind>(k))];
            for (auto& e : fl) drop.emplace_back(static_cast<Kind>(k), e.second);
            cached_[key(device, static_cast<Kind>(k))] = 0;
            fl.clear();
        }
    }
    for (auto& d : drop) { if (d.first == kDevice) (void)hipFree(d.second); else (void)hipHostFree(d.second); }
}
size_t BlockPool::cap(Kind kind) {
    static const size_t caps[2] = {env_mb("CCD_POOL_MAX_MB", 16384), env_mb("CCD_PINNED_POOL_MAX_MB", 2048)};
    return caps[kind];
}
size_t BlockPool::env_mb(const char* name, size_t dflt) {
    const char* e = std::getenv(name);
    return (e ? static_cast<size_t>(std::strtoull(e, nullptr, 10)) : dflt) << 20;
}
BlockPool& pool() { static BlockPool p; return p; }
}  // namespace ccd

using namespace ccd;

namespace {
std::mutex g_shared_mu;
std::map<int, DeviceShared> g_shared;

// Which side streams run concurrently (see DeviceShared::conc).  Two spin kernels of ~0.2 ms, one on each of two streams, take
// ~0.2 ms when the streams sit on different hardware queues and ~0.4 ms when they share one; a greedy clique of up to four.  ~10 ms
// once per device and process.  CCD_SIDE_STREAMS=k skips the measurement and takes the first k (0 < k <= 8; r05's behaviour: 8).
// Under a profiler that serialises kernels nothing is concurrent: one stream, launches in a row - correct, only slower.
void calibrate_side_streams(DeviceShared& d) {
    d.n_conc = 1; d.conc[0] = 0;
    if (const char* e = std::getenv("CCD_SIDE_STREAMS")) {
        const int k = std::atoi(e);
        if (k >= 1 && k <= DeviceShared::kSide) { d.n_conc = k; for (int i = 0; i < k; ++i) d.conc[i] = i; return; }
    }
    const unsigned long long ticks = 400000ull;  // ~0.17 ms of the shader clock
    auto pair_ms = [&](int a, int b2) -> double {
        double best = 1e9;
        for (int trial = 0; trial < 3; ++trial) {
            if (hipStreamSynchronize(d.side[a]) != hipSuccess || hipStreamSynchronize(d.side[b2]) != hipSuccess) return 1e9;
            const auto t0 = std::chrono::steady_clock::now();
            if (launch_spin(ticks, d.side[a]) != hipSuccess || launch_spin(ticks, d.side[b2]) != hipSuccess) return 1e9;
            if (hipStreamSynchronize(d.side[a]) != hipSuccess || hipStreamSynchronize(d.side[b2]) != hipSuccess) return 1e9;
            best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        return best;
    };
    // one kernel alone (same stream twice = certainly serial): the yardstick, whatever the clock
    const double serial = pair_ms(0, 0);
    if (serial >= 1e8) return;
    for (int j = 1; j < DeviceShared::kSide && d.n_conc < 4; ++j) {
        bool with_all = true;
        for (int i = 0; i < d.n_conc && with_all; ++i) with_all = pair_ms(d.conc[i], j) < 0.75 * serial;
        if (with_all) d.conc[d.n_conc++] = j;
    }
    if (std::getenv("CCD_VIDEO_TIMING") || std::getenv("CCD_DEBUG_STREAMS")) {
        std::fprintf(stderr, "[ccd] side streams that run concurrently: %d (", d.n_conc);
        for (int i = 0; i < d.n_conc; ++i) std::fprintf(stderr, "%s%d", i ? " " : "", d.conc[i]);
        std::fprintf(stderr, "), two kernels in a row %.3f ms\n", serial);
    }
}
}  // namespace

int ccd::device_shared(int device, DeviceShared** out) {
    std::lock_guard<std::mutex> lock(g_shared_mu);
    DeviceShared& d = g_shared[device];
    if (!d.up_stream) {
        float* st = nullptr;
        double* rt = nullptr;
        hipStream_t us = nullptr;
        std::vector<double> rcp(kNumScale);
        for (int i = 0; i < kNumScale; ++i) {
            float f;
            std::memcpy(&f, &kScaleBits[i], 4);
            rcp[i] = 1.0 / static_cast<double>(f);  // IEEE division on the host: correctly rounded
        }
        if (hipMalloc(&st, sizeof(kScaleBits)) != hipSuccess || hipMalloc(&rt, sizeof(double) * kNumScale) != hipSuccess) {
            if (st) (void)hipFree(st);
            return CCD_ERR_NOMEM;
        }
        if (hipMemcpy(st, kScaleBits, sizeof(kScaleBits), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(rt, rcp.data(), sizeof(double) * kNumScale, hipMemcpyHostToDevice) != hipSuccess ||
            hipStreamCreateWithFlags(&us, hipStreamNonBlocking) != hipSuccess) {
            (void)hipFree(st); (void)hipFree(rt);
            return CCD_ERR_HIP;
        }
        d.d_scale_table = st; d.d_rcp_table = rt; d.up_stream = us;
        bool ok = true;
        for (int k = 0; k < DeviceShared::kSide && ok; ++k) ok = hipStreamCreateWithFlags(&d.side[k], hipStreamNonBlocking) == hipSuccess;
        if (!ok) return CCD_ERR_HIP;
        calibrate_side_streams(d);
        { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) d.n_cu = v; }
    }
    *out = &d;
    return CCD_OK;
}

extern "C" {

const char* ccd_strerror(int code) {
    switch (code) {
        case CCD_OK: return "ok";
        case CCD_ERR_TRUNCATED: return "bitstream truncated";
        case CCD_ERR_VALUE: return "header value out of range";
        case CCD_ERR_INVALID_DATA: return "invalid compressed data";
        case CCD_ERR_UNSUPPORTED: return "feature not supported by this build";
        case CCD_ERR_NOMEM: return "out of memory";
        case CCD_ERR_HIP: return "HIP runtime error / no usable gfx950 device";
        case CCD_ERR_ARG: return "bad argument";
        default: return "unknown error";
    }
}

const char* ccd_version(void) { return "ccd 0.1.0 gfx950"; }

int ccd_read_video_header(const uint8_t* p, size_t n, ccd_video_header* h) { return (p && h) ? read_video_header(p, n, h) : CCD_ERR_ARG; }
int ccd_read_frame_header(const uint8_t* p, size_t n, ccd_frame_header* h) { return (p && h) ? read_frame_header(p, n, h) : CCD_ERR_ARG; }
int ccd_read_cc_header(const uint8_t* p, size_t n, ccd_cc_header* h) { return (p && h) ? read_cc_header(p, n, h) : CCD_ERR_ARG; }

int ccd_get_coding_structure(const ccd_video_header* h, int32_t* display_order, int32_t* frame_type, int32_t* refs, int32_t* depth) {
    if (!h) return CCD_ERR_ARG;
    std::vector<CodedFrame> cs;
    const int rc = coding_structure(*h, cs);
    if (rc < 0) return rc;
    for (size_t i = 0; i < cs.size(); ++i) {
        if (display_order) display_order[i] = cs[i].display_order;
        if (frame_type) frame_type[i] = cs[i].frame_type;
        if (refs) { refs[2 * i] = cs[i].n_refs > 0 ? cs[i].refs[0] : -1; refs[2 * i + 1] = cs[i].n_refs > 1 ? cs[i].refs[1] : -1; }
        if (depth) depth[i] = cs[i].depth;
    }
    return static_cast<int>(cs.size());
}

void ccd_free(void* p) { std::free(p); }

void ccd_pool_trim(int device) {
    if (hipSetDevice(device) != hipSuccess) return;
    (void)hipDeviceSynchronize();
    pool().trim(device);
}

int ccd_concurrent_streams(int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return CCD_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    DeviceShared* sh = nullptr;
    const int rc = device_shared(device, &sh);
    return rc < 0 ? rc : sh->n_conc;
}

int ccd_network_fits_fast_path(const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn) {
    if (!cc_header || !bytes_nn) return CCD_ERR_ARG;
    std::unique_ptr<ccd_cc_header> h(new (std::nothrow) ccd_cc_header());
    if (!h) return CCD_ERR_NOMEM;
    int rc = read_cc_header(cc_header, n_hdr, h.get());
    if (rc < 0) return rc;
    Network net;
    rc = decode_network(*h, bytes_nn, n_nn, net);
    if (rc < 0) return rc;
    int max_w = 0;
    for (int g = 0; g < h->n_grids; ++g) max_w = std::max(max_w, static_cast<int>(h->grid_w[g]));
    return entropy_pipe_supports(h->total_context_arm, h->n_hidden_layers_arm + 1, (net.arm.w32 && net.feat_i32 && !net.arm.dyn_act) ? 1 : 0, max_w) ? 1 : 0;
}

int ccd_network_kernel_class(const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn) {
    if (!cc_header || !bytes_nn) return CCD_ERR_ARG;
    std::unique_ptr<ccd_cc_header> h(new (std::nothrow) ccd_cc_header());
    if (!h) return CCD_ERR_NOMEM;
    int rc = read_cc_header(cc_header, n_hdr, h.get());
    if (rc < 0) return rc;
    Network net;
    rc = decode_network(*h, bytes_nn, n_nn, net);
    if (rc < 0) return rc;
    int max_w = 0;
    for (int g = 0; g < h->n_grids; ++g) max_w = std::max(max_w, static_cast<int>(h->grid_w[g]));
    const bool pipe = entropy_pipe_supports(h->total_context_arm, h->n_hidden_layers_arm + 1, (net.arm.w32 && net.feat_i32 && !net.arm.dyn_act) ? 1 : 0, max_w);
    int n_levels = 0;
    for (int g = 0; g < h->n_grids; ++g) n_levels += h->is_hyperlatent[g] ? 0 : 1;
    const bool finite = float_path_stays_finite(net, n_levels, h->flag_common_randomness ? n_levels : 0);
    const bool mfma = pipe && entropy_pipe_supports_mfma(h->total_context_arm, h->n_hidden_layers_arm + 1, h->output_feature_ifce, net.arm.narrow ? 1 : 0,
                                                         max_w, arm_max_abs_weight(net.arm), worst_feature_bound(net));
    return (pipe ? 1 : 0) | (pipe && net.arm.dyn_feat ? 16 : 0) | (finite ? 0 : 128) | (((h->total_context_arm + 3) / 4 & 15) << 8) |
           (((h->n_hidden_layers_arm + 1) & 15) << 12) | (net.arm.narrow ? 1 << 16 : 0) | (net.ifce_w32 ? 1 << 17 : 0) | (mfma ? 1 << 18 : 0) |
           (net.arm.w32 ? 1 << 19 : 0) | (net.arm.dyn_act ? 1 << 20 : 0) | (net.feat_i32 ? 1 << 21 : 0) | (net.arm.dyn_feat ? 1 << 22 : 0);
}

int ccd_debug_fd_profile(uint64_t* out16, int reset) {
    return out16 ? fused_dec_profile(reinterpret_cast<unsigned long long*>(out16), reset) : CCD_ERR_ARG;
}

int ccd_debug_laplace_bounds(int device, const int32_t* mu_idx, const int32_t* scale_idx, const int32_t* s, int64_t n,
                             uint32_t* left, uint32_t* right) {
    if (n <= 0) return CCD_OK;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return CCD_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    int32_t *d_mu = nullptr, *d_sc = nullptr, *d_s = nullptr;
    uint32_t *d_l = nullptr, *d_r = nullptr;
    float* d_tab = nullptr;
    int rc = CCD_OK;
    const size_t nb = static_cast<size_t>(n) * 4;
    if (hipMalloc(&d_mu, nb) != hipSuccess || hipMalloc(&d_sc, nb) != hipSuccess || hipMalloc(&d_s, nb) != hipSuccess ||
        hipMalloc(&d_l, nb) != hipSuccess || hipMalloc(&d_r, nb) != hipSuccess || hipMalloc(&d_tab, sizeof(kScaleBits)) != hipSuccess)
        rc = CCD_ERR_NOMEM;
    if (rc == CCD_OK &&
        (hipMemcpy(d_mu, mu_idx, nb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_sc, scale_idx, nb, hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(d_s, s, nb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_tab, kScaleBits, sizeof(kScaleBits), hipMemcpyHostToDevice) != hipSuccess))
        rc = CCD_ERR_HIP;
    if (rc == CCD_OK && launch_laplace_bounds(d_mu, d_sc, d_s, d_tab, n, d_l, d_r, nullptr) != hipSuccess) rc = CCD_ERR_HIP;
    if (rc == CCD_OK && (hipMemcpy(left, d_l, nb, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(right, d_r, nb, hipMemcpyDeviceToHost) != hipSuccess))
        rc = CCD_ERR_HIP;
    (void)hipFree(d_mu); (void)hipFree(d_sc); (void)hipFree(d_s); (void)hipFree(d_l); (void)hipFree(d_r); (void)hipFree(d_tab);
    return rc;
}

int ccd_debug_laplace_sweep(int device, int which, int scale_first, int n_scales, uint32_t* out) {
    if (!out || scale_first < 0 || n_scales <= 0 || scale_first + n_scales > kNumScale || (which != 0 && which != 1)) return CCD_ERR_ARG;
    ccd_batch* b = nullptr;  // owns the two Laplace-scale tables on the device
    int rc = ccd_batch_create(device, &b);
    if (rc < 0) return rc;
    const size_t bytes = static_cast<size_t>(n_scales) * kNumMu * 127 * sizeof(uint32_t);
    uint32_t* d_out = nullptr;
    if (hipMalloc(&d_out, bytes) != hipSuccess) rc = CCD_ERR_NOMEM;
    if (rc == CCD_OK) {
        const hipError_t e = which == 0 ? launch_laplace_sweep_pipe(b->d_scale_table, b->d_rcp_table, scale_first, n_scales, d_out, nullptr)
                                        : launch_laplace_sweep_generic(b->d_scale_table, scale_first, n_scales, d_out, nullptr);
        if (e != hipSuccess || hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = CCD_ERR_HIP;
    }
    if (d_out) (void)hipFree(d_out);
    ccd_batch_destroy(b);
    return rc;
}

}  // extern "C"
