// ccd_quality_api.cpp - ccd_quality_* of include/ccd.h: the host side of the quality meter.
#include <cmath>
#include <cstring>
#include <new>

#include "ccd_host.hpp"
#include "ccd_quality.hpp"

using namespace ccd;

extern "C" {

// ---- quality meter (ccd_quality.hip) --------------------------------------------------------
namespace {
// Everything the host decides about a scoring: the plane table, the tile prefix tables and where each piece sits in the one
// device block.  Built by the validation that ccd_quality_scratch_bytes exposes, so no device is needed to refuse a batch.
struct QualityPlan {
    std::vector<QualityPlane> planes;        // pool pointers are filled in once the block is there
    std::vector<size_t> pool_off;            // [plane][2][kQScales - 1] byte offsets into the block
    std::vector<uint32_t> sse_prefix, ms_prefix;
    uint32_t scale_first[kQScales + 1] = {0};
    size_t off_planes = 0, off_sse_prefix = 0, off_ms_prefix = 0, head_bytes = 0;  // the head is uploaded in one copy
    size_t off_sse_part = 0, off_ms_part = 0, off_out = 0, total = 0;
};

int quality_plan(const ccd_quality_item* items, int n, int what, QualityPlan& q) {
    if (!items || n <= 0 || n > (1 << 20) || what <= 0 || (what & ~(CCD_QUALITY_PSNR | CCD_QUALITY_MS_SSIM))) return CCD_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        const ccd_quality_item& it = items[i];
        if (it.bitdepth < 8 || it.bitdepth > 16) return CCD_ERR_ARG;
        if (it.h < 1 || it.w < 1 || it.ch < 1 || it.cw < 1 || it.h > kQMaxDim || it.w > kQMaxDim || it.ch > kQMaxDim || it.cw > kQMaxDim)
            return CCD_ERR_ARG;
        for (int p = 0; p < 3; ++p) if (!it.dec[p] || !it.src[p]) return CCD_ERR_ARG;
    }
    const size_t np = static_cast<size_t>(n) * 3;
    q.planes.assign(np, QualityPlane{});
    q.pool_off.assign(np * 2 * (kQScales - 1), 0);
    q.sse_prefix.assign(np + 1, 0);
    q.ms_prefix.assign(kQScales * (np + 1), 0);
    size_t at = 0;
    q.off_planes = at; at = align256(at + np * sizeof(QualityPlane));
    q.off_sse_prefix = at; at = align256(at + (np + 1) * sizeof(uint32_t));
    q.off_ms_prefix = at; at = align256(at + kQScales * (np + 1) * sizeof(uint32_t));
    q.head_bytes = at;
    size_t pool_at = 0;  // relative to the start of the pooled pictures, placed last
    uint64_t sse_tiles = 0, ms_tiles[kQScales] = {0};
    for (size_t k = 0; k < np; ++k) {
        const ccd_quality_item& it = items[k / 3];
        const int p = static_cast<int>(k % 3);
        QualityPlane& P = q.planes[k];
        P.dec = it.dec[p];
        P.src = it.src[p];
        P.h = p ? it.ch : it.h;
        P.w = p ? it.cw : it.w;
        P.wide = it.bitdepth > 8;
        P.inv_maxv = 1.0 / static_cast<double>((1 << it.bitdepth) - 1);
        P.n_scales = ((what & CCD_QUALITY_MS_SSIM) && std::min(P.h, P.w) >= kQMinSide) ? kQScales : 0;
        if (what & CCD_QUALITY_PSNR) {
            const size_t bytes = (static_cast<size_t>(P.h) * P.w) << P.wide;
            sse_tiles += (bytes + kQSseBytes - 1) / kQSseBytes;
        }
        for (int j = 0; j < P.n_scales; ++j) {
            const int hj = P.h >> j, wj = P.w >> j;
            ms_tiles[j] += static_cast<uint64_t>((hj - kQWin + kQTile) / kQTile) * ((wj - kQWin + kQTile) / kQTile);
            if (j) {
                for (int s = 0; s < 2; ++s) {
                    q.pool_off[(k * 2 + s) * (kQScales - 1) + (j - 1)] = pool_at;
                    pool_at = align256(pool_at + static_cast<size_t>(hj) * wj * sizeof(float));
                }
            }
        }
        if (sse_tiles > 0x7fffffffu) return CCD_ERR_ARG;
        q.sse_prefix[k + 1] = static_cast<uint32_t>(sse_tiles);
        for (int j = 0; j < kQScales; ++j) {
            if (ms_tiles[j] > 0x0fffffffu) return CCD_ERR_ARG;
            q.ms_prefix[j * (np + 1) + k + 1] = static_cast<uint32_t>(ms_tiles[j]);
        }
    }
    for (int j = 0; j < kQScales; ++j) q.scale_first[j + 1] = q.scale_first[j] + static_cast<uint32_t>(ms_tiles[j]);
    q.off_sse_part = at; at = align256(at + static_cast<size_t>(sse_tiles) * sizeof(uint64_t));
    q.off_ms_part = at; at = align256(at + static_cast<size_t>(q.scale_first[kQScales]) * 2 * sizeof(double));
    q.off_out = at; at = align256(at + np * sizeof(QualityOut));
    for (auto& o : q.pool_off) o += at;
    q.total = at + pool_at;
    return CCD_OK;
}

const double kMsSsimWeights[kQScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
}  // namespace

struct ccd_quality {
    int device = 0;
    Block dev, head_host, out_host;    // scratch (device), its head (pinned), QualityOut[planes] (pinned)
    QualityPlan plan;                  // of the scoring in flight / last finished
    int pending = 0;                   // items of the scoring in flight
    hipStream_t score_stream = nullptr;  // ... and the stream it was enqueued on
    double g[kQWin];
    StreamSet streams;                 // every stream a scoring was enqueued on
};

int64_t ccd_quality_scratch_bytes(const ccd_quality_item* items, int n, int what) {
    QualityPlan q;
    const int rc = quality_plan(items, n, what, q);
    return rc < 0 ? rc : static_cast<int64_t>(q.total);
}

int ccd_quality_create(int device, ccd_quality** out) {
    if (!out) return CCD_ERR_ARG;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return CCD_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    ccd_quality* q = new (std::nothrow) ccd_quality();
    if (!q) return CCD_ERR_NOMEM;
    q->device = device;
    double sum = 0.;
    for (int i = 0; i < kQWin; ++i) { q->g[i] = std::exp(-static_cast<double>((i - 5) * (i - 5)) / (2. * 1.5 * 1.5)); sum += q->g[i]; }
    for (int i = 0; i < kQWin; ++i) q->g[i] /= sum;
    *out = q;
    return CCD_OK;
}

void ccd_quality_destroy(ccd_quality* q) {
    if (!q) return;
    (void)hipSetDevice(q->device);
    (void)q->streams.drain();
    q->dev.drop(); q->head_host.drop(); q->out_host.drop();
    delete q;
}

int ccd_quality_score_batch(ccd_quality* q, const ccd_quality_item* items, int n, int what, void* stream) {
    if (!q || q->pending) return CCD_ERR_ARG;
    QualityPlan& P = q->plan;
    const int rc = quality_plan(items, n, what, P);
    if (rc < 0) return rc;
    HIP_TRY(hipSetDevice(q->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t np = P.planes.size();
    // nothing of an earlier scoring is in flight (its finish synchronised), so the blocks may be exchanged for larger ones
    if (!q->dev.ensure(q->device, BlockPool::kDevice, P.total) || !q->head_host.ensure(q->device, BlockPool::kPinned, P.head_bytes) ||
        !q->out_host.ensure(q->device, BlockPool::kPinned, np * sizeof(QualityOut)))
        return CCD_ERR_NOMEM;
    char* base = q->dev.as<char>();
    for (size_t k = 0; k < np; ++k)
        for (int s = 0; s < 2; ++s)
            for (int j = 0; j + 1 < P.planes[k].n_scales; ++j)
                P.planes[k].pool[s][j] = reinterpret_cast<float*>(base + P.pool_off[(k * 2 + s) * (kQScales - 1) + j]);
    char* head = q->head_host.as<char>();
    std::memcpy(head + P.off_planes, P.planes.data(), np * sizeof(QualityPlane));
    std::memcpy(head + P.off_sse_prefix, P.sse_prefix.data(), P.sse_prefix.size() * sizeof(uint32_t));
    std::memcpy(head + P.off_ms_prefix, P.ms_prefix.data(), P.ms_prefix.size() * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(base, head, P.head_bytes, hipMemcpyHostToDevice, st));
    QualityBatch B;
    std::memset(&B, 0, sizeof(B));
    B.planes = reinterpret_cast<const QualityPlane*>(base + P.off_planes);
    B.n_planes = static_cast<int32_t>(np);
    B.sse_prefix = reinterpret_cast<const uint32_t*>(base + P.off_sse_prefix);
    B.ms_prefix = reinterpret_cast<const uint32_t*>(base + P.off_ms_prefix);
    std::memcpy(B.scale_first, P.scale_first, sizeof(B.scale_first));
    B.sse_part = reinterpret_cast<uint64_t*>(base + P.off_sse_part);
    B.ms_part = reinterpret_cast<double*>(base + P.off_ms_part);
    B.out = reinterpret_cast<QualityOut*>(base + P.off_out);
    std::memcpy(B.g, q->g, sizeof(B.g));
    q->streams.note(st);
    HIP_TRY(launch_quality(B, P.sse_prefix[np], st));
    HIP_TRY(hipMemcpyAsync(q->out_host.p, B.out, np * sizeof(QualityOut), hipMemcpyDeviceToHost, st));
    q->pending = n;
    q->score_stream = st;
    return CCD_OK;
}

int ccd_quality_finish_batch(ccd_quality* q, void* stream, ccd_quality_result* results, int n) {
    if (!q || !results || q->pending <= 0 || n != q->pending) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(q->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    // the results are behind the scoring on the stream the scoring was given, whichever stream this call names
    if (q->score_stream != static_cast<hipStream_t>(stream)) HIP_TRY(hipStreamSynchronize(q->score_stream));
    q->pending = 0;
    const QualityOut* out = q->out_host.as<QualityOut>();
    for (int i = 0; i < n; ++i) {
        ccd_quality_result& R = results[i];
        std::memset(&R, 0, sizeof(R));
        for (int p = 0; p < 3; ++p) {
            const QualityPlane& P = q->plan.planes[static_cast<size_t>(i) * 3 + p];
            const QualityOut& O = out[static_cast<size_t>(i) * 3 + p];
            R.sse[p] = O.sse;
            R.n[p] = static_cast<uint64_t>(P.h) * static_cast<uint64_t>(P.w);
            R.n_scales[p] = P.n_scales;
            for (int j = 0; j < P.n_scales; ++j) {
                const double cnt = static_cast<double>((P.h >> j) - (kQWin - 1)) * static_cast<double>((P.w >> j) - (kQWin - 1));
                R.cs[p][j] = O.cs_sum[j] / cnt;
                R.ssim[p][j] = O.ssim_sum[j] / cnt;
            }
        }
    }
    return CCD_OK;
}

double ccd_quality_psnr(const ccd_quality_result* r, int bitdepth, int plane) {
    if (!r || bitdepth < 8 || bitdepth > 16 || plane < -1 || plane > 2) return std::nan("");
    uint64_t sse = 0, n = 0;
    for (int p = 0; p < 3; ++p)
        if (plane < 0 || plane == p) { sse += r->sse[p]; n += r->n[p]; }
    if (n == 0) return std::nan("");
    const double maxv = static_cast<double>((1 << bitdepth) - 1);
    const double mse = static_cast<double>(sse) / (static_cast<double>(n) * maxv * maxv);
    return -10. * std::log10(mse);  // +inf for identical pictures
}

double ccd_quality_ms_ssim(const ccd_quality_result* r, int plane) {
    if (!r || plane < 0 || plane > 2 || r->n_scales[plane] != kQScales) return std::nan("");
    double v = 1.;
    for (int j = 0; j < kQScales; ++j) {
        const double t = j + 1 < kQScales ? r->cs[plane][j] : r->ssim[plane][j];
        v *= std::pow(std::max(t, 0.), kMsSsimWeights[j]);
    }
    return v;
}

}  // extern "C"
