// ccd_enc_api.cpp - ccd_enc_* of include/ccd.h: the host side of the device writer.
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>

#include "ccd_host.hpp"
#include "ccd_kernels.hpp"
#include "ccd_wavefront.hpp"

using namespace ccd;

extern "C" {

// ---- device writer (ccd_encode.hip) ---------------------------------------------------------
namespace {
constexpr int kEncStatusWords = 8;  // per slot: error, words written, inverted runs begun, resolved with / without a carry

struct EncSlot {
    ccd_cc_header hdr;             // re-derived from the template, nn_n_bytes = size of `nn`
    std::vector<uint8_t> nn;
    EncodeParams ep;               // ep.ep.status is set when the handle's table is built
    Block params;                  // device: ARM | IFCE | step prefix tables | latents given as host pointers
    Block pairs, out;
    bool ran = false;              // part of a run that was waited for
    int status = CCD_OK;
    uint32_t n_words = 0;
    bool measured = false;         // part of a measure that was waited for; `rate` and `map_off` are that measure's
    ccd_enc_rate rate{};
    size_t map_off = 0;            // floats before this slot's planes in the handle's map block
    size_t delta_off = 0;          // floats before this slot's delta maps in the handle's delta map block
    // ARM parameter deltas (ccd_enc_measure_param_deltas)
    ArmDeltaShape arm_shape{};
    std::vector<int64_t> arm_ints; // the ARM's transmitted integers, stream order
    int param_first = 0, param_count = 0;  // the range the last table covers, clipped to this slot
    size_t param_off = 0;          // candidates before this slot's in the handle's tables
    // IFCE parameter deltas (ccd_enc_measure_ifce_deltas): the same three fields above hold its range when the table is its
    IfceDeltaShape ifce_shape{};
    std::vector<int64_t> ifce_ints;  // the IFCE's transmitted integers, stream order (empty: no grid has IFCE)
};
enum { kIdle = 0, kRun = 1, kMeasure = 2 };  // what ccd_enc::in_flight holds
}  // namespace

struct ccd_enc {
    int device = 0;
    DeviceShared* sh = nullptr;
    std::vector<std::unique_ptr<EncSlot>> slots;
    Mirror table, status;          // EncodeParams[n], int32 [n][8]
    size_t table_slots = 0;        // slots the two above describe
    hipStream_t last_stream = nullptr;
    int in_flight = kIdle;         // one run OR one measure at a time
    int last_kind = kRun;          // what the last wait ended: whose per-slot errors an idle wait reports
    size_t n_run = 0;              // slots of the run in flight / last waited for
    // the rate meter's own buffers: a run and a measure never write to the same place
    Mirror rate_table, rate_out;   // RateParams[n]; per slot RateGrid[n_grids] + total, then int32 status [n]
    Block rate_slab, rate_map;     // partials; the planes of a map
    size_t rate_slots = 0, rate_out_bytes = 0, rate_status_off = 0;
    bool rate_has_map = false;     // rate_table describes a map (the last measure asked for one)
    size_t n_measured = 0;         // slots of the measure in flight / last waited for
    bool map_valid = false;        // the last finished measure wrote a map
    // rate sensitivity (ccd_enc_measure_deltas): a measure whose two extra launches write here
    Mirror delta_table;            // DeltaParams[n]
    Block delta_slab, delta_map;   // f64 cells, f32 [2][h][w] per grid
    size_t delta_slots = 0;        // slots the three above describe
    bool delta_pending = false;    // the measure in flight is a measure_deltas
    bool delta_valid = false;      // the last finished measure was one
    // ARM parameter deltas (ccd_enc_measure_param_deltas): a measure whose two extra launches write here
    Mirror param_table, param_out; // RateDeltaParams[n], every slot's candidates and the IFCE table's rows; one ParamDeltaCell per candidate
    Block param_slab;              // the chunks' cells
    bool param_pending = false;    // the measure in flight is a measure_param_deltas
    bool param_valid = false;      // the last finished measure was one
    int param_pending_kind = kRateDeltaArm, param_kind = kRateDeltaArm;  // kRateDeltaArm / kRateDeltaIfce: of the table in flight / of the valid one
    StreamSet streams;             // every stream a run was enqueued on
};

size_t ccd_enc_payload_bound(int64_t n_symbols) {
    if (n_symbols < 0) return 0;
    // the leaky model gives every symbol at least 1 / 2^24 of the interval: at most 24 bits each, plus the two words of the seal
    return 4 * ((static_cast<size_t>(n_symbols) * kRcPrecision + 31) / 32 + 2);
}

int ccd_enc_create(int device, ccd_enc** out) {
    if (!out) return CCD_ERR_ARG;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return CCD_ERR_HIP;
    HIP_TRY(hipSetDevice(device));
    DeviceShared* sh = nullptr;
    const int rc = device_shared(device, &sh);
    if (rc < 0) return rc;
    ccd_enc* e = new (std::nothrow) ccd_enc();
    if (!e) return CCD_ERR_NOMEM;
    e->device = device;
    e->sh = sh;
    *out = e;
    return CCD_OK;
}

void ccd_enc_destroy(ccd_enc* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)e->streams.drain();
    for (auto& s : e->slots) { s->params.drop(); s->pairs.drop(); s->out.drop(); }
    e->table.drop(); e->status.drop();
    e->rate_table.drop(); e->rate_slab.drop(); e->rate_out.drop(); e->rate_map.drop();
    e->delta_table.drop(); e->delta_slab.drop(); e->delta_map.drop();
    e->param_table.drop(); e->param_out.drop(); e->param_slab.drop();
    delete e;
}

int ccd_enc_size(const ccd_enc* e) { return e ? static_cast<int>(e->slots.size()) : CCD_ERR_ARG; }

int ccd_enc_add(ccd_enc* e, const ccd_cc_header* tmpl, const uint8_t* bytes_nn, size_t n_nn, const int8_t* const* latents,
                int latents_on_device) {
    if (!e || !tmpl || !bytes_nn || !latents) return CCD_ERR_ARG;
    std::unique_ptr<EncSlot> sp(new (std::nothrow) EncSlot());
    if (!sp) return CCD_ERR_NOMEM;
    EncSlot& s = *sp;
    // ---- everything the host can refuse, before the device is touched ----
    if (rederive_cc_header(*tmpl, n_nn, &s.hdr) < 0) return CCD_ERR_VALUE;
    const ccd_cc_header& h = s.hdr;
    if (!grids_nest(h)) return CCD_ERR_VALUE;
    Network net;
    int rc = decode_network(h, bytes_nn, n_nn, net);
    if (rc < 0) return rc;
    const int n = h.n_grids;
    for (int g = 0; g < n; ++g) if (!latents[g]) return CCD_ERR_ARG;
    if (h.n_symbols < 0 || h.n_symbols > 0x7fffffff) return CCD_ERR_UNSUPPORTED;
    if (!latents_on_device)
        for (int g = 0; g < n; ++g) {
            const size_t cnt = static_cast<size_t>(h.grid_h[g]) * h.grid_w[g];
            for (size_t i = 0; i < cnt; ++i)
                if (latents[g][i] < kAcLo || latents[g][i] > kAcLo + kAlphabet - 1) return CCD_ERR_VALUE;
        }
    IntNetBlobs blobs;
    pack_int_networks(h, net, blobs);
    EncodeParams& Q = s.ep;
    std::memset(&Q, 0, sizeof(Q));
    EntropyParams& E = Q.ep;
    fill_entropy_model(h, net, blobs, E);
    {   // the shapes the kernel indexes by: dim x dim hidden layers, dim x 2 output and stabiliser, one IFCE layer per grid
        const int dim = E.dim, n_if = E.has_ifce ? E.n_ifce_out : 0;
        bool ok = dim >= 1 && dim == E.n_spatial + n_if && E.n_spatial <= kMaxCtx && net.arm.dim == dim &&
                  static_cast<int>(net.arm.layers.size()) == E.n_layers &&
                  E.arm_len == (E.n_layers - 1) * (dim * dim + dim) + 2 * (2 * dim + 2) &&
                  encode_contexts_lds_bytes(dim) <= 160 * 1024;
        for (int g = 0; g < n && ok; ++g) {
            const int fin = E.ifce_in[g];
            if (fin == 0) continue;
            ok = n_if > 0 && (g == n - 1 || g + fin < n) && net.ifce[g].layers.size() == 1 &&
                 static_cast<int>(net.ifce[g].layers[0].w.size()) == fin * n_if &&
                 static_cast<int>(net.ifce[g].layers[0].b.size()) == n_if;
        }
        if (!ok) return CCD_ERR_UNSUPPORTED;
    }
    // ---- where every pixel goes: grids n-1 .. 0, each in coding order (ccd_wavefront.hpp); wavefront grids get a table of
    // the pixels in front of every step ----
    const uint32_t threads = static_cast<uint32_t>(encode_block_threads());
    std::vector<std::vector<uint32_t>> prefix(n);
    uint32_t first = 0;
    for (int g = n - 1; g >= 0; --g) {
        const int H = h.grid_h[g], W = h.grid_w[g];
        Q.grid_first[g] = first;
        first += static_cast<uint32_t>(H) * static_cast<uint32_t>(W);
        if (wf_raster(W) || H < 1) continue;
        const int n_steps = wf_n_steps(H, W);
        prefix[g].resize(static_cast<size_t>(n_steps));
        uint32_t before = 0;
        for (int c = 0; c < n_steps; ++c) {
            int y0, x0;
            prefix[g][static_cast<size_t>(c)] = before;
            before += static_cast<uint32_t>(wf_step(H, W, c, y0, x0));
        }
    }
    Q.n_symbols = first;
    uint32_t blocks = 0;
    for (int g = 0; g < n; ++g) {
        Q.block_first[g] = blocks;
        blocks += (static_cast<uint32_t>(h.grid_h[g]) * static_cast<uint32_t>(h.grid_w[g]) + threads - 1) / threads;
    }
    Q.n_blocks = blocks;
    Q.cap_words = static_cast<uint32_t>(ccd_enc_payload_bound(first) / 4);

    // ---- device image: ARM | IFCE | step prefix tables | host latents ----
    TableImage img;
    const size_t o_arm = img.put(blobs.arm), o_ifce = img.put(blobs.ifce);
    std::vector<size_t> o_prefix(n, 0), o_lat(n, 0);
    for (int g = 0; g < n; ++g) o_prefix[g] = img.put(prefix[g]);
    if (!latents_on_device)
        for (int g = 0; g < n; ++g) o_lat[g] = img.put(latents[g], static_cast<size_t>(h.grid_h[g]) * h.grid_w[g]);
    std::vector<char>& image = img.bytes;
    image.resize(std::max<size_t>(align256(image.size()), 256));  // whole 256-byte units, never empty

    HIP_TRY(hipSetDevice(e->device));
    auto fail = [&](int code) { s.params.drop(); s.pairs.drop(); s.out.drop(); return code; };
    if (!s.params.get(e->device, BlockPool::kDevice, image.size()) ||
        !s.pairs.get(e->device, BlockPool::kDevice, std::max<size_t>(static_cast<size_t>(first) * sizeof(EncodePair), 256)) ||
        !s.out.get(e->device, BlockPool::kDevice, static_cast<size_t>(Q.cap_words) * 4))
        return fail(CCD_ERR_NOMEM);
    if (hipMemcpy(s.params.p, image.data(), image.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(CCD_ERR_HIP);
    char* base = s.params.as<char>();
    E.arm = reinterpret_cast<const int64_t*>(base + o_arm);
    E.ifce = reinterpret_cast<const int64_t*>(base + o_ifce);
    E.scale_table = e->sh->d_scale_table;
    E.rcp_table = e->sh->d_rcp_table;
    for (int g = 0; g < n; ++g) {
        E.latent[g] = latents_on_device ? const_cast<int8_t*>(latents[g]) : reinterpret_cast<int8_t*>(base + o_lat[g]);  // read-only here
        Q.step_prefix[g] = prefix[g].empty() ? nullptr : reinterpret_cast<const uint32_t*>(base + o_prefix[g]);
    }
    Q.pairs = s.pairs.as<EncodePair>();
    Q.out = s.out.as<uint32_t>();
    s.nn.assign(bytes_nn, bytes_nn + n_nn);
    s.arm_shape = armdelta_shape(h);
    s.arm_ints.assign(net.ints.begin(), net.ints.begin() + std::min<int64_t>(armdelta_count(s.arm_shape), static_cast<int64_t>(net.ints.size())));
    s.ifce_shape = ifcedelta_shape(h);
    {   // groups 2 and 3 follow the ARM's two in the stream
        const int64_t lo = static_cast<int64_t>(s.arm_ints.size()), total = static_cast<int64_t>(net.ints.size());
        s.ifce_ints.assign(net.ints.begin() + lo, net.ints.begin() + std::min<int64_t>(lo + ifcedelta_count(s.ifce_shape), total));
    }
    e->slots.push_back(std::move(sp));
    return static_cast<int>(e->slots.size()) - 1;
}

namespace {
// Takes in what the run or measure in flight left in the pinned buffers; the caller has synchronised its stream.
void harvest(ccd_enc* e) {
    if (e->in_flight == kRun) {
        const int32_t* hs = e->status.host.as<int32_t>();
        for (size_t i = 0; i < e->n_run; ++i) {
            EncSlot& s = *e->slots[i];
            s.ran = true;
            s.status = hs[i * kEncStatusWords];
            s.n_words = s.status == CCD_OK ? static_cast<uint32_t>(hs[i * kEncStatusWords + 1]) : 0;
        }
    } else if (e->in_flight == kMeasure) {
        const char* out = e->rate_out.host.as<char>();
        const int32_t* hs = reinterpret_cast<const int32_t*>(out + e->rate_status_off);
        size_t off = 0;
        for (size_t i = 0; i < e->n_measured; ++i) {
            EncSlot& s = *e->slots[i];
            const int n = s.hdr.n_grids;
            ccd_enc_rate& r = s.rate;
            std::memset(&r, 0, sizeof(r));
            r.status = hs[i];
            r.n_grids = n;
            r.n_bytes_nn = static_cast<int64_t>(s.nn.size());
            r.n_bytes_header = s.hdr.n_bytes_header;
            if (r.status == CCD_OK) {  // a slot with an error reports no numbers
                const RateGrid* rg = reinterpret_cast<const RateGrid*>(out + off);
                for (int g = 0; g < n; ++g) { r.n_symbols[g] = rg[g].n_symbols; r.sum_width[g] = rg[g].sum_width; r.bits[g] = rg[g].bits; }
                std::memcpy(&r.total_bits, rg + n, sizeof(double));
            }
            off += static_cast<size_t>(n) * sizeof(RateGrid) + sizeof(double);
            s.measured = true;
        }
        e->map_valid = e->rate_has_map;
        e->delta_valid = e->delta_pending;
        e->delta_pending = false;
        e->param_valid = e->param_pending;
        e->param_kind = e->param_pending_kind;
        e->param_pending = false;
    }
    e->last_kind = e->in_flight;
    e->in_flight = kIdle;
}

// What run and measure share: at most one of them in flight, and the EncodeParams table of the handle's slots.
int prepare_launch(ccd_enc* e, hipStream_t st, unsigned* max_blocks, size_t* lds) {
    const size_t n = e->slots.size();
    HIP_TRY(hipSetDevice(e->device));
    if (e->in_flight != kIdle) {  // its tables are about to be reused
        HIP_TRY(hipStreamSynchronize(e->last_stream));
        harvest(e);
    }
    if (e->table_slots != n) {  // (the blocks only grow; the loop below rewrites every entry of the table, so what a kept block held is gone)
        e->table_slots = 0;
        if (!e->table.ensure(e->device, n * sizeof(EncodeParams)) || !e->status.ensure(e->device, n * kEncStatusWords * sizeof(int32_t)))
            return CCD_ERR_NOMEM;
        for (size_t i = 0; i < n; ++i) {
            e->slots[i]->ep.ep.status = e->status.dev.as<int32_t>() + i * kEncStatusWords;
            e->table.host.as<EncodeParams>()[i] = e->slots[i]->ep;
        }
        e->table_slots = n;
    }
    *max_blocks = 0;
    *lds = 0;
    for (auto& s : e->slots) {
        *max_blocks = std::max<unsigned>(*max_blocks, s->ep.n_blocks);
        *lds = std::max(*lds, encode_contexts_lds_bytes(s->ep.ep.dim));
    }
    HIP_TRY(e->table.upload(n * sizeof(EncodeParams), st));
    return CCD_OK;
}

void launched(ccd_enc* e, hipStream_t st, int kind) {
    e->last_stream = st;
    e->in_flight = kind;
    e->streams.note(st);
}
}  // namespace

int ccd_enc_run(ccd_enc* e, void* stream) {
    if (!e) return CCD_ERR_ARG;
    const size_t n = e->slots.size();
    if (n == 0) return CCD_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned max_blocks = 0;
    size_t lds = 0;
    const int rc = prepare_launch(e, st, &max_blocks, &lds);
    if (rc < 0) return rc;
    HIP_TRY(hipMemsetAsync(e->status.dev.p, 0, n * kEncStatusWords * sizeof(int32_t), st));
    HIP_TRY(launch_encode(e->table.dev.as<EncodeParams>(), static_cast<int>(n), max_blocks, lds, st));
    HIP_TRY(e->status.download(n * kEncStatusWords * sizeof(int32_t), st));
    e->n_run = n;
    launched(e, st, kRun);
    return CCD_OK;
}

namespace {
// The meter's launches and the copy of its results, enqueued on `st`: what ccd_enc_measure and ccd_enc_measure_deltas share.
int enqueue_measure(ccd_enc* e, hipStream_t st, bool map, unsigned* max_blocks_out, size_t* lds_out) {
    const size_t n = e->slots.size();
    unsigned max_blocks = 0;
    size_t lds = 0;
    const int rc = prepare_launch(e, st, &max_blocks, &lds);
    if (rc < 0) return rc;
    *max_blocks_out = max_blocks;
    *lds_out = lds;
    e->map_valid = false;  // the planes of the last measure are about to be overwritten or given back
    e->delta_valid = false;
    e->param_valid = false;
    if (e->rate_slots != n || e->rate_has_map != map) {
        e->rate_slots = 0;
        size_t n_blocks = 0, out_bytes = 0, n_map = 0;
        for (auto& s : e->slots) {
            n_blocks += s->ep.n_blocks;
            out_bytes += static_cast<size_t>(s->hdr.n_grids) * sizeof(RateGrid) + sizeof(double);
            n_map += s->ep.n_symbols;
        }
        e->rate_status_off = out_bytes;
        e->rate_out_bytes = out_bytes + n * sizeof(int32_t);
        if (!map) e->rate_map.drop();
        // (grow only: every entry of the table is rewritten below and the results are cleared before each launch)
        if (!e->rate_table.ensure(e->device, n * sizeof(RateParams)) ||
            !e->rate_slab.ensure(e->device, BlockPool::kDevice, std::max<size_t>(n_blocks * sizeof(RatePartial), 256)) ||
            !e->rate_out.ensure(e->device, e->rate_out_bytes) ||
            (map && !e->rate_map.ensure(e->device, BlockPool::kDevice, std::max<size_t>(n_map * sizeof(float), 256))))
            return CCD_ERR_NOMEM;
        size_t block = 0, off = 0, cell = 0;
        for (size_t i = 0; i < n; ++i) {
            EncSlot& s = *e->slots[i];
            RateParams& R = e->rate_table.host.as<RateParams>()[i];
            std::memset(&R, 0, sizeof(R));
            R.partial = e->rate_slab.as<RatePartial>() + block;
            R.grids = reinterpret_cast<RateGrid*>(e->rate_out.dev.as<char>() + off);
            R.status = reinterpret_cast<int32_t*>(e->rate_out.dev.as<char>() + e->rate_status_off) + i;
            s.map_off = cell;
            for (int g = 0; g < s.hdr.n_grids; ++g) {
                if (map) R.map[g] = e->rate_map.as<float>() + cell;
                cell += static_cast<size_t>(s.hdr.grid_h[g]) * s.hdr.grid_w[g];
            }
            block += s.ep.n_blocks;
            off += static_cast<size_t>(s.hdr.n_grids) * sizeof(RateGrid) + sizeof(double);
        }
        e->rate_slots = n;
        e->rate_has_map = map;
    }
    int max_grids = 0;
    for (auto& s : e->slots) max_grids = std::max<int>(max_grids, s->hdr.n_grids);
    HIP_TRY(e->rate_table.upload(n * sizeof(RateParams), st));
    HIP_TRY(hipMemsetAsync(e->rate_out.dev.p, 0, e->rate_out_bytes, st));
    HIP_TRY(launch_encode_rate(e->table.dev.as<EncodeParams>(), e->rate_table.dev.as<RateParams>(), static_cast<int>(n), max_blocks, max_grids, lds, st));
    HIP_TRY(e->rate_out.download(e->rate_out_bytes, st));
    e->n_measured = n;
    return CCD_OK;
}
}  // namespace

int ccd_enc_measure(ccd_enc* e, void* stream, int want_map) {
    if (!e) return CCD_ERR_ARG;
    if (e->slots.empty()) return CCD_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned max_blocks = 0;
    size_t lds = 0;
    const int rc = enqueue_measure(e, st, want_map != 0, &max_blocks, &lds);
    if (rc < 0) return rc;
    launched(e, st, kMeasure);
    return CCD_OK;
}

int ccd_enc_measure_deltas(ccd_enc* e, void* stream) {
    if (!e) return CCD_ERR_ARG;
    const size_t n = e->slots.size();
    if (n == 0) return CCD_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    if (e->in_flight != kIdle) {  // the delta tables below may be rebuilt: nothing of this handle may still read them
        HIP_TRY(hipStreamSynchronize(e->last_stream));
        harvest(e);
    }
    e->delta_valid = false;  // the maps of the last call are about to be overwritten or given back
    // which fine grids have IFCE sources, their tiles and their cells: the geometry the kernels re-derive (ccd_device.hpp)
    auto has_sources = [](const EntropyParams& E, int g) { return E.ifce_in[g] > 0 && g != E.n_grids - 1; };
    if (e->delta_slots != n) {
        e->delta_slots = 0;
        size_t n_cells = 0, n_map = 0;
        for (auto& s : e->slots) {
            const EntropyParams& E = s->ep.ep;
            for (int g = 0; g < E.n_grids; ++g) {
                if (!has_sources(E, g)) continue;
                for (int c = 0; c < E.ifce_in[g]; ++c)
                    n_cells += 2 * static_cast<size_t>(delta_cells(E.grid_h[g], E.grid_w[g], delta_cell_shift(E.level[g + 1 + c] - E.level[g + 1])));
            }
            n_map += 2 * static_cast<size_t>(s->ep.n_symbols);
        }
        if (n_cells > 0xffffffffu) return CCD_ERR_UNSUPPORTED;
        if (!e->delta_table.ensure(e->device, n * sizeof(DeltaParams)) ||  // (grow only: every entry is rewritten below)
            !e->delta_slab.ensure(e->device, BlockPool::kDevice, std::max<size_t>(n_cells * sizeof(double), 256)) ||
            !e->delta_map.ensure(e->device, BlockPool::kDevice, std::max<size_t>(n_map * sizeof(float), 256)))
            return CCD_ERR_NOMEM;
        size_t cell = 0, at = 0;
        for (size_t i = 0; i < n; ++i) {
            EncSlot& s = *e->slots[i];
            const EntropyParams& E = s.ep.ep;
            DeltaParams& D = e->delta_table.host.as<DeltaParams>()[i];
            std::memset(&D, 0, sizeof(D));
            D.partial = e->delta_slab.as<double>() + cell;
            s.delta_off = at;
            uint32_t first = 0, tiles = 0;
            for (int g = 0; g < E.n_grids; ++g) {
                const int H = E.grid_h[g], W = E.grid_w[g];
                D.part_first[g] = first;
                D.tile_first[g] = tiles;
                D.map[g] = e->delta_map.as<float>() + at;
                at += 2 * static_cast<size_t>(H) * W;
                if (!has_sources(E, g)) continue;
                for (int c = 0; c < E.ifce_in[g]; ++c) first += 2 * delta_cells(H, W, delta_cell_shift(E.level[g + 1 + c] - E.level[g + 1]));
                tiles += delta_cells(H, W, kDeltaTileLog);
            }
            D.n_tiles = tiles;
            cell += first;
        }
        e->delta_slots = n;
    }
    unsigned max_blocks = 0;
    size_t lds = 0;
    const int rc = enqueue_measure(e, st, false, &max_blocks, &lds);  // the meter's two launches first: its results are its own
    if (rc < 0) return rc;
    launched(e, st, kMeasure);
    unsigned max_tiles = 0;
    for (size_t i = 0; i < n; ++i) max_tiles = std::max<unsigned>(max_tiles, e->delta_table.host.as<DeltaParams>()[i].n_tiles);
    HIP_TRY(e->delta_table.upload(n * sizeof(DeltaParams), st));
    HIP_TRY(launch_encode_deltas(e->table.dev.as<EncodeParams>(), e->delta_table.dev.as<DeltaParams>(), static_cast<int>(n), max_blocks, max_tiles, lds, st));
    e->delta_pending = true;
    return CCD_OK;
}

namespace {
// ccd_enc_measure_param_deltas (kind == kRateDeltaArm) and ccd_enc_measure_ifce_deltas (kRateDeltaIfce): the range, the refusals, the
// cells, the candidates and the meter's launches in front are the same; the integers, their places, the incremental path's LDS,
// the order of the candidates (the IFCE's are sorted by grid) and the kernel's instantiation are the kind's.
int measure_table(ccd_enc* e, void* stream, int first, int count, int mode, int kind) {
    if (!e || first < 0 || mode < kArmDeltaAuto || mode > kArmDeltaIncremental) return CCD_ERR_ARG;
    const bool ifce = kind == kRateDeltaIfce;
    const size_t n = e->slots.size();
    if (n == 0) return CCD_OK;
    // ---- everything the host can refuse, before the device is touched: the path of every slot, the launch's dimensions ----
    if (n > 65535) return CCD_ERR_UNSUPPORTED;
    std::vector<std::pair<int, int>> range(n);  // first, count per slot: the range asked for, clipped
    size_t n_cand = 0, n_cells = 0;
    unsigned max_cand = 0, max_chunks = 0;
    std::vector<int> path(n);
    size_t lds_generic = 0, lds_incremental = 0;  // 0: no slot takes that path
    for (size_t i = 0; i < n; ++i) {
        const EncSlot& s = *e->slots[i];
        const int64_t n_arm = static_cast<int64_t>((ifce ? s.ifce_ints : s.arm_ints).size());  // the integers of the kind
        if (ifce && n_arm == 0) {  // nothing to price by either path: the slot refuses no mode and asks for no LDS
            range[i] = {0, 0};
            path[i] = kArmDeltaGeneric;
            continue;
        }
        const int64_t lds_inc = ifce ? ifcedelta_incremental_lds(s.ifce_shape) : armdelta_incremental_lds(s.arm_shape);
        const int rc = ratedelta_path(lds_inc, mode);
        if (rc < 0) return rc;
        path[i] = rc;
        if (rc == kArmDeltaIncremental) lds_incremental = std::max(lds_incremental, static_cast<size_t>(lds_inc));
        else lds_generic = std::max(lds_generic, encode_contexts_lds_bytes(s.ep.ep.dim));
        const int64_t lo = std::min<int64_t>(first, n_arm), hi = count < 0 ? n_arm : std::min<int64_t>(static_cast<int64_t>(first) + count, n_arm);
        range[i] = {static_cast<int>(lo), static_cast<int>(hi - lo)};
        const size_t cand = 2 * static_cast<size_t>(hi - lo);
        const size_t chunks = (s.ep.n_blocks + kArmDeltaChunkBlocks - 1) / kArmDeltaChunkBlocks;
        if ((cand + kArmDeltaTile - 1) / kArmDeltaTile > 65535) return CCD_ERR_UNSUPPORTED;
        n_cand += cand;
        n_cells += cand * chunks;
        max_cand = std::max<unsigned>(max_cand, static_cast<unsigned>(cand));
        max_chunks = std::max<unsigned>(max_chunks, static_cast<unsigned>(chunks));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(e->device));
    if (e->in_flight != kIdle) {  // the tables below are rebuilt: nothing of this handle may still read them
        HIP_TRY(hipStreamSynchronize(e->last_stream));
        harvest(e);
    }
    e->param_valid = false;  // the table of the last call is about to be overwritten: a failure from here on leaves no table
    const size_t n_cand1 = std::max<size_t>(n_cand, 1);
    const size_t cand_at = align256(n * sizeof(RateDeltaParams));
    const size_t row_at = cand_at + align256(n_cand1 * sizeof(RateDeltaMove));  // the IFCE table's rows
    const size_t table_bytes = row_at + (ifce ? n_cand1 * sizeof(uint32_t) : 0);
    const size_t out_bytes = n_cand1 * sizeof(ParamDeltaCell);
    if (!e->param_table.ensure(e->device, table_bytes) || !e->param_out.ensure(e->device, out_bytes) ||
        !e->param_slab.ensure(e->device, BlockPool::kDevice, std::max<size_t>(n_cells * sizeof(ParamDeltaCell), 256)))
        return CCD_ERR_NOMEM;
    RateDeltaParams* tab = e->param_table.host.as<RateDeltaParams>();
    RateDeltaMove* cands = reinterpret_cast<RateDeltaMove*>(e->param_table.host.as<char>() + cand_at);
    uint32_t* rows = reinterpret_cast<uint32_t*>(e->param_table.host.as<char>() + row_at);
    const RateDeltaMove* d_cands = reinterpret_cast<const RateDeltaMove*>(e->param_table.dev.as<char>() + cand_at);
    const uint32_t* d_rows = reinterpret_cast<const uint32_t*>(e->param_table.dev.as<char>() + row_at);
    size_t at = 0, cell = 0;
    std::vector<RateDeltaMove> unsorted;
    for (size_t i = 0; i < n; ++i) {
        const EncSlot& s = *e->slots[i];
        const std::vector<int64_t>& ints = ifce ? s.ifce_ints : s.arm_ints;
        const int p_first = range[i].first;
        const uint32_t cand = 2 * static_cast<uint32_t>(range[i].second);
        const uint32_t chunks = (s.ep.n_blocks + kArmDeltaChunkBlocks - 1) / kArmDeltaChunkBlocks;
        unsorted.resize(ifce ? cand : 0);
        RateDeltaMove* moves = ifce ? unsorted.data() : cands + at;  // the ARM's candidate c is row c: made in place
        for (uint32_t c = 0; c < cand; ++c) {
            const int64_t k = p_first + (c >> 1);
            int64_t index = 0;
            int shift = 0;
            int rc = ifce ? ifcedelta_place(s.ifce_shape, k, &moves[c], &index, &shift) : armdelta_place(s.arm_shape, k, &moves[c], &index, &shift);
            if (rc == CCD_OK) rc = ratedelta_move((c & 1) ? 1 : -1, ints[static_cast<size_t>(k)], shift, &moves[c]);
            if (rc < 0) return rc;  // (cannot happen: decode_network took these shifts)
        }
        if (ifce) {  // sorted by grid, rows in order inside a grid: a counting sort over the grids
            uint32_t next[CCD_MAX_GRIDS + 1] = {0};
            for (uint32_t c = 0; c < cand; ++c) ++next[moves[c].at + 1];
            for (int g = 0; g < CCD_MAX_GRIDS; ++g) next[g + 1] += next[g];
            for (uint32_t c = 0; c < cand; ++c) {
                const uint32_t j = next[moves[c].at]++;
                cands[at + j] = moves[c];
                rows[at + j] = c;
            }
        }
        tab[i] = RateDeltaParams{d_cands + at, ifce ? d_rows + at : nullptr, e->param_slab.as<ParamDeltaCell>() + cell,
                                 e->param_out.dev.as<ParamDeltaCell>() + at, cand, chunks, path[i], 0};
        at += cand;
        cell += static_cast<size_t>(cand) * chunks;
    }
    unsigned max_blocks = 0;
    size_t lds = 0;
    const int rc = enqueue_measure(e, st, false, &max_blocks, &lds);  // the meter's two launches first: its results are its own
    if (rc < 0) return rc;
    launched(e, st, kMeasure);
    {   // the slots learn their rows only now that the measure is under way
        size_t at = 0;
        for (size_t i = 0; i < n; ++i) {
            EncSlot& s = *e->slots[i];
            s.param_first = range[i].first;
            s.param_count = range[i].second;
            s.param_off = at;
            at += 2 * static_cast<size_t>(s.param_count);
        }
    }
    HIP_TRY(e->param_table.upload(table_bytes, st));
    HIP_TRY(launch_encode_rate_deltas(kind, e->table.dev.as<EncodeParams>(), e->param_table.dev.as<RateDeltaParams>(), static_cast<int>(n), max_chunks,
                                      max_cand, lds_generic, lds_incremental, st));
    HIP_TRY(e->param_out.download(out_bytes, st));
    e->param_pending = true;
    e->param_pending_kind = kind;
    return CCD_OK;
}

// The rows of the valid table when it is of `kind`; CCD_ERR_ARG when the last measure left the other kind's or none.
int slot_table(const ccd_enc* e, int slot, int kind, int* first, int* count, double* bits, int64_t* sum_width, int64_t* moved) {
    if (!e || slot < 0 || slot >= static_cast<int>(e->slots.size()) || e->in_flight == kMeasure || !e->param_valid || e->param_kind != kind ||
        static_cast<size_t>(slot) >= e->n_measured || !e->slots[slot]->measured)
        return CCD_ERR_ARG;
    const EncSlot& s = *e->slots[slot];
    if (s.rate.status < 0) return s.rate.status;
    if (first) *first = s.param_first;
    if (count) *count = s.param_count;
    const ParamDeltaCell* cell = e->param_out.host.as<ParamDeltaCell>() + s.param_off;
    for (int c = 0; c < 2 * s.param_count; ++c) {
        if (bits) bits[c] = cell[c].bits;
        if (sum_width) sum_width[c] = cell[c].sum_width;
        if (moved) moved[c] = cell[c].moved;
    }
    return CCD_OK;
}
}  // namespace

int ccd_enc_measure_param_deltas(ccd_enc* e, void* stream, int first, int count, int mode) { return measure_table(e, stream, first, count, mode, kRateDeltaArm); }
int ccd_enc_measure_ifce_deltas(ccd_enc* e, void* stream, int first, int count, int mode) { return measure_table(e, stream, first, count, mode, kRateDeltaIfce); }

int ccd_enc_slot_param_count(const ccd_enc* e, int slot) {
    if (!e || slot < 0 || slot >= static_cast<int>(e->slots.size())) return CCD_ERR_ARG;
    return static_cast<int>(e->slots[slot]->arm_ints.size());
}
int ccd_enc_slot_ifce_count(const ccd_enc* e, int slot) {
    if (!e || slot < 0 || slot >= static_cast<int>(e->slots.size())) return CCD_ERR_ARG;
    return static_cast<int>(e->slots[slot]->ifce_ints.size());
}

int ccd_enc_slot_param_deltas(const ccd_enc* e, int slot, int* first, int* count, double* bits, int64_t* sum_width, int64_t* moved) {
    return slot_table(e, slot, kRateDeltaArm, first, count, bits, sum_width, moved);
}
int ccd_enc_slot_ifce_deltas(const ccd_enc* e, int slot, int* first, int* count, double* bits, int64_t* sum_width, int64_t* moved) {
    return slot_table(e, slot, kRateDeltaIfce, first, count, bits, sum_width, moved);
}

int ccd_enc_wait(ccd_enc* e, void* stream) {
    if (!e) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (e->in_flight != kIdle) {
        if (e->last_stream != static_cast<hipStream_t>(stream)) HIP_TRY(hipStreamSynchronize(e->last_stream));
        harvest(e);
    }
    if (e->last_kind == kMeasure) {
        for (size_t i = 0; i < e->n_measured; ++i) if (e->slots[i]->rate.status < 0) return e->slots[i]->rate.status;
        return CCD_OK;
    }
    for (size_t i = 0; i < e->n_run; ++i) if (e->slots[i]->status < 0) return e->slots[i]->status;
    return CCD_OK;
}

int ccd_enc_slot_rate(const ccd_enc* e, int slot, ccd_enc_rate* out) {
    if (!e || !out || slot < 0 || slot >= static_cast<int>(e->slots.size()) || e->in_flight == kMeasure || !e->slots[slot]->measured)
        return CCD_ERR_ARG;
    *out = e->slots[slot]->rate;
    return out->status;
}

int64_t ccd_enc_slot_rate_map(const ccd_enc* e, int slot, int grid, const float** device_ptr) {
    if (!e || !device_ptr || slot < 0 || slot >= static_cast<int>(e->slots.size()) || e->in_flight == kMeasure || !e->map_valid ||
        static_cast<size_t>(slot) >= e->n_measured || !e->slots[slot]->measured)
        return CCD_ERR_ARG;
    const EncSlot& s = *e->slots[slot];
    if (grid < 0 || grid >= s.hdr.n_grids) return CCD_ERR_ARG;
    if (s.rate.status < 0) return s.rate.status;
    size_t off = s.map_off;
    for (int g = 0; g < grid; ++g) off += static_cast<size_t>(s.hdr.grid_h[g]) * s.hdr.grid_w[g];
    *device_ptr = e->rate_map.as<float>() + off;
    return static_cast<int64_t>(s.hdr.grid_h[grid]) * s.hdr.grid_w[grid];
}

int ccd_enc_slot_delta_map(const ccd_enc* e, int slot, int grid, void** dev_ptr) {
    if (!e || !dev_ptr || slot < 0 || slot >= static_cast<int>(e->slots.size()) || e->in_flight == kMeasure || !e->delta_valid ||
        static_cast<size_t>(slot) >= e->n_measured || !e->slots[slot]->measured)
        return CCD_ERR_ARG;
    const EncSlot& s = *e->slots[slot];
    if (grid < 0 || grid >= s.hdr.n_grids) return CCD_ERR_ARG;
    if (s.rate.status < 0) return s.rate.status;
    size_t off = s.delta_off;
    for (int g = 0; g < grid; ++g) off += 2 * static_cast<size_t>(s.hdr.grid_h[g]) * s.hdr.grid_w[g];
    *dev_ptr = e->delta_map.as<float>() + off;
    return s.hdr.grid_h[grid] * s.hdr.grid_w[grid];
}

int ccd_enc_slot_status(const ccd_enc* e, int slot, int32_t* out8) {
    if (!e || slot < 0 || slot >= static_cast<int>(e->slots.size()) || e->in_flight == kRun || !e->slots[slot]->ran) return CCD_ERR_ARG;
    if (out8) std::memcpy(out8, e->status.host.as<int32_t>() + static_cast<size_t>(slot) * kEncStatusWords, kEncStatusWords * sizeof(int32_t));
    return e->slots[slot]->status;
}

int64_t ccd_enc_slot_payload(const ccd_enc* e, int slot, const uint8_t** device_ptr) {
    if (!e || !device_ptr || slot < 0 || slot >= static_cast<int>(e->slots.size()) || e->in_flight == kRun || !e->slots[slot]->ran) return CCD_ERR_ARG;
    const EncSlot& s = *e->slots[slot];
    if (s.status < 0) return s.status;
    *device_ptr = s.out.as<uint8_t>();
    return static_cast<int64_t>(s.n_words) * 4;
}

int64_t ccd_enc_slot_bytes(ccd_enc* e, int slot, uint8_t** out) {
    if (!e || !out || slot < 0 || slot >= static_cast<int>(e->slots.size()) || e->in_flight == kRun || !e->slots[slot]->ran) return CCD_ERR_ARG;
    const EncSlot& s = *e->slots[slot];
    if (s.status < 0) return s.status;
    ccd_cc_header h = s.hdr;
    h.n_bytes_latent = static_cast<int32_t>(s.n_words * 4);
    uint8_t hb[256];
    const int n_hb = ccd_write_cc_header(&h, hb, sizeof(hb));
    if (n_hb < 0) return n_hb;
    const size_t n_lat = static_cast<size_t>(s.n_words) * 4, total = static_cast<size_t>(n_hb) + s.nn.size() + n_lat;
    uint8_t* p = static_cast<uint8_t*>(std::malloc(total + 4));
    if (!p) return CCD_ERR_NOMEM;
    std::memcpy(p, hb, static_cast<size_t>(n_hb));
    std::memcpy(p + n_hb, s.nn.data(), s.nn.size());
    // (the words are little-endian in memory, which is the byte order of the stream)
    if (hipSetDevice(e->device) != hipSuccess ||
        (n_lat && hipMemcpy(p + n_hb + s.nn.size(), s.out.p, n_lat, hipMemcpyDeviceToHost) != hipSuccess)) {
        std::free(p);
        return CCD_ERR_HIP;
    }
    *out = p;
    return static_cast<int64_t>(total);
}

}  // extern "C"
