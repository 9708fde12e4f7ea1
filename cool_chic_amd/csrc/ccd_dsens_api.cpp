// ccd_dsens_api.cpp - ccd_dsens_* and ccd_latent_footprint of include/ccd.h: the host side of the distortion deltas
// (DESIGN.md sections 4.13, 4.15 for the cool-chics of P / B frames, 4.16 for the frames that predict from a candidate's).  Built on the public ccd_batch_* calls: the float path is
// the decode batch's, untouched.
#include <array>
#include <cstring>
#include <new>

#include "ccd_host.hpp"
#include "ccd_inter_job.hpp"
#include "ccd_kernels.hpp"

using namespace ccd;

namespace {
int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && ((a < 0) != (b < 0))) ? 1 : 0); }  // b > 0
int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }
}  // namespace

namespace ccd {
// Where a move of one latent of `grid` can reach (supports only).  Per axis a (0 rows, 1 columns): the samples
// [s + lo[a], s + hi[a]] with s = floor(i * num[a] / den[a]) for the latent index i.  Returns 1 for a hyperlatent grid.
int footprint(const ccd_cc_header& h, int grid, Footprint& f) {
    if (grid < 0 || grid >= h.n_grids) return CCD_ERR_ARG;
    if (h.is_hyperlatent[grid]) return 1;
    int lat[CCD_MAX_GRIDS], n_lv = 0, lv = -1;
    for (int g = 0; g < h.n_grids; ++g)
        if (!h.is_hyperlatent[g]) { if (g == grid) lv = n_lv; lat[n_lv++] = g; }
    int64_t lo = 0, hi = 0;  // in samples of the grid's own level, around the latent
    if (lv != n_lv - 1) {    // the pre-concatenation filter: output y reads y + ky - k / 2, ky < k (the coarsest grid has none)
        const int k = h.ups_preconcat_k_size;
        lo -= (k - 1) - k / 2;  // so the source s reaches y = s + k / 2 - (k - 1) .. s + k / 2: (k - 1) / 2 on either side for odd k
        hi += k / 2;
    }
    for (int step = 0; step < lv; ++step) {  // x2 transposed convolution: input s reaches outputs 2s + 1 - k/2 .. 2s + k - k/2
        const int k = h.ups_k_size;
        lo = 2 * lo + 1 - k / 2;
        hi = 2 * hi + k - k / 2;
    }
    for (int l = 0; l < h.n_layer_synthesis; ++l) {  // replicate-padded k x k layers; the stabiliser and the output transform are 1 x 1
        const int pad = h.syn_layer[l].k_size / 2;
        lo -= pad;
        hi += pad;
    }
    const int g0 = lat[0];
    for (int a = 0; a < 2; ++a) {
        const int64_t in = a ? h.grid_w[g0] : h.grid_h[g0], out = h.img_size[a], pitch = int64_t{1} << lv;
        if (in == out) {  // every final resize is the identity at equal sizes
            f.lo[a] = static_cast<int32_t>(lo); f.hi[a] = static_cast<int32_t>(hi);
            f.num[a] = static_cast<uint32_t>(pitch); f.den[a] = 1;
            continue;
        }
        // output Y reads sources around Y' = (Y + c/2) in / out - c/2 (c = 1: bilinear, bicubic; c = 0: nearest): floor(Y') for
        // nearest, floor(Y') and the next for bilinear, floor(Y') - 1 .. floor(Y') + 2 for bicubic (index clamps only move reads
        // towards the picture).  So a source interval [a, b] is read where a - m_lo <= Y' < b + m_hi with (m_lo, m_hi) = (0, 1),
        // (1, 1), (2, 2), that is (2a - 2 m_lo + c) out - c in <= 2 in Y < (2b + 2 m_hi + c) out - c in.  One more half source sample
        // on each side pays for the float32 evaluation of Y' (an error far below 1/2 at sides up to 16383).
        const int c = h.final_upsampling_type == 0 ? 0 : 1;
        const int64_t m_lo = h.final_upsampling_type, m_hi = h.final_upsampling_type == 2 ? 2 : 1;
        const int64_t mlo = 2 * m_lo - c + 1, mhi = 2 * m_hi + c + 1;
        // Y >= ((2 lo - mlo) out - c in) / (2 in) relative to i pitch out / in, whose floor is s: floor(a + b) >= floor(a) + floor(b)
        f.lo[a] = static_cast<int32_t>(floor_div((2 * lo - mlo) * out - c * in, 2 * in));
        // ... and ceil(a + b) <= floor(a) + 1 + ceil(b)
        f.hi[a] = static_cast<int32_t>(ceil_div((2 * hi + mhi) * out - c * in, 2 * in) + 1);
        f.num[a] = static_cast<uint32_t>(pitch * out); f.den[a] = static_cast<uint32_t>(in);
    }
    return CCD_OK;
}
}  // namespace ccd

namespace {
// Axis a (0 rows, 1 columns) of `grid` as ccd_lattice.hpp describes it.  4:2:0: the chroma planes take the footprint halved,
// rounded outwards - as samples of the full picture that is the interval widened to even alignment.
LatticeAxis lattice_axis(const ccd_cc_header& h, const Footprint& f, int grid, int a, int frame_data_type) {
    LatticeAxis A;
    A.n = a ? h.grid_w[grid] : h.grid_h[grid]; A.N = h.img_size[a];
    A.lo = f.lo[a]; A.hi = f.hi[a]; A.num = f.num[a]; A.den = f.den[a];
    A.even = frame_data_type == 1 ? 1 : 0;
    return A;
}

// The stride of the grid's lattices: the regions of two latents S apart in either direction keep `margin` samples between them
// (0: they are disjoint, all the own maps need; DESIGN.md 4.16 for a candidate with dependents).
int probe_stride(const ccd_cc_header& h, const Footprint& f, int grid, int frame_data_type, int margin) {
    return std::max(lattice_stride(lattice_axis(h, f, grid, 0, frame_data_type), margin),
                    lattice_stride(lattice_axis(h, f, grid, 1, frame_data_type), margin));
}

struct PassPlan { int grid, py, px, move; };

struct Candidate {
    ccd_cc_header hdr;
    int bitdepth = 0, frame_data_type = 0;
    const int8_t* lat[CCD_MAX_GRIDS] = {};
    const void* src[3] = {};
    int base_slot = -1, first_probe = -1;
    Block priv, maps;                        // K private copies of every grid; the int64 maps
    size_t grid_off[CCD_MAX_GRIDS] = {};     // of grid g inside one private copy
    size_t copy_bytes = 0;                   // of one private copy
    size_t map_off[CCD_MAX_GRIDS] = {};
    Footprint fp[CCD_MAX_GRIDS];
    int stride[CCD_MAX_GRIDS] = {};          // 0: hyperlatent
    std::vector<PassPlan> passes;            // the float passes, grid by grid
    int status = CCD_OK;
    bool covered = false;                    // by a finished run
    // one cool-chic of a P / B frame: its slots have no integer planes of their own, dsens_inter_kernel writes
    // those of the FRAME into `inter_buf`, which also holds the references as f32 and, for a residue candidate, the warped ones
    bool is_inter = false;
    ccd_dsens_inter inter = {};
    Block inter_buf;
    float* ref_f32[2] = {};
    float* warped[2] = {};
    std::vector<std::array<void*, 3>> inter_planes;  // [0] base, [1 + k] probe slot k
    // the frames that predict from this one: the passes keep `margin` samples between two regions, dsens_dep_kernel
    // sums what every probe does to the dependents into `dep_maps`
    struct Dependent {
        ccd_dsens_dependent in;
        Block buf;                 // [the other reference as f32, B frames][base planes]
        float* other_f32 = nullptr;
        void* base[3] = {};
    };
    std::vector<Dependent> deps;
    int margin = 0;
    Block dep_maps, dep_f32;                 // [maps][flags][conflict counters]; the frame's base and K probe planes as f32 4:4:4
    size_t dep_zero_bytes = 0, flag_off[CCD_MAX_GRIDS] = {}, count_off = 0;
    int64_t conflicts[CCD_MAX_GRIDS] = {};   // of the last finished run
    bool dep_covered = false;
    int64_t* dep_map(int g) const { return reinterpret_cast<int64_t*>(dep_maps.as<char>() + map_off[g]); }
    uint8_t* dep_flag(int g) const { return dep_maps.as<uint8_t>() + flag_off[g]; }
    unsigned long long* dep_count(int g) const { return reinterpret_cast<unsigned long long*>(dep_maps.as<char>() + count_off) + g; }
    float* frame_f32(int k) const {  // k = -1: the base planes, else probe slot k
        return dep_f32.as<float>() + static_cast<size_t>(k + 1) * 3 * hdr.img_size[0] * hdr.img_size[1];
    }
    const void* frame_plane(const ccd_dsens* d, int k, int p) const;
    // the candidate's frame with the frame header of a P / B frame of its size: its own, or a dependent's
    InterFrameDesc frame_desc(int frame_type, int warp_filter_size, const int32_t* global_flow) const {
        return InterFrameDesc{hdr.img_size[0], hdr.img_size[1], bitdepth, frame_data_type, frame_type, warp_filter_size, global_flow};
    }
    void drop() { priv.drop(); maps.drop(); inter_buf.drop(); dep_maps.drop(); dep_f32.drop(); for (auto& q : deps) q.buf.drop(); }
    int8_t* copy(int k, int g) const { return priv.as<int8_t>() + static_cast<size_t>(k) * copy_bytes + grid_off[g]; }
    int64_t* map(int g) const { return reinterpret_cast<int64_t*>(maps.as<char>() + map_off[g]); }
};

struct Round {  // offsets into the tables block
    size_t segs = 0, seg_prefix = 0, passes = 0, unit_prefix = 0, probe_prefix = 0;
    int n_segs = 0, n_passes = 0;
    uint32_t n_blocks = 0, n_units = 0, n_probes = 0;
    JobLaunch probes[2];  // dsens_inter_kernel, by kernel instantiation: [0] run-time taps, [1] sinc-8
    JobLaunch deps[2];    // dsens_dep_kernel, by the DEPENDENT's filter
};
}  // namespace

struct ccd_dsens {
    int device = 0, K = 0;
    ccd_batch* batch = nullptr;
    std::vector<std::unique_ptr<Candidate>> cands;
    std::vector<Round> rounds;
    Mirror tables;
    Block slab;
    JobLaunch inter_base[2];  // the base slots of the inter candidates, behind the first round's float path
    JobLaunch dep_base[2];    // the base planes of the dependents, behind those
    JobLaunch dep_final;      // dsens_dep_final_kernel over the grids of the candidates with dependents
    bool planned = false;   // the tables describe every candidate
    int pending = 0;        // a run is in flight
    hipStream_t run_stream = nullptr;  // ... on this stream
    int dead = CCD_OK;      // an add failed half way: the batch holds slots no candidate owns
    int stages = 31;        // ccd_dsens_debug_stages
    StreamSet streams;
};

// plane p of the candidate's frame as slot k decodes it (-1: the base slot)
const void* Candidate::frame_plane(const ccd_dsens* d, int k, int p) const {
    int ph = 0, pw = 0;
    if (is_inter) return inter_planes[k + 1][p];
    return ccd_batch_plane(d->batch, k < 0 ? base_slot : first_probe + k, p, &ph, &pw);
}

namespace {
DsensPass make_pass(const ccd_dsens* d, const Candidate& c, int k, const PassPlan& pp, bool empty) {
    const ccd_cc_header& h = c.hdr;
    DsensPass P;
    std::memset(&P, 0, sizeof(P));
    const int g = pp.grid;
    P.lat = c.lat[g];
    P.map = c.map(g);
    P.h = h.grid_h[g]; P.w = h.grid_w[g];
    P.move = pp.move;
    P.H = h.img_size[0]; P.W = h.img_size[1];
    P.chroma_shift = c.frame_data_type == 1 ? 1 : 0;
    P.wide = c.bitdepth > 8;
    P.num_y = P.den_y = P.num_x = P.den_x = 1;
    if (empty) {
        P.empty = 1; P.stride = 1; P.ny = P.h; P.nx = P.w; P.upp = 1; P.rows = 1;
        return P;
    }
    const Footprint& f = c.fp[g];
    for (int p = 0; p < 3; ++p) {
        P.base[p] = c.frame_plane(d, -1, p);
        P.probe[p] = c.frame_plane(d, k, p);
        P.src[p] = c.src[p];
    }
    P.stride = c.stride[g]; P.py = pp.py; P.px = pp.px;
    P.ny = (P.h - 1 - pp.py) / P.stride + 1;
    P.nx = (P.w - 1 - pp.px) / P.stride + 1;
    P.box[0] = f.lo[0]; P.box[1] = f.lo[1]; P.box[2] = f.hi[0]; P.box[3] = f.hi[1];
    P.num_y = f.num[0]; P.den_y = f.den[0]; P.num_x = f.num[1]; P.den_x = f.den[1];
    const int box_w = std::min<int64_t>(P.W, static_cast<int64_t>(f.hi[1]) - f.lo[1] + 1);
    const int box_h = std::min<int64_t>(P.H, static_cast<int64_t>(f.hi[0]) - f.lo[0] + 1);
    P.rows = std::max(1, kDsensBandSamples / std::max(1, box_w));
    P.upp = (box_h + P.rows - 1) / P.rows;
    return P;
}

// slot `which` (-1: the base slot, else probe slot k) of an inter candidate as dsens_inter_kernel reconstructs it
InterUnitJob make_inter_job(const ccd_dsens* d, const Candidate& c, int which) {
    InterUnitJob J;
    std::memset(&J, 0, sizeof(J));
    fill_inter_geometry(J, c.frame_desc(c.inter.frame_type, c.inter.warp_filter_size, c.inter.global_flow));
    const float* own = ccd_batch_output(d->batch, which < 0 ? c.base_slot : c.first_probe + which);
    J.residue = c.inter.role == 0 ? own : c.inter.partner;
    J.motion = c.inter.role == 0 ? c.inter.partner : own;
    const bool two = c.inter.frame_type == 2;
    J.ref0 = c.ref_f32[0]; J.ref1 = two ? c.ref_f32[1] : c.ref_f32[0];
    J.w0 = c.warped[0]; J.w1 = c.warped[1];
    for (int p = 0; p < 3; ++p) J.plane[p] = c.inter_planes[which + 1][p];
    J.mode = which < 0 ? 0 : (c.inter.role == 0 ? 1 : 2);
    return J;
}

// dependent q of the candidate reconstructed with `ref` (the candidate's frame as f32 4:4:4) as its reference `which`: into its
// base planes (base = true: a job of dsens_inter_kernel), or as dsens_dep_kernel reconstructs a unit
InterUnitJob make_dep_recon(const Candidate& c, const Candidate::Dependent& q, const float* ref, bool base) {
    InterUnitJob J;
    std::memset(&J, 0, sizeof(J));
    fill_inter_geometry(J, c.frame_desc(q.in.frame_type, q.in.warp_filter_size, q.in.global_flow));
    const bool two = q.in.frame_type == 2;
    J.residue = q.in.residue; J.motion = q.in.motion;
    J.ref0 = (two && q.in.which == 1) ? q.other_f32 : ref;
    J.ref1 = (two && q.in.which == 0) ? q.other_f32 : ref;
    for (int p = 0; p < 3; ++p) J.plane[p] = q.base[p];
    J.mode = base ? 0 : 2;
    return J;
}

DsensDepJob make_dep_job(const Candidate& c, const Candidate::Dependent& q, int k, const PassPlan& pp) {
    DsensDepJob D;
    std::memset(&D, 0, sizeof(D));
    D.recon = make_dep_recon(c, q, c.frame_f32(k), false);
    for (int p = 0; p < 3; ++p) D.src[p] = q.in.src[p];
    const int g = pp.grid;
    D.acc = reinterpret_cast<unsigned long long*>(c.dep_map(g));
    D.flag = c.dep_flag(g);
    D.which = q.in.which;
    D.h = c.hdr.grid_h[g]; D.w = c.hdr.grid_w[g];
    D.move = pp.move; D.stride = c.stride[g]; D.py = pp.py; D.px = pp.px;
    D.ay = lattice_axis(c.hdr, c.fp[g], g, 0, c.frame_data_type);
    D.ax = lattice_axis(c.hdr, c.fp[g], g, 1, c.frame_data_type);
    return D;
}

// Every round's segments, passes and reconstruction jobs, one block, one copy.
int build_tables(ccd_dsens* d, hipStream_t st) {
    const int K = d->K;
    size_t n_rounds = 1;
    for (const auto& c : d->cands) n_rounds = std::max(n_rounds, (c->passes.size() + K - 1) / K);
    TableImage img;
    d->rounds.assign(n_rounds, Round{});
    uint32_t max_units = 1;
    {
        std::vector<InterUnitJob> base[2];
        for (const auto& cp : d->cands)
            if (cp->is_inter) base[cp->inter.warp_filter_size == 8].push_back(make_inter_job(d, *cp, -1));
        for (int i = 0; i < 2; ++i) {
            const int rc = put_job_launch(img, base[i], d->inter_base[i]);
            if (rc < 0) return rc;
        }
        std::vector<InterUnitJob> dep_base[2];
        std::vector<DsensDepGrid> grids;
        std::vector<uint32_t> grid_prefix(1, 0);
        for (const auto& cp : d->cands) {
            for (const auto& q : cp->deps) dep_base[q.in.warp_filter_size == 8].push_back(make_dep_recon(*cp, q, cp->frame_f32(-1), true));
            for (int g = 0; !cp->deps.empty() && g < cp->hdr.n_grids; ++g) {
                DsensDepGrid G;
                std::memset(&G, 0, sizeof(G));
                G.lat = cp->lat[g]; G.map = cp->dep_map(g); G.flag = cp->dep_flag(g); G.conflicts = cp->dep_count(g);
                G.n = static_cast<uint32_t>(cp->hdr.grid_h[g]) * static_cast<uint32_t>(cp->hdr.grid_w[g]);
                grids.push_back(G);
                grid_prefix.push_back(grid_prefix.back() + (2 * G.n + 255) / 256);
            }
        }
        for (int i = 0; i < 2; ++i) {
            const int rc = put_job_launch(img, dep_base[i], d->dep_base[i]);
            if (rc < 0) return rc;
        }
        d->dep_final.n_jobs = static_cast<int>(grids.size()); d->dep_final.n_blocks = grid_prefix.back();
        d->dep_final.jobs = img.put(grids); d->dep_final.prefix = img.put(grid_prefix);
    }
    for (size_t r = 0; r < n_rounds; ++r) {
        std::vector<DsensSeg> segs;
        std::vector<DsensPass> passes;
        std::vector<InterUnitJob> jobs[2];
        std::vector<DsensDepJob> dep_jobs[2];
        for (const auto& cp : d->cands) {
            const Candidate& c = *cp;
            const ccd_cc_header& h = c.hdr;
            auto seg = [&](int k, int g, const PassPlan* pp) {
                DsensSeg S;
                std::memset(&S, 0, sizeof(S));
                S.src = c.lat[g];
                S.dst = c.copy(k, g);
                S.n = static_cast<uint32_t>(h.grid_h[g]) * static_cast<uint32_t>(h.grid_w[g]);
                S.w = h.grid_w[g];
                S.stride = 1;
                if (pp) { S.stride = c.stride[g]; S.py = pp->py; S.px = pp->px; S.move = pp->move; }
                segs.push_back(S);
            };
            for (int k = 0; k < K; ++k) {
                const size_t i = r * K + k;
                const PassPlan* cur = i < c.passes.size() ? &c.passes[i] : nullptr;
                const PassPlan* prev = (r > 0 && i - K < c.passes.size()) ? &c.passes[i - K] : nullptr;
                if (r == 0) {
                    for (int g = 0; g < h.n_grids; ++g) seg(k, g, (cur && cur->grid == g) ? cur : nullptr);
                } else {
                    if (cur) seg(k, cur->grid, cur);
                    if (prev && (!cur || cur->grid != prev->grid)) seg(k, prev->grid, nullptr);  // the grid moves on: restore
                }
                if (cur) passes.push_back(make_pass(d, c, k, *cur, false));
                if (cur && c.is_inter) jobs[c.inter.warp_filter_size == 8].push_back(make_inter_job(d, c, k));
                for (size_t q = 0; cur && q < c.deps.size(); ++q)
                    dep_jobs[c.deps[q].in.warp_filter_size == 8].push_back(make_dep_job(c, c.deps[q], k, *cur));
            }
            if (r == 0)
                for (int g = 0; g < h.n_grids; ++g)
                    if (h.is_hyperlatent[g])
                        for (int move = -1; move <= 1; move += 2) passes.push_back(make_pass(d, c, 0, PassPlan{g, 0, 0, move}, true));
        }
        Round& R = d->rounds[r];
        for (int i = 0; i < 2; ++i) {
            int rc = put_job_launch(img, jobs[i], R.probes[i]);
            if (rc >= 0) rc = put_job_launch(img, dep_jobs[i], R.deps[i]);
            if (rc < 0) return rc;
        }
        std::vector<uint32_t> seg_prefix(segs.size() + 1, 0), unit_prefix(passes.size() + 1, 0), probe_prefix(passes.size() + 1, 0);
        uint64_t blocks = 0, units = 0, probes = 0;
        for (size_t i = 0; i < segs.size(); ++i) { blocks += (segs[i].n + kDsensChunk - 1) / kDsensChunk; seg_prefix[i + 1] = static_cast<uint32_t>(blocks); }
        for (size_t i = 0; i < passes.size(); ++i) {
            const uint64_t n = static_cast<uint64_t>(passes[i].ny) * passes[i].nx;
            probes += n;
            units += n * passes[i].upp;
            if (units > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
            unit_prefix[i + 1] = static_cast<uint32_t>(units);
            probe_prefix[i + 1] = static_cast<uint32_t>(probes);
        }
        if (blocks > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
        R.n_segs = static_cast<int>(segs.size()); R.n_passes = static_cast<int>(passes.size());
        R.n_blocks = static_cast<uint32_t>(blocks); R.n_units = static_cast<uint32_t>(units); R.n_probes = static_cast<uint32_t>(probes);
        R.segs = img.put(segs); R.seg_prefix = img.put(seg_prefix);
        R.passes = img.put(passes); R.unit_prefix = img.put(unit_prefix); R.probe_prefix = img.put(probe_prefix);
        max_units = std::max(max_units, R.n_units);
    }
    // nothing of an earlier run is in flight (its wait synchronised), so the blocks may be exchanged for larger ones
    const std::vector<char>& buf = img.bytes;
    if (!d->tables.ensure(d->device, buf.size()) || !d->slab.ensure(d->device, BlockPool::kDevice, max_units * sizeof(int64_t))) return CCD_ERR_NOMEM;
    std::memcpy(d->tables.host.p, buf.data(), buf.size());
    HIP_TRY(d->tables.upload(buf.size(), st));
    d->planned = true;
    return CCD_OK;
}
}  // namespace

extern "C" {

int ccd_latent_footprint(const ccd_cc_header* arch, int grid, int32_t box[4]) {
    if (!arch || !box) return CCD_ERR_ARG;
    ccd_cc_header h;
    if (rederive_cc_header(*arch, static_cast<size_t>(std::max(arch->nn_n_bytes, 0)), &h) < 0) return CCD_ERR_VALUE;
    Footprint f;
    const int rc = footprint(h, grid, f);
    if (rc < 0) return rc;
    if (rc == 1) { box[0] = box[1] = 0; box[2] = box[3] = -1; return 1; }
    box[0] = f.lo[0]; box[1] = f.lo[1]; box[2] = f.hi[0]; box[3] = f.hi[1];
    return CCD_OK;
}

int ccd_latent_probe_stride_margin(const ccd_cc_header* arch, int grid, int frame_data_type, int margin) {
    if (!arch || frame_data_type < 0 || frame_data_type > 2 || margin < 0) return CCD_ERR_ARG;
    ccd_cc_header h;
    if (rederive_cc_header(*arch, static_cast<size_t>(std::max(arch->nn_n_bytes, 0)), &h) < 0) return CCD_ERR_VALUE;
    Footprint f;
    const int rc = footprint(h, grid, f);
    if (rc < 0) return rc;
    return rc == 1 ? 0 : probe_stride(h, f, grid, frame_data_type, margin);
}

int ccd_latent_probe_stride(const ccd_cc_header* arch, int grid, int frame_data_type) {
    return ccd_latent_probe_stride_margin(arch, grid, frame_data_type, 0);
}

// Host only (tests): ccd_lattice.hpp on one axis given by its numbers - n latents over N samples, the footprint interval
// [lo, hi] around floor(i num / den), `even` the 4:2:0 widening.  Not a function of any handle.
int ccd_debug_lattice_stride(int n, int N, int lo, int hi, uint32_t num, uint32_t den, int even, int margin) {
    if (n < 1 || N < 1 || den == 0 || lo > 0 || hi < 0 || margin < 0) return CCD_ERR_ARG;
    return lattice_stride(LatticeAxis{n, N, lo, hi, num, den, even ? 1 : 0}, margin);
}

// ... -1: no member of the lattice (stride S, phase) has its region under [a, b]; its index: exactly one has; -2: more than one.
// *first, *count (may be NULL): the first member hit and how many.
int ccd_debug_lattice_hit(int n, int N, int lo, int hi, uint32_t num, uint32_t den, int even, int S, int phase, int a, int b, int32_t* first,
                          int32_t* count) {
    if (n < 1 || N < 1 || den == 0 || lo > 0 || hi < 0 || S < 1 || phase < 0) return CCD_ERR_ARG;
    int f = -1;
    const int c = lattice_hit(LatticeAxis{n, N, lo, hi, num, den, even ? 1 : 0}, S, phase, a, b, &f);
    if (first) *first = f;
    if (count) *count = c;
    return c == 0 ? -1 : (c == 1 ? f : -2);
}

int ccd_dsens_create(int device, int n_probe_slots, ccd_dsens** out) {
    if (!out) return CCD_ERR_ARG;
    *out = nullptr;
    if (n_probe_slots < 1 || n_probe_slots > 64) return CCD_ERR_ARG;
    ccd_dsens* d = new (std::nothrow) ccd_dsens();
    if (!d) return CCD_ERR_NOMEM;
    d->device = device;
    d->K = n_probe_slots;
    const int rc = ccd_batch_create(device, &d->batch);
    if (rc < 0) { delete d; return rc; }
    // the float output is not looked at: slots that can write integer planes alone do
    (void)ccd_batch_set_option(d->batch, CCD_OPT_KEEP_FLOAT, 0);
    *out = d;
    return CCD_OK;
}

void ccd_dsens_destroy(ccd_dsens* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)d->streams.drain();
    ccd_batch_destroy(d->batch);  // drains the streams it was run on
    for (auto& c : d->cands) c->drop();
    d->tables.drop(); d->slab.drop();
    delete d;
}

// The passes of a candidate, grid by grid: every lattice of the stride that keeps c.margin samples between two regions.
static void plan_passes(Candidate& c) {
    const ccd_cc_header& h = c.hdr;
    c.passes.clear();
    for (int g = 0; g < h.n_grids; ++g) {
        if (h.is_hyperlatent[g]) continue;
        const int S = c.stride[g] = probe_stride(h, c.fp[g], g, c.frame_data_type, c.margin);
        for (int move = -1; move <= 1; move += 2)
            for (int py = 0; py < std::min(S, h.grid_h[g]); ++py)
                for (int px = 0; px < std::min(S, h.grid_w[g]); ++px) c.passes.push_back(PassPlan{g, py, px, move});
    }
}

// ccd_dsens_add and ccd_dsens_add_inter behind their pointer checks (inter: null for an intra candidate)
static int add_candidate(ccd_dsens* d, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn, const int8_t* const* latents,
                         const void* const* src, int bitdepth, int frame_data_type, const ccd_dsens_inter* inter) {
    if (bitdepth < 8 || bitdepth > 16 || frame_data_type < 0 || frame_data_type > 2 || d->pending) return CCD_ERR_ARG;
    if (d->dead < 0) return d->dead;
    std::unique_ptr<Candidate> cp(new (std::nothrow) Candidate());
    if (!cp) return CCD_ERR_NOMEM;
    Candidate& c = *cp;
    if (rederive_cc_header(*arch, n_nn, &c.hdr) < 0) return CCD_ERR_VALUE;
    const ccd_cc_header& h = c.hdr;
    if (h.n_symbols < 0 || h.n_symbols > 0x7fffffff) return CCD_ERR_UNSUPPORTED;
    if (inter) {
        if (!warp_filter_ok(inter->warp_filter_size) || !yuv420_sides_ok(frame_data_type, h.img_size[0], h.img_size[1])) return CCD_ERR_VALUE;
        if (h.out_channels != inter_channels(inter->frame_type, inter->role)) return CCD_ERR_VALUE;
        c.is_inter = true;
        c.inter = *inter;
    }
    c.bitdepth = bitdepth;
    c.frame_data_type = frame_data_type;
    size_t map_bytes = 0;
    for (int g = 0; g < h.n_grids; ++g) {
        if (!latents[g]) return CCD_ERR_ARG;
        c.lat[g] = latents[g];
        const size_t n = static_cast<size_t>(h.grid_h[g]) * h.grid_w[g];
        c.grid_off[g] = c.copy_bytes;
        c.copy_bytes += align256(n);
        c.map_off[g] = map_bytes;
        map_bytes += align256(2 * n * sizeof(int64_t));
        const int rc = footprint(h, g, c.fp[g]);
        if (rc < 0) return rc;
        if (rc == 1) continue;
    }
    plan_passes(c);
    for (int p = 0; p < 3; ++p) c.src[p] = src[p];
    // ---- the device from here on ----
    HIP_TRY(hipSetDevice(d->device));
    auto drop = [&c] { c.drop(); };
    if (!c.priv.get(d->device, BlockPool::kDevice, std::max<size_t>(256, c.copy_bytes * d->K)) ||
        !c.maps.get(d->device, BlockPool::kDevice, std::max<size_t>(256, map_bytes))) {
        drop();
        return CCD_ERR_NOMEM;
    }
    if (inter) {  // [references as f32][warped references, residue candidates][planes of the base and the K probe slots]
        const PlaneLayout lay = plane_layout(h.img_size[0], h.img_size[1], bitdepth, frame_data_type);
        const int n_refs = inter->frame_type == 2 ? 2 : 1, n_warped = inter->role == 0 ? n_refs : 0;
        const size_t total = (n_refs + n_warped) * lay.f32_3 + static_cast<size_t>(d->K + 1) * lay.planes();
        if (!c.inter_buf.get(d->device, BlockPool::kDevice, total)) { drop(); return CCD_ERR_NOMEM; }
        BlockCursor cur(c.inter_buf);
        for (int r = 0; r < n_refs; ++r) c.ref_f32[r] = cur.f32(lay);
        for (int r = 0; r < n_warped; ++r) c.warped[r] = cur.f32(lay);
        c.inter_planes.resize(d->K + 1);
        for (auto& pl : c.inter_planes) cur.planes(lay, pl.data());
    }
    // the slots of an inter cool-chic produce its float output only (as the decoder adds them): the planes are the frame's
    const int slot_bitdepth = inter ? 0 : bitdepth;
    c.base_slot = ccd_batch_add_latents(d->batch, arch, bytes_nn, n_nn, latents, 1, slot_bitdepth, frame_data_type);
    if (c.base_slot < 0) { drop(); return c.base_slot; }  // (nothing was added to the batch)
    for (int k = 0; k < d->K; ++k) {
        const int8_t* ptrs[CCD_MAX_GRIDS];
        for (int g = 0; g < h.n_grids; ++g) ptrs[g] = c.copy(k, g);
        const int s = ccd_batch_add_latents(d->batch, arch, bytes_nn, n_nn, ptrs, 1, slot_bitdepth, frame_data_type);
        if (s < 0) { drop(); d->dead = s; return s; }
        if (k == 0) c.first_probe = s;
    }
    d->planned = false;
    d->cands.push_back(std::move(cp));
    return static_cast<int>(d->cands.size()) - 1;
}

int ccd_dsens_add(ccd_dsens* d, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn, const int8_t* const* latents,
                  const void* const* src, int bitdepth, int frame_data_type) {
    if (!d || !arch || !bytes_nn || !latents || !src || !src[0] || !src[1] || !src[2]) return CCD_ERR_ARG;
    return add_candidate(d, arch, bytes_nn, n_nn, latents, src, bitdepth, frame_data_type, nullptr);
}

int ccd_dsens_add_inter(ccd_dsens* d, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn, const int8_t* const* latents,
                        const void* const* src, int bitdepth, int frame_data_type, const ccd_dsens_inter* inter) {
    if (!d || !arch || !bytes_nn || !latents || !src || !src[0] || !src[1] || !src[2] || !inter) return CCD_ERR_ARG;
    if (inter->frame_type < 1 || inter->frame_type > 2 || inter->role < 0 || inter->role > 1 || !inter->partner) return CCD_ERR_ARG;
    for (int p = 0; p < 3; ++p)
        if (!inter->ref0[p] || (inter->frame_type == 2 && !inter->ref1[p])) return CCD_ERR_ARG;
    return add_candidate(d, arch, bytes_nn, n_nn, latents, src, bitdepth, frame_data_type, inter);
}

int ccd_dsens_add_dependent(ccd_dsens* d, int slot, const ccd_dsens_dependent* dep) {
    if (!d || !dep || !dep->residue || !dep->motion || !dep->src[0] || !dep->src[1] || !dep->src[2]) return CCD_ERR_ARG;
    if (dep->frame_type < 1 || dep->frame_type > 2 || dep->which < 0 || dep->which > 1 || (dep->frame_type == 1 && dep->which != 0)) return CCD_ERR_ARG;
    for (int p = 0; p < 3; ++p)
        if (dep->frame_type == 2 && !dep->other_ref[p]) return CCD_ERR_ARG;
    if (d->pending) return CCD_ERR_ARG;
    if (!warp_filter_ok(dep->warp_filter_size)) return CCD_ERR_VALUE;
    if (slot < 0 || slot >= static_cast<int>(d->cands.size())) return CCD_ERR_ARG;
    if (d->dead < 0) return d->dead;
    Candidate& c = *d->cands[slot];
    const ccd_cc_header& h = c.hdr;
    if (!yuv420_sides_ok(c.frame_data_type, h.img_size[0], h.img_size[1])) return CCD_ERR_VALUE;
    // ---- the device from here on ----
    HIP_TRY(hipSetDevice(d->device));
    const size_t hw = static_cast<size_t>(h.img_size[0]) * h.img_size[1];
    const PlaneLayout lay = plane_layout(h.img_size[0], h.img_size[1], c.bitdepth, c.frame_data_type);
    if (c.deps.empty()) {  // the first one: [maps as the own ones][flags][counters], and the frame as f32 for the base and K probe slots
        size_t at = align256(c.map_off[h.n_grids - 1] + 2 * sizeof(int64_t) * h.grid_h[h.n_grids - 1] * h.grid_w[h.n_grids - 1]);
        for (int g = 0; g < h.n_grids; ++g) { c.flag_off[g] = at; at += align256(2 * static_cast<size_t>(h.grid_h[g]) * h.grid_w[g]); }
        c.count_off = at;
        at += align256(CCD_MAX_GRIDS * sizeof(unsigned long long));
        if (!c.dep_maps.get(d->device, BlockPool::kDevice, at) ||
            !c.dep_f32.get(d->device, BlockPool::kDevice, static_cast<size_t>(d->K + 1) * 3 * hw * sizeof(float))) {
            c.dep_maps.drop(); c.dep_f32.drop();
            return CCD_ERR_NOMEM;
        }
        c.dep_zero_bytes = at;
    }
    Candidate::Dependent q;
    q.in = *dep;
    const bool two = dep->frame_type == 2;
    if (!q.buf.get(d->device, BlockPool::kDevice, (two ? lay.f32_3 : 0) + lay.planes())) {
        if (c.deps.empty()) { c.dep_maps.drop(); c.dep_f32.drop(); }
        return CCD_ERR_NOMEM;
    }
    BlockCursor cur(q.buf);
    if (two) q.other_f32 = cur.f32(lay);
    cur.planes(lay, q.base);
    c.deps.push_back(q);
    int W = 0;  // the widest window of the dependents' warps: 2 bilinear, 4 bicubic, the filter size for sinc
    for (const auto& e : c.deps) W = std::max(W, e.in.warp_filter_size);
    c.margin = c.frame_data_type == 1 ? W + 2 : W - 1;
    plan_passes(c);
    c.covered = c.dep_covered = false;
    d->planned = false;
    return CCD_OK;
}

int ccd_dsens_run(ccd_dsens* d, void* stream) {
    if (!d || d->pending) return CCD_ERR_ARG;
    if (d->dead < 0) return d->dead;
    if (d->cands.empty()) return CCD_OK;
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    d->streams.note(st);
    if (!d->planned) {
        const int rc = build_tables(d, st);
        if (rc < 0) return rc;
    }
    const Mirror& T = d->tables;
    d->pending = 1;
    d->run_stream = st;
    auto reconstruct = [&](const JobLaunch (&L)[2]) -> int {  // one launch per kernel instantiation in use
        for (int i = 0; i < 2; ++i)
            if (launch_dsens_inter(T.dev_at<InterUnitJob>(L[i].jobs), T.dev_at<uint32_t>(L[i].prefix), L[i].n_jobs, L[i].n_blocks, i, st) != hipSuccess)
                return CCD_ERR_HIP;
        return CCD_OK;
    };
    for (const auto& cp : d->cands) {  // the references of the inter candidates as the warp reads them
        const Candidate& c = *cp;
        for (int r = 0; c.is_inter && r < (c.inter.frame_type == 2 ? 2 : 1); ++r) {
            const void* const* pl = r ? c.inter.ref1 : c.inter.ref0;
            HIP_TRY(launch_planes_to_444(pl[0], pl[1], pl[2], c.ref_f32[r], c.hdr.img_size[0], c.hdr.img_size[1], c.bitdepth, c.frame_data_type, st));
        }
    }
    auto dep_launches = [&](const JobLaunch (&L)[2]) -> int {
        for (int i = 0; i < 2; ++i)
            if (launch_dsens_dep(T.dev_at<DsensDepJob>(L[i].jobs), T.dev_at<uint32_t>(L[i].prefix), L[i].n_jobs, L[i].n_blocks, i, st) != hipSuccess)
                return CCD_ERR_HIP;
        return CCD_OK;
    };
    // slot k (-1: the base slot) of a candidate with dependents as the dependents' warps read it
    auto to_f32 = [&](const Candidate& c, int k) {
        return launch_planes_to_444(c.frame_plane(d, k, 0), c.frame_plane(d, k, 1), c.frame_plane(d, k, 2), c.frame_f32(k), c.hdr.img_size[0],
                                    c.hdr.img_size[1], c.bitdepth, c.frame_data_type, st);
    };
    const bool dep_convert = (d->stages & 8) != 0, dep_sum = (d->stages & 16) != 0;
    for (const auto& cp : d->cands) {  // the sums and flags of the dependents start from zero; their other references as f32
        const Candidate& c = *cp;
        if (c.deps.empty()) continue;
        HIP_TRY(hipMemsetAsync(c.dep_maps.p, 0, c.dep_zero_bytes, st));
        for (const auto& q : c.deps)
            if (q.other_f32 && dep_convert)
                HIP_TRY(launch_planes_to_444(q.in.other_ref[0], q.in.other_ref[1], q.in.other_ref[2], q.other_f32, c.hdr.img_size[0], c.hdr.img_size[1],
                                             c.bitdepth, c.frame_data_type, st));
    }
    bool first = true;
    size_t round = 0;
    for (const Round& R : d->rounds) {
        int rc = CCD_OK;
        if (d->stages & 1) {
            HIP_TRY(launch_dsens_apply(T.dev_at<DsensSeg>(R.segs), T.dev_at<uint32_t>(R.seg_prefix), R.n_segs, R.n_blocks, st));
            if ((rc = ccd_batch_run(d->batch, stream)) < 0) return rc;
        }
        if (first && (d->stages & 2) && (rc = reconstruct(d->inter_base)) < 0) return rc;  // the base planes, and the warped references they leave
        if (first && dep_convert) {  // the dependents' base planes from the candidates' base planes
            for (const auto& cp : d->cands)
                if (!cp->deps.empty()) HIP_TRY(to_f32(*cp, -1));
            if ((rc = reconstruct(d->dep_base)) < 0) return rc;
        }
        first = false;
        if ((d->stages & 2) && (rc = reconstruct(R.probes)) < 0) return rc;
        if (dep_convert)
            for (const auto& cp : d->cands)
                for (int k = 0; !cp->deps.empty() && k < d->K && round * d->K + k < cp->passes.size(); ++k) HIP_TRY(to_f32(*cp, k));
        if (dep_sum && (rc = dep_launches(R.deps)) < 0) return rc;
        ++round;
        if (d->stages & 4) {
            HIP_TRY(launch_dsens_sse(T.dev_at<DsensPass>(R.passes), T.dev_at<uint32_t>(R.unit_prefix), T.dev_at<uint32_t>(R.probe_prefix), R.n_passes,
                                     R.n_units, R.n_probes, d->slab.as<int64_t>(), st));
        }
    }
    if (dep_sum)
        HIP_TRY(launch_dsens_dep_final(T.dev_at<DsensDepGrid>(d->dep_final.jobs), T.dev_at<uint32_t>(d->dep_final.prefix), d->dep_final.n_jobs,
                                       d->dep_final.n_blocks, st));
    return CCD_OK;
}

// Not part of include/ccd.h: the measurement hook of tools/rd_bench.py --inter, which looks the symbol up by name.  Which stages of
// every round the following runs enqueue - bit 0 the float path (apply + ccd_batch_run), bit 1 the reconstruction launches of inter
// candidates, bit 2 the squared-error split, bit 3 the conversions of candidates with dependents (their planes to f32, the
// dependents' base planes), bit 4 dsens_dep_kernel and its finalising pass; 31 by default.  A run with another mask covers no slot: ccd_dsens_slot_map refuses
// (CCD_ERR_ARG) until a full run has finished.
int ccd_dsens_debug_stages(ccd_dsens* d, int mask) {
    if (!d || d->pending || mask < 0 || mask > 31) return CCD_ERR_ARG;
    d->stages = mask;
    return CCD_OK;
}

int ccd_dsens_wait(ccd_dsens* d, void* stream) {
    if (!d) return CCD_ERR_ARG;
    if (d->cands.empty() || !d->planned) {
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        d->pending = 0;
        return CCD_OK;
    }
    // the maps are behind the run on the stream the run was given, whichever stream this call names
    if (d->pending && d->run_stream != static_cast<hipStream_t>(stream)) {
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipStreamSynchronize(d->run_stream));
    }
    const int rc = ccd_batch_wait(d->batch, stream);  // synchronises; the first error of the batch's slots
    const bool ran = d->pending != 0;
    d->pending = 0;
    if (rc < 0 && rc != CCD_ERR_VALUE) return rc;
    if (!ran) return CCD_OK;
    int first = CCD_OK;
    for (auto& cp : d->cands) {
        Candidate& c = *cp;
        c.status = ccd_batch_slot_status(d->batch, c.base_slot);
        for (int k = 0; c.status == CCD_OK && k < d->K; ++k) c.status = ccd_batch_slot_status(d->batch, c.first_probe + k);
        c.covered = (d->stages & 7) == 7;
        c.dep_covered = c.covered && !c.deps.empty() && (d->stages & 24) == 24;
        if (c.dep_covered && c.status == CCD_OK) {  // (the stream is idle: ccd_batch_wait synchronised)
            unsigned long long n[CCD_MAX_GRIDS];
            HIP_TRY(hipMemcpy(n, c.dep_count(0), sizeof(n), hipMemcpyDeviceToHost));
            for (int g = 0; g < CCD_MAX_GRIDS; ++g) c.conflicts[g] = static_cast<int64_t>(n[g]);
        }
        if (first == CCD_OK && c.status != CCD_OK) first = c.status;
    }
    return first;
}

int64_t ccd_dsens_slot_map(const ccd_dsens* d, int slot, int grid, void** dev_ptr) {
    if (!d || !dev_ptr || slot < 0 || slot >= static_cast<int>(d->cands.size())) return CCD_ERR_ARG;
    const Candidate& c = *d->cands[slot];
    if (grid < 0 || grid >= c.hdr.n_grids || !c.covered || d->pending) return CCD_ERR_ARG;
    if (c.status != CCD_OK) return c.status;
    *dev_ptr = c.map(grid);
    return static_cast<int64_t>(c.hdr.grid_h[grid]) * c.hdr.grid_w[grid];
}

int64_t ccd_dsens_slot_dep_map(const ccd_dsens* d, int slot, int grid, void** dev_ptr) {
    if (!d || !dev_ptr || slot < 0 || slot >= static_cast<int>(d->cands.size())) return CCD_ERR_ARG;
    const Candidate& c = *d->cands[slot];
    if (grid < 0 || grid >= c.hdr.n_grids || c.deps.empty() || !c.dep_covered || d->pending) return CCD_ERR_ARG;
    if (c.status != CCD_OK) return c.status;
    *dev_ptr = c.dep_map(grid);
    return static_cast<int64_t>(c.hdr.grid_h[grid]) * c.hdr.grid_w[grid];
}

int64_t ccd_dsens_slot_dep_conflicts(const ccd_dsens* d, int slot, int grid) {
    if (!d || slot < 0 || slot >= static_cast<int>(d->cands.size())) return CCD_ERR_ARG;
    const Candidate& c = *d->cands[slot];
    if (grid < 0 || grid >= c.hdr.n_grids || c.deps.empty() || !c.dep_covered || d->pending) return CCD_ERR_ARG;
    if (c.status != CCD_OK) return c.status;
    return c.conflicts[grid];
}

int ccd_dsens_passes(const ccd_dsens* d, int slot) {
    if (!d || slot < 0 || slot >= static_cast<int>(d->cands.size())) return CCD_ERR_ARG;
    return static_cast<int>(d->cands[slot]->passes.size());
}

}  // extern "C"
