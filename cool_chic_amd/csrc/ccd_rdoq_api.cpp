// ccd_rdoq_api.cpp - ccd_rdoq_* of include/ccd.h: the host side of one RDOQ step.  The geometry of the
// influence boxes is stated once, in influence_box() below: ccd_rdoq_influence_box answers from it and ccd_rdoq_add builds the
// device tables from it.
#include <cmath>
#include <cstring>
#include <new>

#include "ccd_host.hpp"
#include "ccd_kernels.hpp"

using namespace ccd;

namespace {
// What the boxes of a cool-chic follow from.
struct Geometry {
    ccd_cc_header h;
    int level[CCD_MAX_GRIDS];          // size changes between grid 0 and grid g
    int dy[kMaxCtx], dx[kMaxCtx];      // context k of (y, x) is the latent (y - dy[k], x + dx[k])
    bool has_foot[CCD_MAX_GRIDS];
    Footprint fp[CCD_MAX_GRIDS];
    int chroma_shift;
    int cells_h, cells_w;
};

int make_geometry(const ccd_cc_header* arch, int frame_data_type, Geometry& G) {
    if (rederive_cc_header(*arch, static_cast<size_t>(std::max(arch->nn_n_bytes, 0)), &G.h) < 0) return CCD_ERR_VALUE;
    const ccd_cc_header& h = G.h;
    if (h.n_grids < 1 || h.grid_h[0] < 1 || h.grid_w[0] < 1 || h.img_size[0] < 1 || h.img_size[1] < 1) return CCD_ERR_VALUE;
    if (h.spatial_context_arm < 0 || h.spatial_context_arm > kMaxCtx) return CCD_ERR_VALUE;
    int level = 0;
    for (int g = 0; g < h.n_grids; ++g) {
        if (g > 0 && (h.grid_h[g] != h.grid_h[g - 1] || h.grid_w[g] != h.grid_w[g - 1])) ++level;
        if (level > 30) return CCD_ERR_UNSUPPORTED;
        G.level[g] = level;
        const int rc = footprint(h, g, G.fp[g]);
        if (rc < 0) return rc;
        G.has_foot[g] = rc == 0;
    }
    context_offsets(h.spatial_context_arm, G.dy, G.dx);
    G.chroma_shift = frame_data_type == 1 ? 1 : 0;
    G.cells_h = (h.img_size[0] + kRdoqCell - 1) / kRdoqCell;
    G.cells_w = (h.img_size[1] + kRdoqCell - 1) / kRdoqCell;
    if (G.cells_h > 0xffff || G.cells_w > 0xffff) return CCD_ERR_UNSUPPORTED;
    return CCD_OK;
}

// A rectangle of luma samples that grows: {top, left, bottom, right}, inclusive.
struct Rect {
    int64_t r[4] = {INT64_MAX, INT64_MAX, -1, -1};
    void add(int64_t top, int64_t left, int64_t bottom, int64_t right) {
        if (top > bottom || left > right) return;
        r[0] = std::min(r[0], top); r[1] = std::min(r[1], left);
        r[2] = std::max(r[2], bottom); r[3] = std::max(r[3], right);
    }
};

// area() of the pixels rows qy0 .. qy1, columns qx0 .. qx1 of grid g (the union of their areas is a rectangle: area is monotone
// in the pixel's index along each axis).
void add_area(const Geometry& G, int g, int64_t qy0, int64_t qy1, int64_t qx0, int64_t qx1, Rect& R) {
    const ccd_cc_header& h = G.h;
    int64_t lo[2], hi[2];
    for (int a = 0; a < 2; ++a) {
        const int64_t n0 = a ? h.grid_w[0] : h.grid_h[0], N = h.img_size[a];
        const int64_t q0 = a ? qx0 : qy0, q1 = a ? qx1 : qy1;
        lo[a] = ((q0 << G.level[g]) * N) / n0;
        const int64_t end = std::min((q1 + 1) << G.level[g], n0);
        hi[a] = (end * N + n0 - 1) / n0 - 1;
        lo[a] = std::min(lo[a], N - 1);
        hi[a] = std::max(lo[a], std::min(hi[a], N - 1));  // never empty, inside the picture
    }
    R.add(lo[0], lo[1], hi[0], hi[1]);
}

// The influence box of the latent (y, x) of grid m, in cells.
RdoqBox influence_box(const Geometry& G, int m, int y, int x) {
    const ccd_cc_header& h = G.h;
    Rect R;
    add_area(G, m, y, y, x, x, R);
    // dep(p), DESIGN.md 4.10 "Rate sensitivity": the spatial dependents ...
    for (int k = 0; k < h.spatial_context_arm; ++k) {
        const int qy = y + G.dy[k], qx = x - G.dx[k];
        if (qy >= 0 && qy < h.grid_h[m] && qx >= 0 && qx < h.grid_w[m]) add_area(G, m, qy, qy, qx, qx, R);
    }
    // ... and the IFCE blocks of the finer grids
    for (int g = 0; g < m; ++g) {
        if (!(h.input_features_ifce[g] > 0 && g != h.n_grids - 1 && m - g - 1 < h.input_features_ifce[g])) continue;
        const int64_t side = int64_t{2} << (G.level[m] - G.level[g + 1]);
        const int64_t r0 = y * side, r1 = std::min<int64_t>((y + 1) * side, h.grid_h[g]) - 1;
        const int64_t c0 = x * side, c1 = std::min<int64_t>((x + 1) * side, h.grid_w[g]) - 1;
        if (r0 <= r1 && c0 <= c1) add_area(G, g, r0, r1, c0, c1, R);
    }
    if (G.has_foot[m]) {  // the clipped footprint; with 4:2:0 the halved box too, in luma samples
        const Footprint& f = G.fp[m];
        int64_t lo[2], hi[2];
        for (int a = 0; a < 2; ++a) {
            const int64_t s = static_cast<int64_t>(a ? x : y) * f.num[a] / f.den[a], N = h.img_size[a];
            lo[a] = std::max<int64_t>(s + f.lo[a], 0);
            hi[a] = std::min<int64_t>(s + f.hi[a], N - 1);
            if (G.chroma_shift && lo[a] <= hi[a]) {
                lo[a] = (lo[a] >> 1) << 1;
                hi[a] = std::min<int64_t>(((hi[a] >> 1) << 1) + 1, N - 1);
            }
        }
        R.add(lo[0], lo[1], hi[0], hi[1]);
    }
    RdoqBox b;
    b.top = static_cast<uint16_t>(R.r[0] / kRdoqCell); b.left = static_cast<uint16_t>(R.r[1] / kRdoqCell);
    b.bottom = static_cast<uint16_t>(R.r[2] / kRdoqCell); b.right = static_cast<uint16_t>(R.r[3] / kRdoqCell);
    return b;
}

struct RSlot {
    Geometry geo;
    int n_grids = 0;
    int8_t* lat[CCD_MAX_GRIDS] = {};
    const int64_t* dd[CCD_MAX_GRIDS] = {};
    const float* db[CCD_MAX_GRIDS] = {};
    bool have_maps = false;
    Block mem;                               // boxes, big lists, move maps, pick bytes, claim raster, taken raster
    size_t box_off[CCD_MAX_GRIDS] = {}, big_off[CCD_MAX_GRIDS] = {}, moves_off[CCD_MAX_GRIDS] = {}, pick_off[CCD_MAX_GRIDS] = {};
    size_t raster_off = 0, taken_off = 0;
    uint32_t n[CCD_MAX_GRIDS] = {}, n_big[CCD_MAX_GRIDS] = {}, first[CCD_MAX_GRIDS] = {};
    uint32_t raster_units = 0, taken_units = 0;
    double kD = 0, kR = 0;
    ccd_rdoq_result result;
    int64_t n_open = 0;                      // candidates of the last round that lost a cell
    bool covered = false;                    // by a finished step
    int frame_data_type = 0;
    uint32_t total = 0;                      // latents of all grids
    int leader = -1, follower = -1;          // ccd_rdoq_link: the slot whose rasters this one claims in / the slot that claims in this one's
    // ccd_rdoq_follow, ccd_rdoq_set_dep_maps
    struct Follow {
        ccd_rdoq_follow_desc d;
        bool stepped = false;                // a finished or pending step built its tables
        size_t reach_off = 0;                // in ccd_rdoq::follow_mem, of the last step
        size_t fbox_off[CCD_MAX_GRIDS] = {};
    };
    std::vector<Follow> follows;
    const int64_t* dd_dep[CCD_MAX_GRIDS] = {};
    bool have_dep = false;
    int64_t dep_sse = 0;                     // the chosen entries of the dependent maps, last step
};
}  // namespace

struct ccd_rdoq {
    int device = 0;
    std::vector<std::unique_ptr<RSlot>> slots;
    Mirror tables, results;
    Block partial;
    int pending = 0;       // a step is in flight
    int n_stepped = 0;     // slots the step in flight covers
    bool following = false;  // ... and it ran the following variants: a dependent sum per slot came back
    bool partial_step = false;  // ... without its rounds (ccd_rdoq_debug_stages): no result was written
    hipStream_t step_stream = nullptr;  // ... and the stream it was enqueued on
    StreamSet streams;
    int debug_stages = 7;  // ccd_rdoq_debug_stages
    Block follow_mem;      // the reach tables (first, one memset) and the flow-box tables of the last step with follows
};

namespace {
// The component-wide first uid of every slot: slots connected by links or follows (slot <-> target) form a
// component; its groups come in ascending order of their leader's slot, the leader's latents first, then the follower's.  A slot
// in no follow relation gets what it always had.  CCD_ERR_VALUE: a component with 2^32 latents or more.
int component_uids(const ccd_rdoq& r, std::vector<uint32_t>& uid0, std::vector<int>& comp) {
    const int n = static_cast<int>(r.slots.size());
    comp.resize(n);
    uid0.assign(n, 0);
    for (int k = 0; k < n; ++k) comp[k] = k;
    auto find = [&](int k) { while (comp[k] != k) k = comp[k] = comp[comp[k]]; return k; };
    auto join = [&](int a, int b) { a = find(a); b = find(b); if (a != b) comp[std::max(a, b)] = std::min(a, b); };
    for (int k = 0; k < n; ++k) {
        if (r.slots[k]->leader >= 0) join(k, r.slots[k]->leader);
        for (const auto& f : r.slots[k]->follows) join(k, f.d.target);
    }
    std::vector<uint64_t> next(n, 0);  // per component root: the latents numbered so far
    for (int k = 0; k < n; ++k) comp[k] = find(k);
    for (int k = 0; k < n; ++k) {      // leaders in ascending order; a follower right behind its leader
        const RSlot& s = *r.slots[k];
        if (s.leader >= 0) continue;
        uint64_t& at = next[comp[k]];
        uid0[k] = static_cast<uint32_t>(at);
        at += s.total;
        if (s.follower >= 0) { uid0[s.follower] = static_cast<uint32_t>(at); at += r.slots[s.follower]->total; }
        if (at > 0xffffffffull) return CCD_ERR_VALUE;
    }
    return CCD_OK;
}

// The tables of one step: grids, slots and the four prefix tables, whose last entries are the launches' block counts.
struct StepTables {
    std::vector<RdoqGrid> grids;
    std::vector<RdoqSlot> slots;
    std::vector<uint32_t> lane_prefix, big_prefix, chunk_prefix, cell_prefix;
};
// Stores the step's kD / kR in the slots as it goes.  CCD_ERR_UNSUPPORTED: more blocks than a launch takes.
int build_step_tables(ccd_rdoq& r, const std::vector<uint32_t>& uid0, const double* kD, const double* kR, const double* min_gain,
                      const uint64_t* grid_mask, StepTables& B) {
    const int n_slots = static_cast<int>(r.slots.size());
    B.slots.resize(n_slots);
    B.lane_prefix.assign(1, 0); B.big_prefix.assign(1, 0); B.chunk_prefix.assign(1, 0); B.cell_prefix.assign(1, 0);
    uint64_t lanes = 0, bigs = 0, chunks = 0, cell_blocks = 0;
    for (int k = 0; k < n_slots; ++k) {
        RSlot& s = *r.slots[k];
        char* base = s.mem.as<char>();
        RdoqSlot& S = B.slots[k];
        std::memset(&S, 0, sizeof(S));
        // a follower claims in its leader's rasters, its uids after the leader's (both at most 2^31 - 1: 32 bits hold the pair);
        // in a component with follows the uids run on over its groups (component_uids)
        const RSlot& owner = s.leader >= 0 ? *r.slots[s.leader] : s;
        S.raster = reinterpret_cast<unsigned long long*>(owner.mem.as<char>() + owner.raster_off);
        S.taken = reinterpret_cast<uint8_t*>(owner.mem.as<char>() + owner.taken_off);
        S.partner = s.leader >= 0 ? s.leader : s.follower;
        S.owns_raster = s.leader < 0;
        S.cells_h = s.geo.cells_h; S.cells_w = s.geo.cells_w;
        S.kD = s.kD = kD[k]; S.kR = s.kR = kR[k]; S.min_gain = min_gain[k];
        S.grid_mask = grid_mask[k];
        S.first_grid = static_cast<int32_t>(B.grids.size()); S.n_grids = s.n_grids;
        S.raster_units = s.raster_units; S.taken_units = s.taken_units;
        if (S.owns_raster) cell_blocks += (static_cast<uint64_t>(s.geo.cells_h) * s.geo.cells_w + 63) / 64;  // settle: a lane per cell
        if (cell_blocks > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
        B.cell_prefix.push_back(static_cast<uint32_t>(cell_blocks));
        for (int g = 0; g < s.n_grids; ++g) {
            RdoqGrid G;
            std::memset(&G, 0, sizeof(G));
            G.lat = s.lat[g]; G.dd = s.dd[g]; G.db = s.db[g];
            G.moves = reinterpret_cast<int8_t*>(base + s.moves_off[g]);
            G.pick = reinterpret_cast<uint8_t*>(base + s.pick_off[g]);
            G.box = reinterpret_cast<const RdoqBox*>(base + s.box_off[g]);
            G.big = reinterpret_cast<const uint32_t*>(base + s.big_off[g]);
            G.n = s.n[g]; G.first = uid0[k] + s.first[g]; G.slot = k; G.grid = g;
            lanes += (G.n + 63) / 64; bigs += s.n_big[g]; chunks += (G.n + kRdoqChunk - 1) / kRdoqChunk;
            if (lanes + bigs > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
            B.lane_prefix.push_back(static_cast<uint32_t>(lanes)); B.big_prefix.push_back(static_cast<uint32_t>(bigs));
            B.chunk_prefix.push_back(static_cast<uint32_t>(chunks));
            B.grids.push_back(G);
        }
    }
    return CCD_OK;
}

// With follows or dependent maps: the tables beside grids and slots, the components, the reach jobs.
struct FollowTables {
    std::vector<RdoqGridX> gridsx;
    std::vector<RdoqSlotX> slotsx;
    std::vector<uint32_t> comp_uid, reach_prefix[2];
    std::vector<int32_t> comp_slot;
    std::vector<RdoqReachJob> reach_jobs[2];
    size_t reach_bytes = 0;  // the reach tables come first in follow_mem (one memset), the flow boxes behind them
};
// Lays out ccd_rdoq::follow_mem and ends what an earlier step built there, whatever it returns.  CCD_ERR_NOMEM, CCD_ERR_HIP;
// CCD_ERR_UNSUPPORTED: more reach blocks than a launch takes.
int build_follow_tables(ccd_rdoq& r, const std::vector<uint32_t>& uid0, const std::vector<int>& comp, const StepTables& B, FollowTables& F) {
    const int n_slots = static_cast<int>(r.slots.size());
    F.gridsx.resize(B.grids.size());
    F.slotsx.resize(n_slots);
    std::memset(F.gridsx.data(), 0, F.gridsx.size() * sizeof(RdoqGridX));
    std::memset(F.slotsx.data(), 0, F.slotsx.size() * sizeof(RdoqSlotX));
    size_t follow_bytes = 0;
    for (auto& s : r.slots)
        for (auto& f : s->follows) {
            f.reach_off = follow_bytes;
            follow_bytes += align256(static_cast<size_t>(s->geo.cells_h) * s->geo.cells_w * kRdoqReachWords * sizeof(uint32_t));
        }
    F.reach_bytes = follow_bytes;
    for (auto& s : r.slots)
        for (auto& f : s->follows)
            for (int g = 0; g < s->n_grids; ++g) {
                f.fbox_off[g] = follow_bytes;
                follow_bytes += align256(static_cast<size_t>(s->n[g]) * sizeof(RdoqBox));
            }
    // nothing of an earlier step is in flight: the block may be exchanged, and what ccd_rdoq_slot_reach handed out ends here
    for (auto& s : r.slots)
        for (auto& f : s->follows) f.stepped = false;
    HIP_TRY(hipSetDevice(r.device));
    if (!r.follow_mem.ensure(r.device, BlockPool::kDevice, std::max<size_t>(follow_bytes, 256))) return CCD_ERR_NOMEM;
    char* fm = r.follow_mem.as<char>();
    for (int root = 0; root < n_slots; ++root) {  // a component's slots in the order of their uids: leaders ascending, follower behind
        if (comp[root] != root) continue;
        const int32_t first = static_cast<int32_t>(F.comp_uid.size());
        for (int k = 0; k < n_slots; ++k) {
            if (comp[k] != root || r.slots[k]->leader >= 0) continue;
            F.comp_uid.push_back(uid0[k]); F.comp_slot.push_back(k);
            const int fo = r.slots[k]->follower;
            if (fo >= 0) { F.comp_uid.push_back(uid0[fo]); F.comp_slot.push_back(fo); }
        }
        for (int k = 0; k < n_slots; ++k)
            if (comp[k] == root) { F.slotsx[k].comp_first = first; F.slotsx[k].comp_n = static_cast<int32_t>(F.comp_uid.size()) - first; }
    }
    uint64_t blocks[2] = {0, 0};
    F.reach_prefix[0].push_back(0); F.reach_prefix[1].push_back(0);
    for (int k = 0; k < n_slots; ++k) {
        RSlot& s = *r.slots[k];
        RdoqSlotX& SX = F.slotsx[k];
        SX.n_follows = static_cast<int32_t>(s.follows.size());
        for (size_t q = 0; q < s.follows.size(); ++q) {
            RSlot::Follow& f = s.follows[q];
            const RdoqSlot& T = B.slots[f.d.target];  // (raster / taken: its group's)
            SX.follow[q].reach = reinterpret_cast<const uint32_t*>(fm + f.reach_off);
            SX.follow[q].raster = T.raster;
            SX.follow[q].taken = T.taken;
            RdoqReachJob J;
            J.motion = f.d.motion; J.reach = reinterpret_cast<uint32_t*>(fm + f.reach_off);
            J.which = f.d.which; J.H = s.geo.h.img_size[0]; J.W = s.geo.h.img_size[1]; J.n_taps = f.d.warp_filter_size;
            J.gx = f.d.global_flow[2 * f.d.which]; J.gy = f.d.global_flow[2 * f.d.which + 1];
            J.cells_h = s.geo.cells_h; J.cells_w = s.geo.cells_w;
            const int c = f.d.warp_filter_size == 8;
            blocks[c] += static_cast<uint64_t>(J.cells_h) * J.cells_w;
            if (blocks[c] > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
            F.reach_jobs[c].push_back(J);
            F.reach_prefix[c].push_back(static_cast<uint32_t>(blocks[c]));
        }
        for (int g = 0; g < s.n_grids; ++g) {
            RdoqGridX& X = F.gridsx[B.slots[k].first_grid + g];
            X.dd_dep = s.dd_dep[g];
            for (size_t q = 0; q < s.follows.size(); ++q) X.fbox[q] = reinterpret_cast<RdoqBox*>(fm + s.follows[q].fbox_off[g]);
        }
    }
    return CCD_OK;
}

// Congruent rasters: the same picture in the same cells, and boxes widened for the same planes.
bool congruent(const RSlot& a, const RSlot& b) {
    return a.frame_data_type == b.frame_data_type && a.geo.h.img_size[0] == b.geo.h.img_size[0] && a.geo.h.img_size[1] == b.geo.h.img_size[1];
}

// The slot a getter answers for: one that exists and that a finished step covers, with no step in flight; else nullptr.
const RSlot* covered_slot(const ccd_rdoq* r, int slot) {
    if (slot >= static_cast<int>(r->slots.size()) || r->pending || !r->slots[slot]->covered) return nullptr;
    return r->slots[slot].get();
}
}  // namespace

extern "C" {

int ccd_rdoq_cell(void) { return kRdoqCell; }

int ccd_rdoq_max_rounds(void) { return kRdoqMaxRounds; }

int ccd_rdoq_influence_box(const ccd_cc_header* arch, int frame_data_type, int grid, int y, int x, int32_t cells[4]) {
    if (!arch || !cells || frame_data_type < 0 || frame_data_type > 2) return CCD_ERR_ARG;
    std::unique_ptr<Geometry> G(new (std::nothrow) Geometry());
    if (!G) return CCD_ERR_NOMEM;
    const int rc = make_geometry(arch, frame_data_type, *G);
    if (rc < 0) return rc;
    if (grid < 0 || grid >= G->h.n_grids || y < 0 || y >= G->h.grid_h[grid] || x < 0 || x >= G->h.grid_w[grid]) return CCD_ERR_ARG;
    const RdoqBox b = influence_box(*G, grid, y, x);
    cells[0] = b.top; cells[1] = b.left; cells[2] = b.bottom; cells[3] = b.right;
    return CCD_OK;
}

int ccd_rdoq_create(int device, ccd_rdoq** out) {
    if (!out) return CCD_ERR_ARG;
    *out = nullptr;
    ccd_rdoq* r = new (std::nothrow) ccd_rdoq();
    if (!r) return CCD_ERR_NOMEM;
    r->device = device;
    *out = r;
    return CCD_OK;
}

void ccd_rdoq_destroy(ccd_rdoq* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)r->streams.drain();
    for (auto& s : r->slots) s->mem.drop();
    r->follow_mem.drop();
    r->tables.drop(); r->partial.drop(); r->results.drop();
    delete r;
}

int ccd_rdoq_add(ccd_rdoq* r, const ccd_cc_header* arch, int frame_data_type, int8_t* const* latents) {
    if (!r || !arch || !latents || frame_data_type < 0 || frame_data_type > 2) return CCD_ERR_ARG;
    if (r->pending) return CCD_ERR_ARG;
    std::unique_ptr<RSlot> sp(new (std::nothrow) RSlot());
    if (!sp) return CCD_ERR_NOMEM;
    RSlot& s = *sp;
    const int rc = make_geometry(arch, frame_data_type, s.geo);
    if (rc < 0) return rc;
    const ccd_cc_header& h = s.geo.h;
    s.n_grids = h.n_grids;
    s.frame_data_type = frame_data_type;
    uint64_t total = 0;
    for (int g = 0; g < h.n_grids; ++g) {
        if (!latents[g]) return CCD_ERR_ARG;
        s.lat[g] = latents[g];
        s.first[g] = static_cast<uint32_t>(total);
        total += static_cast<uint64_t>(h.grid_h[g]) * h.grid_w[g];
        if (total > 0x7fffffffu) return CCD_ERR_UNSUPPORTED;
        s.n[g] = static_cast<uint32_t>(h.grid_h[g]) * static_cast<uint32_t>(h.grid_w[g]);
    }
    s.total = static_cast<uint32_t>(total);
    // the boxes of every latent and the lists of those a wave walks, laid out as they go to the device
    std::vector<std::vector<RdoqBox>> boxes(h.n_grids);
    std::vector<std::vector<uint32_t>> big(h.n_grids);
    TableImage img;
    for (int g = 0; g < h.n_grids; ++g) {
        boxes[g].resize(s.n[g]);
        for (int y = 0; y < h.grid_h[g]; ++y)
            for (int x = 0; x < h.grid_w[g]; ++x) {
                const uint32_t i = static_cast<uint32_t>(y) * h.grid_w[g] + x;
                const RdoqBox b = boxes[g][i] = influence_box(s.geo, g, y, x);
                if (static_cast<uint32_t>(b.bottom - b.top + 1) * static_cast<uint32_t>(b.right - b.left + 1) > kRdoqLaneCells) big[g].push_back(i);
            }
        s.n_big[g] = static_cast<uint32_t>(big[g].size());
        s.box_off[g] = img.put(boxes[g]);
        s.big_off[g] = img.put(big[g]);
    }
    std::vector<char>& host = img.bytes;
    host.resize(align256(host.size()));
    const size_t upload = host.size();
    size_t bytes = upload;
    for (int g = 0; g < h.n_grids; ++g) {
        s.moves_off[g] = bytes; bytes += align256(s.n[g]);
        s.pick_off[g] = bytes; bytes += align256(s.n[g]);
    }
    s.raster_off = bytes;
    const size_t raster_bytes = align256(static_cast<size_t>(s.geo.cells_h) * s.geo.cells_w * sizeof(unsigned long long));
    s.raster_units = static_cast<uint32_t>(raster_bytes / 16);
    bytes += raster_bytes;
    s.taken_off = bytes;
    const size_t taken_bytes = align256(static_cast<size_t>(s.geo.cells_h) * s.geo.cells_w);
    s.taken_units = static_cast<uint32_t>(taken_bytes / 16);
    bytes += taken_bytes;
    // ---- the device from here on ----
    HIP_TRY(hipSetDevice(r->device));
    if (!s.mem.get(r->device, BlockPool::kDevice, bytes)) return CCD_ERR_NOMEM;
    if (hipMemcpy(s.mem.p, host.data(), upload, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(s.mem.as<char>() + s.raster_off, 0xff, raster_bytes) != hipSuccess ||  // what the first step's claim needs:
        hipMemset(s.mem.as<char>() + s.taken_off, 0, taken_bytes) != hipSuccess ||      // all ones, and no cell taken
        hipDeviceSynchronize() != hipSuccess) {
        s.mem.drop();
        return CCD_ERR_HIP;
    }
    r->slots.push_back(std::move(sp));
    return static_cast<int>(r->slots.size()) - 1;
}

int ccd_rdoq_set_maps(ccd_rdoq* r, int slot, const int64_t* const* dd, const float* const* dbits) {
    if (!r || !dd || !dbits || slot < 0) return CCD_ERR_ARG;
    if (slot >= static_cast<int>(r->slots.size()) || r->pending) return CCD_ERR_ARG;
    RSlot& s = *r->slots[slot];
    for (int g = 0; g < s.n_grids; ++g)
        if (!dbits[g]) return CCD_ERR_ARG;
    for (int g = 0; g < s.n_grids; ++g) { s.dd[g] = dd[g]; s.db[g] = dbits[g]; }
    s.have_maps = true;
    return CCD_OK;
}

int ccd_rdoq_link(ccd_rdoq* r, int slot, int leader) {
    if (!r || slot < 0 || leader < 0 || slot == leader) return CCD_ERR_ARG;
    const int n_slots = static_cast<int>(r->slots.size());
    if (slot >= n_slots || leader >= n_slots || r->pending) return CCD_ERR_ARG;
    RSlot& f = *r->slots[slot];
    RSlot& l = *r->slots[leader];
    if (f.leader >= 0 || f.follower >= 0 || l.leader >= 0 || l.follower >= 0) return CCD_ERR_ARG;  // pairs only
    if (!congruent(f, l)) return CCD_ERR_VALUE;
    f.leader = leader;
    l.follower = slot;
    std::vector<uint32_t> uid0;
    std::vector<int> comp;
    if (component_uids(*r, uid0, comp) < 0) {  // (only with follows: a pair alone holds 2^32 - 2 at most)
        f.leader = l.follower = -1;
        return CCD_ERR_VALUE;
    }
    return CCD_OK;
}

int ccd_rdoq_max_follows(void) { return kRdoqMaxFollows; }

int ccd_rdoq_lane_cells(void) { return static_cast<int>(kRdoqLaneCells); }

// Not part of include/ccd.h (tests/test_rdoq_follow.py): the pick bytes of the last finished step, device uint8 [h][w] - 0 no
// candidate, 1 / 2 a candidate for -1 / +1, with 4 once selected and 8 once blocked; neither: open after the last round.
int64_t ccd_rdoq_debug_picks(const ccd_rdoq* r, int slot, int grid, void** dev_ptr) {
    if (!r || !dev_ptr || slot < 0 || grid < 0) return CCD_ERR_ARG;
    const RSlot* s = covered_slot(r, slot);
    if (!s || grid >= s->n_grids) return CCD_ERR_ARG;
    *dev_ptr = s->mem.as<char>() + s->pick_off[grid];
    return static_cast<int64_t>(s->n[grid]);
}

// Not part of include/ccd.h (tools/rd_bench.py --follow, as ccd_dsens_debug_stages): which stages of a step with follows are
// enqueued - 1 the memset and the reach launch(es), 2 the flow boxes, 4 the rounds and the sums; 7 is a step.  Without bit 4 the
// tables of the last full step stay in use and no result is written: after such a step no slot is covered, so the result
// getters refuse until a full step has run.  For timing only.
int ccd_rdoq_debug_stages(ccd_rdoq* r, int mask) {
    if (!r || mask < 1 || mask > 7 || r->pending) return CCD_ERR_ARG;
    r->debug_stages = mask;
    return CCD_OK;
}

int ccd_rdoq_follow(ccd_rdoq* r, int slot, const ccd_rdoq_follow_desc* f) {
    if (!r || !f || slot < 0 || !f->motion || f->target < 0 || f->frozen < -1) return CCD_ERR_ARG;
    if (f->frame_type < 1 || f->frame_type > 2 || f->which < 0 || f->which >= f->frame_type) return CCD_ERR_ARG;
    const int n_slots = static_cast<int>(r->slots.size());
    if (slot >= n_slots || f->target >= n_slots || f->frozen >= n_slots || r->pending) return CCD_ERR_ARG;
    RSlot& s = *r->slots[slot];
    if (static_cast<int>(s.follows.size()) >= kRdoqMaxFollows) return CCD_ERR_ARG;
    if (f->target == slot || !warp_filter_ok(f->warp_filter_size)) return CCD_ERR_VALUE;
    if (!congruent(s, *r->slots[f->target])) return CCD_ERR_VALUE;  // as ccd_rdoq_link asks
    RSlot::Follow fo;
    fo.d = *f;
    s.follows.push_back(fo);
    std::vector<uint32_t> uid0;
    std::vector<int> comp;
    if (component_uids(*r, uid0, comp) < 0) {
        s.follows.pop_back();
        return CCD_ERR_VALUE;
    }
    return static_cast<int>(s.follows.size()) - 1;
}

int ccd_rdoq_set_dep_maps(ccd_rdoq* r, int slot, const int64_t* const* dd_dep) {
    if (!r || slot < 0) return CCD_ERR_ARG;
    if (slot >= static_cast<int>(r->slots.size()) || r->pending) return CCD_ERR_ARG;
    RSlot& s = *r->slots[slot];
    s.have_dep = false;
    for (int g = 0; g < s.n_grids; ++g) {
        s.dd_dep[g] = dd_dep ? dd_dep[g] : nullptr;
        s.have_dep = s.have_dep || s.dd_dep[g];
    }
    return CCD_OK;
}

int ccd_rdoq_step(ccd_rdoq* r, const double* kD, const double* kR, const double* min_gain, const uint64_t* grid_mask, void* stream) {
    return ccd_rdoq_step_rounds(r, kD, kR, min_gain, grid_mask, 1, stream);
}

int ccd_rdoq_step_rounds(ccd_rdoq* r, const double* kD, const double* kR, const double* min_gain, const uint64_t* grid_mask, int max_rounds,
                         void* stream) {
    if (!r || !kD || !kR || !min_gain || !grid_mask || max_rounds < 1 || max_rounds > kRdoqMaxRounds) return CCD_ERR_ARG;
    if (r->pending) return CCD_ERR_ARG;
    const int n_slots = static_cast<int>(r->slots.size());
    for (int k = 0; k < n_slots; ++k) {
        if (!(std::isfinite(kD[k]) && kD[k] >= 0 && std::isfinite(kR[k]) && kR[k] >= 0 && std::isfinite(min_gain[k]) && min_gain[k] >= 0))
            return CCD_ERR_ARG;
        if (!r->slots[k]->have_maps) return CCD_ERR_ARG;
    }
    if (n_slots == 0) return CCD_OK;
    // the flows are followed as they are: no move of a followed frame's motion cool-chic in the same step
    bool following = false;
    for (int k = 0; k < n_slots; ++k) {
        const RSlot& s = *r->slots[k];
        following = following || s.have_dep || !s.follows.empty();
        for (const auto& f : s.follows)
            if (f.d.frozen >= 0 && grid_mask[f.d.frozen] != 0) return CCD_ERR_VALUE;
    }
    std::vector<uint32_t> uid0;
    std::vector<int> comp;
    StepTables B;
    FollowTables F;
    int rc = component_uids(*r, uid0, comp);
    if (rc == CCD_OK) rc = build_step_tables(*r, uid0, kD, kR, min_gain, grid_mask, B);
    if (rc == CCD_OK && following) rc = build_follow_tables(*r, uid0, comp, B, F);
    if (rc < 0) return rc;
    // one block, one copy
    TableImage img;
    const size_t o_grids = img.put(B.grids), o_slots = img.put(B.slots);
    const size_t o_lane = img.put(B.lane_prefix), o_big = img.put(B.big_prefix), o_chunk = img.put(B.chunk_prefix), o_cell = img.put(B.cell_prefix);
    const size_t o_gx = img.put(F.gridsx), o_sx = img.put(F.slotsx), o_cuid = img.put(F.comp_uid), o_cslot = img.put(F.comp_slot);
    const size_t o_rj[2] = {img.put(F.reach_jobs[0]), img.put(F.reach_jobs[1])}, o_rp[2] = {img.put(F.reach_prefix[0]), img.put(F.reach_prefix[1])};
    const std::vector<char>& buf = img.bytes;
    HIP_TRY(hipSetDevice(r->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    r->streams.note(st);
    // nothing of an earlier step is in flight (its wait synchronised), so the blocks may be exchanged for larger ones
    // the results, then one int64 per slot: its open candidates
    const size_t n_chunks = B.chunk_prefix.back();
    const size_t open_off = static_cast<size_t>(n_slots) * sizeof(ccd_rdoq_result);
    const size_t dep_off = open_off + static_cast<size_t>(n_slots) * sizeof(int64_t);  // (following) and one more: its dependent sum
    const size_t res_bytes = dep_off + (following ? static_cast<size_t>(n_slots) * sizeof(int64_t) : 0);
    const size_t partial_dep_off = align256(n_chunks * sizeof(RdoqPartial));
    if (!r->tables.ensure(r->device, buf.size()) ||
        !r->partial.ensure(r->device, BlockPool::kDevice, partial_dep_off + (following ? n_chunks * sizeof(int64_t) : 0)) ||
        !r->results.ensure(r->device, res_bytes))
        return CCD_ERR_NOMEM;
    std::memcpy(r->tables.host.p, buf.data(), buf.size());
    const Mirror& T = r->tables;
    RdoqStepLaunch L = {};
    L.t.grids = T.dev_at<RdoqGrid>(o_grids); L.t.slots = T.dev_at<RdoqSlot>(o_slots);
    L.t.lane_prefix = T.dev_at<uint32_t>(o_lane); L.t.big_prefix = T.dev_at<uint32_t>(o_big);
    L.t.chunk_prefix = T.dev_at<uint32_t>(o_chunk); L.t.cell_prefix = T.dev_at<uint32_t>(o_cell);
    L.t.n_grids = static_cast<int32_t>(B.grids.size()); L.t.n_slots = n_slots;
    L.t.n_lane_blocks = B.lane_prefix.back();
    L.n_big = B.big_prefix.back(); L.n_chunks = B.chunk_prefix.back(); L.n_cell_blocks = B.cell_prefix.back();
    L.rounds = max_rounds;
    L.sums.partial = r->partial.as<RdoqPartial>();
    L.sums.results = r->results.dev.as<ccd_rdoq_result>();
    L.sums.open = reinterpret_cast<int64_t*>(r->results.dev.as<char>() + open_off);
    if (following) {
        L.t.gx = T.dev_at<RdoqGridX>(o_gx); L.t.sx = T.dev_at<RdoqSlotX>(o_sx);
        L.t.comp_uid = T.dev_at<uint32_t>(o_cuid); L.t.comp_slot = T.dev_at<int32_t>(o_cslot);
        for (int c = 0; c < 2; ++c) {
            L.reach_jobs[c] = T.dev_at<RdoqReachJob>(o_rj[c]);
            L.reach_prefix[c] = T.dev_at<uint32_t>(o_rp[c]);
            L.n_reach[c] = static_cast<int>(F.reach_jobs[c].size());
            L.reach_blocks[c] = F.reach_prefix[c].back();
        }
        L.reach_mem = r->follow_mem.p; L.reach_bytes = F.reach_bytes;
        L.sums.partial_dep = reinterpret_cast<int64_t*>(r->partial.as<char>() + partial_dep_off);
        L.sums.dep_out = reinterpret_cast<int64_t*>(r->results.dev.as<char>() + dep_off);
        L.stages = r->debug_stages;
    }
    const bool ok = r->tables.upload(buf.size(), st) == hipSuccess && launch_rdoq_step(L, st) == hipSuccess &&
                    r->results.download(res_bytes, st) == hipSuccess;
    if (!ok) {  // part of the step may have been enqueued: drain it; no slot has a result, no step is in flight
        (void)hipStreamSynchronize(st);
        for (auto& s : r->slots) {
            s->covered = false;
            for (auto& f : s->follows) f.stepped = false;
        }
        return CCD_ERR_HIP;
    }
    for (auto& s : r->slots)
        for (auto& f : s->follows) f.stepped = true;
    r->following = following;
    r->partial_step = following && !(r->debug_stages & 4);
    r->pending = 1;  // everything is enqueued
    r->n_stepped = n_slots;
    r->step_stream = st;
    return CCD_OK;
}

int ccd_rdoq_wait(ccd_rdoq* r, void* stream) {
    if (!r) return CCD_ERR_ARG;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (!r->pending) return CCD_OK;
    // the results are behind the step on the stream the step was given, whichever stream this call names
    if (r->step_stream != static_cast<hipStream_t>(stream)) HIP_TRY(hipStreamSynchronize(r->step_stream));
    r->pending = 0;
    if (r->partial_step) {  // a timing run of the tables alone: no slot has a result
        for (auto& s : r->slots) s->covered = false;
        return CCD_OK;
    }
    const ccd_rdoq_result* res = r->results.host.as<ccd_rdoq_result>();
    const int64_t* open = reinterpret_cast<const int64_t*>(res + r->n_stepped);
    for (int k = 0; k < r->n_stepped; ++k) {
        RSlot& s = *r->slots[k];
        s.result = res[k];
        s.n_open = open[k];
        s.dep_sse = r->following ? open[r->n_stepped + k] : 0;
        // (d_sse + dep_sse: 0 without dependent maps, and the sum is then d_sse to the bit)
        s.result.d_cost = s.kD * static_cast<double>(s.result.d_sse + s.dep_sse) + s.kR * s.result.d_bits;
        s.covered = true;
    }
    return CCD_OK;
}

int ccd_rdoq_slot_result(const ccd_rdoq* r, int slot, ccd_rdoq_result* out) {
    if (!r || !out || slot < 0) return CCD_ERR_ARG;
    const RSlot* s = covered_slot(r, slot);
    if (!s) return CCD_ERR_ARG;
    *out = s->result;
    return CCD_OK;
}

int64_t ccd_rdoq_slot_open(const ccd_rdoq* r, int slot) {
    if (!r || slot < 0) return CCD_ERR_ARG;
    const RSlot* s = covered_slot(r, slot);
    return s ? s->n_open : CCD_ERR_ARG;
}

int ccd_rdoq_slot_dep_sse(const ccd_rdoq* r, int slot, int64_t* out) {
    if (!r || !out || slot < 0) return CCD_ERR_ARG;
    const RSlot* s = covered_slot(r, slot);
    if (!s) return CCD_ERR_ARG;
    *out = s->dep_sse;
    return CCD_OK;
}

int64_t ccd_rdoq_slot_reach(const ccd_rdoq* r, int slot, int follow, void** dev_ptr) {
    if (!r || !dev_ptr || slot < 0 || follow < 0) return CCD_ERR_ARG;
    const RSlot* s = covered_slot(r, slot);
    if (!s || follow >= static_cast<int>(s->follows.size()) || !s->follows[follow].stepped) return CCD_ERR_ARG;
    *dev_ptr = r->follow_mem.as<char>() + s->follows[follow].reach_off;
    return static_cast<int64_t>(s->geo.cells_h) * s->geo.cells_w;
}

int64_t ccd_rdoq_slot_flow_boxes(const ccd_rdoq* r, int slot, int follow, int grid, void** dev_ptr) {
    if (!r || !dev_ptr || slot < 0 || follow < 0 || grid < 0) return CCD_ERR_ARG;
    const RSlot* s = covered_slot(r, slot);
    if (!s || follow >= static_cast<int>(s->follows.size()) || grid >= s->n_grids || !s->follows[follow].stepped) return CCD_ERR_ARG;
    *dev_ptr = r->follow_mem.as<char>() + s->follows[follow].fbox_off[grid];
    return static_cast<int64_t>(s->n[grid]);
}

int64_t ccd_rdoq_slot_moves(const ccd_rdoq* r, int slot, int grid, void** dev_ptr) {
    if (!r || !dev_ptr || slot < 0 || grid < 0) return CCD_ERR_ARG;
    const RSlot* s = covered_slot(r, slot);
    if (!s || grid >= s->n_grids) return CCD_ERR_ARG;
    *dev_ptr = s->mem.as<char>() + s->moves_off[grid];
    return static_cast<int64_t>(s->n[grid]);
}

}  // extern "C"
