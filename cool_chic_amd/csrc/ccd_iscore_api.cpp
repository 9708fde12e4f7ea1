// ccd_iscore_api.cpp - ccd_iscore_* of include/ccd.h: the squared error of many candidates of P / B frames per launch (DESIGN.md
// section 4.19).  A candidate is a frame with the float output of one of its two cool-chics replaced; inter_score_kernel
// (ccd_inter.hip) reconstructs, quantises and scores it without storing a plane.  A reference item (ccd_iscore_add_refs, section 4.22)
// is the frame's base pair against other reference planes.
#include <cstring>
#include <new>

#include "ccd_host.hpp"
#include "ccd_inter_job.hpp"
#include "ccd_iscore_plan.hpp"
#include "ccd_kernels.hpp"

using namespace ccd;

namespace {
struct Frame {
    ccd_iscore_frame in;
    Block buf;                 // [references as 4:4:4 f32][the base pair's warped references]
    float* ref_f32[2] = {};
    float* warped[2] = {};
};
struct Item {
    int frame, role;           // role -1: a reference item
    const float* output;
    int refs = 0;              // a reference item: bit r = reference r is replaced
    const void* planes[2][3] = {};
    Block buf;                 // the replaced references as 4:4:4 f32 (dropped by clear_items / destroy, never by a copy of the entry)
    float* ref_f32[2] = {};
};

// the frame's own pair, which keeps the warps (it: null), or an item: `output` in place of the output of cool-chic `role`, or the
// item's tensors in place of the references it replaces
InterScoreJob make_job(const Frame& f, const Item* it, uint32_t part_first) {
    const int role = it ? it->role : -1, refs = it ? it->refs : 0;
    const float* output = it ? it->output : nullptr;
    InterScoreJob S;
    std::memset(&S, 0, sizeof(S));
    InterUnitJob& J = S.recon;
    const ccd_iscore_frame& in = f.in;
    const bool two = in.frame_type == 2;
    fill_inter_geometry(J, InterFrameDesc{in.h, in.w, in.bitdepth, in.frame_data_type, in.frame_type, in.warp_filter_size, in.global_flow});
    J.residue = role == 0 ? output : in.residue;
    J.motion = role == 1 ? output : in.motion;
    J.ref0 = (refs & 1) ? it->ref_f32[0] : f.ref_f32[0];
    J.ref1 = two ? ((refs & 2) ? it->ref_f32[1] : f.ref_f32[1]) : J.ref0;
    J.w0 = f.warped[0]; J.w1 = f.warped[1];
    J.mode = refs ? iscore_ref_mode(in.frame_type, refs) : (role < 0 ? 0 : (role == 0 ? 1 : 2));
    for (int p = 0; p < 3; ++p) S.src[p] = in.src[p];
    S.part_first = part_first;
    return S;
}
}  // namespace

struct ccd_iscore {
    int device = 0;
    std::vector<std::unique_ptr<Frame>> frames;
    std::vector<Item> items;
    Mirror tables, out;        // job tables (up); uint64 sse[results][3] (down)
    Block part;                // uint64 [workgroups][3]
    std::vector<IScoreSlot> plan;  // of the run in flight / last finished: frames first, then items
    int pending = 0;
    hipStream_t run_stream = nullptr;     // the stream of the run in flight
    int done_frames = 0, done_items = 0;  // what the last finished run covered
    StreamSet streams;
};

extern "C" {

int ccd_iscore_create(int device, ccd_iscore** out) {
    if (!out) return CCD_ERR_ARG;
    *out = nullptr;
    ccd_iscore* s = new (std::nothrow) ccd_iscore();
    if (!s) return CCD_ERR_NOMEM;
    s->device = device;
    *out = s;
    return CCD_OK;
}

void ccd_iscore_destroy(ccd_iscore* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)s->streams.drain();
    for (auto& f : s->frames) f->buf.drop();
    for (auto& it : s->items) it.buf.drop();
    s->tables.drop(); s->out.drop(); s->part.drop();
    delete s;
}

int ccd_iscore_add_frame(ccd_iscore* s, const ccd_iscore_frame* frame) {
    if (!s || !frame || !frame->residue || !frame->motion) return CCD_ERR_ARG;
    if (frame->frame_type < 1 || frame->frame_type > 2 || frame->bitdepth < 8 || frame->bitdepth > 16 || frame->frame_data_type < 0 ||
        frame->frame_data_type > 2)
        return CCD_ERR_ARG;
    for (int p = 0; p < 3; ++p)
        if (!frame->ref0[p] || !frame->src[p] || (frame->frame_type == 2 && !frame->ref1[p])) return CCD_ERR_ARG;
    if (s->pending) return CCD_ERR_ARG;
    if (!warp_filter_ok(frame->warp_filter_size)) return CCD_ERR_VALUE;
    if (frame->h < 1 || frame->w < 1 || frame->h > kIScoreMaxSide || frame->w > kIScoreMaxSide) return CCD_ERR_VALUE;
    if (!yuv420_sides_ok(frame->frame_data_type, frame->h, frame->w)) return CCD_ERR_VALUE;
    std::unique_ptr<Frame> fp(new (std::nothrow) Frame());
    if (!fp) return CCD_ERR_NOMEM;
    fp->in = *frame;
    // ---- the device from here on ----
    HIP_TRY(hipSetDevice(s->device));
    const int n_refs = frame->frame_type == 2 ? 2 : 1;
    const PlaneLayout lay = plane_layout(frame->h, frame->w, frame->bitdepth, frame->frame_data_type);
    if (!fp->buf.get(s->device, BlockPool::kDevice, 2 * n_refs * lay.f32_3)) return CCD_ERR_NOMEM;
    BlockCursor cur(fp->buf);
    for (int r = 0; r < n_refs; ++r) fp->ref_f32[r] = cur.f32(lay);
    for (int r = 0; r < n_refs; ++r) fp->warped[r] = cur.f32(lay);
    s->frames.push_back(std::move(fp));
    return static_cast<int>(s->frames.size()) - 1;
}

int ccd_iscore_add(ccd_iscore* s, int frame, int role, const float* output) {
    if (!s || !output || role < 0 || role > 1 || frame < 0) return CCD_ERR_ARG;
    if (frame >= static_cast<int>(s->frames.size()) || s->pending) return CCD_ERR_ARG;
    if (s->items.size() >= static_cast<size_t>(kIScoreMaxItems)) return CCD_ERR_UNSUPPORTED;
    Item it;
    it.frame = frame; it.role = role; it.output = output;
    s->items.push_back(it);
    return static_cast<int>(s->items.size()) - 1;
}

int ccd_iscore_add_refs(ccd_iscore* s, int frame, const void* const ref0[3], const void* const ref1[3]) {
    if (!s || frame < 0 || frame >= static_cast<int>(s->frames.size()) || (!ref0 && !ref1)) return CCD_ERR_ARG;
    const ccd_iscore_frame& in = s->frames[frame]->in;
    for (int p = 0; p < 3; ++p)
        if ((ref0 && !ref0[p]) || (ref1 && !ref1[p])) return CCD_ERR_ARG;
    if ((ref1 && in.frame_type != 2) || s->pending) return CCD_ERR_ARG;
    if (s->items.size() >= static_cast<size_t>(kIScoreMaxItems)) return CCD_ERR_UNSUPPORTED;
    Item it;
    it.frame = frame; it.role = -1; it.output = nullptr;
    it.refs = (ref0 ? 1 : 0) | (ref1 ? 2 : 0);
    for (int p = 0; p < 3; ++p) { it.planes[0][p] = ref0 ? ref0[p] : nullptr; it.planes[1][p] = ref1 ? ref1[p] : nullptr; }
    // ---- the device from here on ----
    HIP_TRY(hipSetDevice(s->device));
    const PlaneLayout lay = plane_layout(in.h, in.w, in.bitdepth, in.frame_data_type);
    if (!it.buf.get(s->device, BlockPool::kDevice, (it.refs == 3 ? 2 : 1) * lay.f32_3)) return CCD_ERR_NOMEM;
    BlockCursor cur(it.buf);
    for (int r = 0; r < 2; ++r)
        if (it.refs >> r & 1) it.ref_f32[r] = cur.f32(lay);
    s->items.push_back(it);
    return static_cast<int>(s->items.size()) - 1;
}

int ccd_iscore_clear_items(ccd_iscore* s) {
    if (!s || s->pending) return CCD_ERR_ARG;
    for (auto& it : s->items) it.buf.drop();  // (nothing is in flight: the last run's wait synchronised)
    s->items.clear();
    s->done_items = 0;
    return CCD_OK;
}

int ccd_iscore_run(ccd_iscore* s, void* stream) {
    if (!s || s->pending) return CCD_ERR_ARG;
    if (s->frames.empty()) return CCD_OK;
    const size_t n_frames = s->frames.size(), n_items = s->items.size(), n_results = n_frames + n_items;
    std::vector<IScoreGeo> geo(n_frames);
    for (size_t f = 0; f < n_frames; ++f) {
        const ccd_iscore_frame& in = s->frames[f]->in;
        geo[f] = IScoreGeo{in.h, in.w, in.frame_data_type == 1 ? 1 : 0, in.warp_filter_size == 8 ? 1 : 0};
    }
    std::vector<int> item_frame(n_items);
    std::vector<IScoreItemGeo> item_geo(n_items);
    for (size_t i = 0; i < n_items; ++i) { item_frame[i] = s->items[i].frame; item_geo[i] = IScoreItemGeo{s->items[i].frame, s->items[i].refs}; }
    uint32_t class_blocks[kIScoreClasses], total_blocks = 0;
    const int rc = iscore_plan(geo, item_frame, s->plan, class_blocks, &total_blocks);
    if (rc < 0) return rc;
    std::vector<IScoreConv> conv_plan;
    uint32_t conv_blocks = 0;
    const int rc_conv = iscore_plan_conv(geo, item_geo, conv_plan, &conv_blocks);
    if (rc_conv < 0) return rc_conv;
    std::vector<PlanesConvJob> conv(conv_plan.size());
    std::vector<uint32_t> conv_prefix(conv_plan.size() + 1, 0);
    for (size_t k = 0; k < conv_plan.size(); ++k) {
        const IScoreConv& P = conv_plan[k];
        const Item& it = s->items[P.item];
        const ccd_iscore_frame& in = s->frames[it.frame]->in;
        PlanesConvJob& C = conv[k];
        std::memset(&C, 0, sizeof(C));
        for (int p = 0; p < 3; ++p) C.p[p] = it.planes[P.which][p];
        C.out = it.ref_f32[P.which];
        C.h = in.h; C.w = in.w; C.chroma_half = in.frame_data_type == 1; C.wide = in.bitdepth > 8;
        C.tiles_x = inter_tiles_x(in.w, 0);
        C.maxv = static_cast<float>((1 << in.bitdepth) - 1);
        conv_prefix[k] = P.block_first;
        conv_prefix[k + 1] = P.block_first + P.n_blocks;
    }
    std::vector<InterScoreJob> jobs[kIScoreClasses];
    std::vector<InterScoreRange> ranges(n_results);
    for (size_t r = 0; r < n_results; ++r) {
        const IScoreSlot& P = s->plan[r];
        const Item* it = r < n_frames ? nullptr : &s->items[r - n_frames];
        const Frame& f = *s->frames[it ? it->frame : r];
        jobs[P.cls].push_back(make_job(f, it, P.part_first));
        ranges[r] = InterScoreRange{P.part_first, P.n_blocks};
    }
    TableImage img;
    JobLaunch L[kIScoreClasses];
    for (int c = 0; c < kIScoreClasses; ++c) {
        const int rc_c = put_job_launch(img, jobs[c], L[c]);  // (its workgroups are the plan's class_blocks[c]: both are inter_blocks)
        if (rc_c < 0) return rc_c;
    }
    const size_t off_ranges = img.put(ranges), off_conv = img.put(conv), off_conv_prefix = img.put(conv_prefix);
    // ---- the device from here on ----
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // nothing of an earlier run is in flight (its wait synchronised), so the blocks may be exchanged for larger ones
    if (!s->tables.ensure(s->device, img.bytes.size()) || !s->out.ensure(s->device, n_results * 3 * sizeof(uint64_t)) ||
        !s->part.ensure(s->device, BlockPool::kDevice, std::max<size_t>(256, static_cast<size_t>(total_blocks) * 3 * sizeof(uint64_t))))
        return CCD_ERR_NOMEM;
    std::memcpy(s->tables.host.p, img.bytes.data(), img.bytes.size());
    s->streams.note(st);
    HIP_TRY(s->tables.upload(img.bytes.size(), st));
    for (const auto& fp : s->frames) {  // the references as the warp reads them
        const ccd_iscore_frame& in = fp->in;
        for (int r = 0; r < (in.frame_type == 2 ? 2 : 1); ++r) {
            const void* const* pl = r ? in.ref1 : in.ref0;
            HIP_TRY(launch_planes_to_444(pl[0], pl[1], pl[2], fp->ref_f32[r], in.h, in.w, in.bitdepth, in.frame_data_type, st));
        }
    }
    for (int c = 0; c < kIScoreClasses; ++c) {  // the base pairs first: residue and one-reference items read the warps they keep
        if (c == 2)  // the replaced references of all reference items as the warp reads them, one launch
            HIP_TRY(launch_planes_to_444_jobs(s->tables.dev_at<PlanesConvJob>(off_conv), s->tables.dev_at<uint32_t>(off_conv_prefix),
                                              static_cast<int>(conv.size()), conv_blocks, st));
        HIP_TRY(launch_inter_score(s->tables.dev_at<InterScoreJob>(L[c].jobs), s->tables.dev_at<uint32_t>(L[c].prefix), L[c].n_jobs, L[c].n_blocks, c & 1,
                                   s->part.as<uint64_t>(), st));
    }
    HIP_TRY(launch_inter_score_final(s->tables.dev_at<InterScoreRange>(off_ranges), static_cast<int>(n_results), s->part.as<uint64_t>(),
                                     s->out.dev.as<uint64_t>(), st));
    HIP_TRY(s->out.download(n_results * 3 * sizeof(uint64_t), st));
    s->pending = 1;
    s->run_stream = st;
    return CCD_OK;
}

int ccd_iscore_wait(ccd_iscore* s, void* stream) {
    if (!s) return CCD_ERR_ARG;
    if (!s->pending) return CCD_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    // the results are behind the run on the stream the run was given, whichever stream this call names
    if (s->run_stream != static_cast<hipStream_t>(stream)) HIP_TRY(hipStreamSynchronize(s->run_stream));
    s->pending = 0;
    s->done_frames = static_cast<int>(s->frames.size());
    s->done_items = static_cast<int>(s->items.size());
    return CCD_OK;
}

static int iscore_result(const ccd_iscore* s, const ccd_iscore_frame& in, size_t r, uint64_t* sse, uint64_t* n) {
    const uint64_t* out = s->out.host.as<uint64_t>() + r * 3;
    const uint64_t luma = static_cast<uint64_t>(in.h) * in.w;
    const uint64_t chroma = in.frame_data_type == 1 ? static_cast<uint64_t>(in.h / 2) * (in.w / 2) : luma;
    for (int p = 0; p < 3; ++p) { sse[p] = out[p]; n[p] = p ? chroma : luma; }
    return CCD_OK;
}

int ccd_iscore_frame_result(const ccd_iscore* s, int frame, uint64_t* sse, uint64_t* n) {
    if (!s || !sse || !n || frame < 0) return CCD_ERR_ARG;
    if (s->pending || frame >= s->done_frames) return CCD_ERR_ARG;
    return iscore_result(s, s->frames[frame]->in, frame, sse, n);
}

int ccd_iscore_result(const ccd_iscore* s, int item, uint64_t* sse, uint64_t* n) {
    if (!s || !sse || !n || item < 0) return CCD_ERR_ARG;
    if (s->pending || item >= s->done_items) return CCD_ERR_ARG;
    // (frames added after the run sit behind the items of the finished run in no table: the run's own frame count places the item)
    return iscore_result(s, s->frames[s->items[item].frame]->in, static_cast<size_t>(s->done_frames) + item, sse, n);
}

}  // extern "C"
